"""The batched error-target loop against the sequential one on the CPU oracle: no GPU.

  python tools/batch_oracle.py [--size 96x72] [--seeds 77,78,79] [--log profiles/batch_target.log]

cornell_box, abs_tol 0.04, first 16 (two full 8-spp passes), pass_spp 16, max_spp 496, truth a 4096-spp frame of seed
999. A pass of a pixel depends on its seed and the pixel alone, so every pass k is rendered once as a full oracle frame
with pass_seed(seed, k) and the loops gather their pixels from it; the accumulator, the selection, the plan and the run
merge are the numpy restatements the GPU tests compare the device against bit for bit (tests/adapt_ref.py,
tests/batch_ref.py). The sequential loop is render_to_error(batch=0); the batched loop render_to_error(batch=C, gain)
over the grid gain in {0.25, 0.5, 1} x C in {4, 8, 16}. Per run: render launches after the two full passes, mean spp,
max spp, linear RMSE against the truth. These figures choose rt_amd.ERROR_TARGET_BATCH_DEFAULTS and the bounds of
tests/test_gpu_batch.py::test_end_to_end.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import accum_ref as aref  # noqa: E402
import adapt_ref as dref  # noqa: E402
import batch_ref as br  # noqa: E402
import oracle_bind  # noqa: E402

ABS_TOL, FIRST, PASS_SPP, MAX_SPP = 0.04, 16, 16, 496
GAINS, BATCHES = (0.25, 0.5, 1.0), (4, 8, 16)


class Passes:
    """Pass k of the frame, rendered on demand: (sub[h, w, 4, 3], n)."""

    def __init__(self, scene, w, h, seed):
        self.scene, self.w, self.h, self.seed, self.cache = scene, w, h, seed, {}

    def __call__(self, k):
        if k not in self.cache:
            spp = FIRST // 2 if k < 2 else PASS_SPP
            self.cache[k] = self.scene.render(self.w, self.h, spp, aref.pass_seed(self.seed, k))[1]
        return self.cache[k]


def _start(passes, w, h):
    acc = dref.Accum(w, h)
    for k in range(2):
        acc.add_sub(passes(k), FIRST // 2 // 4)
    return acc


def sequential(passes, w, h, limit=None):
    """render_to_error(batch=0): (launches, accumulator)."""
    acc, k, n, max_n = _start(passes, w, h), 2, PASS_SPP // 4, MAX_SPP // 4
    while limit is None or k - 2 < limit:
        ids = dref.select(acc, ABS_TOL, 0.0, max_n)
        if ids.size == 0:
            break
        acc.add_sub_pixels(ids, dref.gather(passes(k), ids), n)
        k += 1
    return k - 2, acc


def batched(passes, w, h, C, gain):
    """render_to_error(batch=C, gain=gain): (launches, passes used in all, accumulator)."""
    acc, k, n, max_n, launches = _start(passes, w, h), 2, PASS_SPP // 4, MAX_SPP // 4, 0
    while True:
        ids, counts, units, used = br.plan(acc, ABS_TOL, 0.0, max_n, n, gain, C)
        if ids.size == 0:
            break
        off = br.offsets(counts)
        m = np.zeros((units, 4, 3))
        for i in range(used):
            has = counts > i
            m[off[has] + i] = dref.gather(passes(k + i), ids[has])
        br.add_runs(acc, ids, counts, m, n)
        k += used
        launches += 1
    return launches, k - 2, acc


def _stats(acc, truth):
    n_p = acc.counts()[1].astype(np.float64)
    rmse = float(np.sqrt(np.mean((aref.c_of(acc.sub()) - truth) ** 2)))
    return 4.0 * n_p.mean(), 4.0 * n_p.max(), rmse


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="96x72")
    ap.add_argument("--seeds", default="77,78,79")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "batch_target.log"))
    args = ap.parse_args()
    w, h = (int(x) for x in args.size.lower().split("x"))
    seeds = [int(x) for x in args.seeds.split(",")]
    out = open(args.log, "w")

    def log(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    scene = oracle_bind.OracleScene(os.path.join(REPO, "scenes", "cornell_box.toml"))
    truth = aref.c_of(scene.render(w, h, 4096, 999)[1])
    log(f"# batch_oracle: cornell_box {w}x{h} on the CPU oracle, abs_tol {ABS_TOL}, first {FIRST}, pass_spp {PASS_SPP}, "
        f"max_spp {MAX_SPP}, seeds pass_seed(seed, k); truth: 4096 spp, seed 999")
    log("seed  loop        C  gain  launches  passes  mean spp  max spp  linear RMSE")
    seq, grid = [], {}
    for seed in seeds:
        passes = Passes(scene, w, h, seed)
        launches, acc = sequential(passes, w, h)
        s = _stats(acc, truth)
        seq.append((launches,) + s)
        log(f"{seed:4d}  sequential  -     -  {launches:8d}  {launches:6d}  {s[0]:8.2f}  {s[1]:7.0f}  {s[2]:.6f}")
        for gain in GAINS:
            for C in BATCHES:
                launches, used, acc = batched(passes, w, h, C, gain)
                s = _stats(acc, truth)
                grid.setdefault((C, gain), []).append((launches,) + s)
                log(f"{seed:4d}  batched    {C:2d}  {gain:4.2f}  {launches:8d}  {used:6d}  {s[0]:8.2f}  {s[1]:7.0f}  {s[2]:.6f}")
    seq = np.array(seq)
    spread_spp, spread_rmse = float(seq[:, 1].max() - seq[:, 1].min()), float(seq[:, 3].max() - seq[:, 3].min())
    log()
    log(f"sequential over the seeds: launches {seq[:, 0].min():.0f} .. {seq[:, 0].max():.0f}, mean spp "
        f"{seq[:, 1].min():.2f} .. {seq[:, 1].max():.2f} (spread {spread_spp:.2f}), RMSE {seq[:, 3].min():.6f} .. "
        f"{seq[:, 3].max():.6f} (spread {spread_rmse:.6f})")
    log("C   gain  launches (max)  mean spp - sequential (worst seed)  RMSE - sequential (worst seed)  within the spread")
    best = None
    for (C, gain), rows in sorted(grid.items()):
        rows = np.array(rows)
        d_spp = float((rows[:, 1] - seq[:, 1]).max())
        d_rmse = float((rows[:, 3] - seq[:, 3]).max())
        ok = d_spp <= spread_spp and d_rmse <= spread_rmse
        log(f"{C:2d}  {gain:4.2f}  {rows[:, 0].max():14.0f}  {d_spp:+35.2f}  {d_rmse:+30.6f}  {'yes' if ok else 'no'}")
        if ok and (best is None or rows[:, 0].max() < best[0]):
            best = (rows[:, 0].max(), C, gain)
    log("fewest launches within the spread: " + (f"C = {best[1]}, gain = {best[2]} ({best[0]:.0f} launches)" if best
                                                 else "none"))


if __name__ == "__main__":
    main()
