"""Measurements of DESIGN.md §15: after a reprojection, two full-frame passes (the flow of §14) against
Accumulator.fill, which samples only the pixels without history (and a refresh pattern).

  python tools/fill_probe.py quality [--scenes ...] [--orbit 8] [--out profiles/fill_quality.log]
      CPU only: the oracle renders the passes, tests/reproject_ref.py reprojects, tests/fill_ref.py fills. §14's
      set-up: 96 x 72, src holds 16 passes of 16 spp, max_n = 64, moves A and B, the three scenes. Per flow: camera
      samples per view and the linear RMSE of the pixel colour against a 1024-spp frame of the view over all / valid /
      hole pixels; then the same over an orbit of --orbit views, each reprojected from the one before.
  python tools/fill_probe.py time [--width 1920 --height 1080] [--flows full,8/0,16/0,16/4] [--out profiles/fill_probe.log]
      One MI355X: the per-view time (reprojection + passes) of both flows, §14's protocol: host clocks around calls
      that wait for the device, one warm-up, best and median of --reps; and the RMSE against a --ref-spp frame.
      --flows keeps only the named rows (full: the two full passes; F/R: fill F spp, refresh R), as DESIGN.md §16's re-run.
A list render of seed s is the full frame's render of seed s at the listed pixels (rt_render_pixels' contract), so the
CPU study renders every pass once as a full frame and gathers."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracer-server_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

W, H, MAX_N, SEED, REF_SEED = 96, 72, 64, 0x5EED, 0xC0FFEE
FILL_SPP, REFRESH = (4, 8, 16), (0, 1, 2, 4)
ORBIT_STEP = dict(dpos=(4.0, 1.5, -6.0), ddir=(-0.02, -0.008, 0.0))  # per view, relative to the scene's camera
PASS_SEED_STEP = 0x9E3779B97F4A7C15


def pass_seed(seed, k):
    return (seed + k * PASS_SEED_STEP) % (1 << 64)


def flows():
    yield "two full 4-spp passes", None
    for f in FILL_SPP:
        for r in REFRESH:
            yield f"fill {f} spp, refresh {r}", (f, r)


class Tee:
    def __init__(self, path):
        self.f = open(path, "w") if path else None

    def __call__(self, *a):
        line = " ".join(str(x) for x in a)
        print(line, flush=True)
        if self.f:
            self.f.write(line + "\n")
            self.f.flush()


# quality (CPU) ------------------------------------------------------------------------------------------------

class CpuView:
    """A view of a scene for the oracle: the scene's text with the view's camera, and a cache of full-frame passes."""

    def __init__(self, ob, rr, path, view, tmp):
        moved, assets = rr.moved_toml(path, view, tmp)
        self.view = view
        self.scene = ob.OracleScene(moved, assets_dir=assets)
        self.cache = {}

    def render(self, spp, seed):
        if (spp, seed) not in self.cache:
            self.cache[spp, seed] = self.scene.render(W, H, spp, seed)[1]
        return self.cache[spp, seed]


def rmse_split(rr, sub, ref, valid):
    d = (rr.pixel_colour(sub) - rr.pixel_colour(ref)) ** 2
    f = lambda m: float(np.sqrt(d[m].mean())) if m.any() else float("nan")
    return f(np.ones_like(valid)), f(valid), f(~valid)


def step(rr, fr, c, src_acc, dst, flow, k, view_index):
    """One view of a flow: reproject src_acc into the view `dst` (a CpuView; c = reproject_ref.classify of the two
    views), then the flow's passes with the seeds pass_seed(SEED, k), pass_seed(SEED, k + 1). Returns (accumulator,
    valid mask, camera samples)."""
    S, Q, K, N, _ = rr.reproject(src_acc.S, src_acc.Q, src_acc.K, src_acc.N, c, MAX_N)
    acc = fr.Accum(W, H)
    acc.seed(S, Q, K, N)
    valid = N > 0
    seeds = (pass_seed(SEED, k), pass_seed(SEED, k + 1))
    if flow is None:
        for s in seeds:
            acc.add_sub(dst.render(4, s), 1)
        return acc, valid, 2 * 4 * W * H
    f, r = flow
    lens = acc.fill(lambda kk, ids: dst.render(f, seeds[kk]).reshape(-1, 4, 3)[ids], f // 4, r,
                    view_index % r if r > 0 else 0)
    return acc, valid, sum(lens) * f


def quality(a):
    import fill_ref as fr
    import oracle_bind as ob
    import reproject_ref as rr

    log = Tee(a.out)
    log(f"# CPU study: {W} x {H}, src 16 passes of 16 spp, max_n {MAX_N}, reference {a.ref_spp} spp; linear RMSE of the "
        "pixel colour over all / valid / hole pixels; samples = camera samples traced for the view")
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            t0 = time.time()
            path = os.path.join(REPO, "scenes", f"{name}.toml")
            kinds = rr.brdf_kinds(path)
            v0 = rr.scene_view(path)
            base = CpuView(ob, rr, path, v0, tmp)
            src = fr.Accum(W, H)
            for k in range(16):
                src.add_sub(base.render(16, pass_seed(SEED, k)), 4)
            base.cache.clear()
            for mv, move in (("A", rr.MOVE_A), ("B", rr.MOVE_B)):
                dst = CpuView(ob, rr, path, rr.scene_view(path, move), tmp)
                ref = dst.scene.render(W, H, a.ref_spp, REF_SEED)[1]
                c = rr.classify(base.scene, kinds, dst.view, v0, W, H)
                for label, flow in flows():
                    acc, valid, samples = step(rr, fr, c, src, dst, flow, 16, 1)
                    e = rmse_split(rr, acc.sub(), ref, valid)
                    log(f"{name} move {mv} valid {valid.mean():.3f} | {label} | samples {samples} "
                        f"({samples / (W * H):.2f} per pixel) | RMSE {e[0]:.4f} / {e[1]:.4f} / {e[2]:.4f}")
            # the orbit: every flow carries its own accumulator from view to view
            n_views = a.orbit
            views = [rr.scene_view(path, dict(dpos=tuple(i * x for x in ORBIT_STEP["dpos"]),
                                              ddir=tuple(i * x for x in ORBIT_STEP["ddir"]))) for i in range(n_views + 1)]
            state = {label: (src, 0) for label, _ in flows()}
            rows = {label: [] for label, _ in flows()}
            prev = base
            for i in range(1, n_views + 1):
                dst = CpuView(ob, rr, path, views[i], tmp)
                ref = dst.scene.render(W, H, a.ref_spp, REF_SEED)[1]
                c = rr.classify(base.scene, kinds, dst.view, prev.view, W, H)
                for label, flow in flows():
                    acc, valid, samples = step(rr, fr, c, state[label][0], dst, flow, 16 + 2 * (i - 1), i)
                    state[label] = (acc, state[label][1] + samples)
                    rows[label].append(rmse_split(rr, acc.sub(), ref, valid) + (float(valid.mean()),))
                prev = dst
            for label, _ in flows():
                alls = " ".join(f"{e[0]:.4f}" for e in rows[label])
                last = rows[label][-1]
                log(f"{name} orbit of {n_views} | {label} | samples per view {state[label][1] / n_views / (W * H):.2f} "
                    f"per pixel | RMSE all pixels, view 1..{n_views}: {alls} | last view valid {last[3]:.3f}: "
                    f"{last[0]:.4f} / {last[1]:.4f} / {last[2]:.4f}")
            log(f"# {name}: {time.time() - t0:.0f} s")


# time (GPU) ---------------------------------------------------------------------------------------------------

def gpu_time(a):
    import rt_amd as rt

    log = Tee(a.out)
    w, h, npix = a.width, a.height, a.width * a.height
    move = dict(dpos=(14.0, 6.0, -40.0), ddir=(-0.10, -0.05, 0.0))
    colour = lambda sub: np.clip(sub, 0.0, 1.0).mean(axis=2)
    log(f"# {w} x {h}, move A, src 16 passes of 16 spp, max_n {MAX_N}, reps {a.reps}; per-view time = "
        "rt_accum_reproject + the flow's passes, host clocks around calls that wait for the device, one warm-up, "
        f"ms as best / median; RMSE against {a.ref_spp} spp over all / valid / hole pixels")
    for name in a.scenes.split(","):
        base = rt.Scene.from_toml(os.path.join(REPO, "scenes", f"{name}.toml"))
        cam = base.camera()
        view = base.view(tuple(p + d for p, d in zip(cam["pos"], move["dpos"])),
                         tuple(p + d for p, d in zip(cam["dir"], move["ddir"])))
        ref = colour(rt.render(view, w, h, a.ref_spp, REF_SEED, megakernel=True, want_sub=True)[1])
        with rt.Accumulator(w, h) as src, rt.Accumulator(w, h) as dst:
            for k in range(16):
                src.add(base, 16, pass_seed(SEED, k))
            s1, s2 = pass_seed(SEED, 16), pass_seed(SEED, 17)
            dst.reproject_from(src, view, base, MAX_N)
            hist = dst.counts()[1] > 0  # the pixels that receive history
            keep = set(a.flows.split(",")) if a.flows else None
            for label, flow in flows():
                if keep is not None and ("full" if flow is None else f"{flow[0]}/{flow[1]}") not in keep:
                    continue
                t_rep, t_fill, lens = [], [], (npix, npix)
                for rep in range(a.reps + 1):
                    t0 = time.perf_counter()
                    n_valid = dst.reproject_from(src, view, base, MAX_N)
                    t1 = time.perf_counter()
                    if flow is None:
                        dst.add(view, 4, s1)
                        dst.add(view, 4, s2)
                    else:
                        lens = dst.fill(view, flow[0], s1, s2, period=flow[1], phase=1 % flow[1] if flow[1] else 0)["fill"]
                    t2 = time.perf_counter()
                    if rep > 0:  # the first round is the warm-up
                        t_rep.append((t1 - t0) * 1e3)
                        t_fill.append((t2 - t1) * 1e3)
                sub = dst.resolve()[0]
                spp = 4 if flow is None else flow[0]
                d = (colour(sub) - ref) ** 2
                rm = lambda m: float(np.sqrt(d[m].mean())) if m.any() else float("nan")
                view_ms = [x + y for x, y in zip(t_rep, t_fill)]
                log(f"{name} valid {n_valid / npix:.3f} | {label} | lists {lens[0]} + {lens[1]} "
                    f"({(lens[0] + lens[1]) * spp / npix:.2f} samples per pixel) | reproject {min(t_rep):.2f} / "
                    f"{statistics.median(t_rep):.2f} | passes {min(t_fill):.2f} / {statistics.median(t_fill):.2f} | "
                    f"view {min(view_ms):.2f} / {statistics.median(view_ms):.2f} | RMSE {rm(np.ones_like(hist)):.4f} / "
                    f"{rm(hist):.4f} / {rm(~hist):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("quality", "time"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="cornell_box,cubes,flying_unicorn")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--orbit", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--flows", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "quality":
        quality(a)
    else:
        gpu_time(a)


if __name__ == "__main__":
    main()
