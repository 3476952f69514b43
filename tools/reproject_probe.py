"""Measurements of DESIGN.md §14 on one MI355X: rt_accum_reproject beside a 4-spp rt_accum_add pass and beside the
merge kernel's traffic, and the equal-time RMSE after a camera move with and without the reprojected history.

Usage: python tools/reproject_probe.py [--width 1920 --height 1080] [--scenes cornell_box,cubes,flying_unicorn]
Times are host clocks around calls that wait for the device (every rt_accum_* call does), after a warm-up call,
best and median of --reps."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracer-server_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

MOVE_A = dict(dpos=(14.0, 6.0, -40.0), ddir=(-0.10, -0.05, 0.0))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), statistics.median(ts)


def colour(sub):
    return np.clip(sub, 0.0, 1.0).mean(axis=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="cornell_box,cubes,flying_unicorn")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    a = ap.parse_args()
    import ctypes

    import torch

    import rt_amd as rt

    w, h, npix = a.width, a.height, a.width * a.height
    print(f"# {w} x {h}, reps {a.reps}, times in ms as best / median")
    for name in a.scenes.split(","):
        base = rt.Scene.from_toml(os.path.join(REPO, "scenes", f"{name}.toml"))
        cam = base.camera()
        view = base.view(tuple(p + d for p, d in zip(cam["pos"], MOVE_A["dpos"])),
                         tuple(p + d for p, d in zip(cam["dir"], MOVE_A["ddir"])))
        seeds = (rt.pass_seed(a.seed, k) for k in range(1 << 20))
        with rt.Accumulator(w, h) as src, rt.Accumulator(w, h) as dst, rt.Accumulator(w, h) as empty:
            for _ in range(16):
                src.add(base, 16, next(seeds))
            # a 4-spp full-frame pass (render + merge), the merge alone, the reprojection
            t_pass = timed(lambda: empty.add(view, 4, next(seeds)), a.reps)
            d_sub = torch.rand(npix * 12, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            t_merge = timed(lambda: rt._check(rt.lib.rt_accum_add_sub_device(
                empty.handle, ctypes.c_void_p(d_sub.data_ptr()), 1, None)), a.reps)
            n_valid = [0]

            def reproject():
                n_valid[0] = dst.reproject_from(src, view, base, 64)

            t_rep = timed(reproject, a.reps)
            nv = n_valid[0]
            b_merge = npix * 480                    # m read, S and Q read and written
            b_rep = nv * 4 * 48 + npix * (192 + 8)  # 6 doubles gathered per valid subpixel; S, Q and counts written
            print(f"{name}: valid {nv / npix:.3f}; rt_accum_add 4 spp {t_pass[0]:.2f} / {t_pass[1]:.2f}; "
                  f"rt_accum_reproject {t_rep[0]:.2f} / {t_rep[1]:.2f} ({t_rep[0] / t_pass[0]:.2f} passes); "
                  f"merge alone (rt_accum_add_sub_device) {t_merge[0]:.2f} / {t_merge[1]:.2f}")
            print(f"{name}: bytes/s of the accumulator traffic: reproject {b_rep / t_rep[0] / 1e6:.1f} GB/s "
                  f"({b_rep / 1e6:.0f} MB), merge call {b_merge / t_merge[0] / 1e6:.1f} GB/s ({b_merge / 1e6:.0f} MB)")
            # equal time after the move: history + two 4-spp passes against as many 4-spp passes as fit in that time
            t_hist = t_rep[0] + 2 * t_pass[0]
            n_equal = max(2, int(round(t_hist / t_pass[0])))
            ref = colour(rt.render(view, w, h, a.ref_spp, 0xC0FFEE, megakernel=True, want_sub=True)[1])
            empty.reset()
            new = [next(seeds) for _ in range(n_equal)]
            for s in new[:2]:
                dst.add(view, 4, s)
            for s in new:
                empty.add(view, 4, s)
            valid = dst.counts()[1] > 2
            c_h, c_e = colour(dst.resolve()[0]), colour(empty.resolve()[0])
            rm = lambda c, m: float(np.sqrt(((c - ref)[m] ** 2).mean()))
            every = np.ones_like(valid)
            print(f"{name}: equal time {t_hist:.2f} ms: history + 2 x 4 spp RMSE {rm(c_h, every):.5f} (valid pixels "
                  f"{rm(c_h, valid):.5f}, others {rm(c_h, ~valid):.5f}); {n_equal} x 4 spp from empty RMSE "
                  f"{rm(c_e, every):.5f} (valid pixels {rm(c_e, valid):.5f}, others {rm(c_e, ~valid):.5f}); "
                  f"reference {a.ref_spp} spp", flush=True)


if __name__ == "__main__":
    main()
