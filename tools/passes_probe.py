"""What a batched render of a mesh scene costs per kernel family, on the GPU.

  python tools/passes_probe.py [--size 1920x1080] [--reps 15] [--scenes cubes,flying_unicorn] [--log profiles/...]
      tools/adapt_probe.py time's protocol at 16 spp: HIP events (torch.cuda.Event on the stream the calls are enqueued
      on) in one process, 3 warm-up rounds, the median of --reps rounds, every row's call once per round in turn:
      rt_render_device of the full frame; rt_render_pixels_with_device of every pixel through the scene's pool; and
      rt_render_pixel_passes_with_device through the pool and through the fused body (RT_LIST_FUSED) for two lists of a
      frame's worth of unit-groups: every pixel once, and every 2nd pixel with two passes. The passes form expands its
      list on the device and waits for the render, so its rows hold the expansion (a scan and a write) as well.
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

import torch  # before rt_amd, as bench.py: the process's HIP runtime is the one torch brings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracer-server_amd"))
import rt_amd  # noqa: E402

V = ctypes.c_void_p
FAMILY_NAMES = {rt_amd.LIST_FUSED: "fused", rt_amd.LIST_FPOOL: "fpool", rt_amd.LIST_ROLES: "roles"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--scenes", default="cubes,flying_unicorn")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "batch_pool_families.log"))
    args = ap.parse_args()
    if rt_amd.device_count() < 1:
        raise RuntimeError("passes_probe: no HIP device visible (it measures on the GPU only)")
    w, h = (int(x) for x in args.size.lower().split("x"))
    npix, spp = w * h, 16
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    out = open(args.log, "w")

    def log(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    st = V(stream) if stream else None
    every = torch.arange(npix, dtype=torch.int32, device=dev)
    half = torch.arange(0, npix, 2, dtype=torch.int32, device=dev)
    ones = torch.ones(npix, dtype=torch.uint8, device=dev)
    twos = torch.full((half.numel(),), 2, dtype=torch.uint8, device=dev)
    lsub = torch.zeros(npix * 12, dtype=torch.float64, device=dev)
    rgb = torch.zeros(npix * 3, dtype=torch.uint8, device=dev)
    seeds = np.array([rt_amd.pass_seed(77, 2), rt_amd.pass_seed(77, 3)], dtype=np.uint64)
    sd = seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    log(f"# passes_probe: {w}x{h}, {spp} spp, median of {args.reps} rounds after 3 warm-up rounds, HIP events, one process")
    log("scene            call                                       family  unit-groups      ms  over the frame")
    for name in args.scenes.split(","):
        sc = rt_amd.Scene.from_toml(os.path.join(REPO, "scenes", f"{name}.toml"))
        pool = rt_amd.render_pixels_path(sc, w, h, spp, npix)[1]
        p = rt_amd.make_params(w, h, spp, int(seeds[0]), None, rt_amd.FLAG_MEGAKERNEL, 0, 1)

        def frame():
            rt_amd._check(rt_amd.lib.rt_render_device(sc.handle, ctypes.byref(p), V(rgb.data_ptr()), None, st, None))

        def plist():
            rt_amd._check(rt_amd.lib.rt_render_pixels_with_device(sc.handle, ctypes.byref(p), V(every.data_ptr()), npix, pool,
                                                                  None, V(lsub.data_ptr()), st, None))

        def passes(ids, counts, n_seeds, fam):
            def run():
                rt_amd._check(rt_amd.lib.rt_render_pixel_passes_with_device(
                    sc.handle, ctypes.byref(p), V(ids.data_ptr()), V(counts.data_ptr()), ids.numel(),
                    ids.numel() * n_seeds, sd, n_seeds, fam, None, V(lsub.data_ptr()), st, None))
            return run

        rows = [("rt_render_device, full frame", "", npix, frame),
                ("rt_render_pixels_with_device, every pixel", FAMILY_NAMES[pool], npix, plist)]
        for fam in (pool, rt_amd.LIST_FUSED):
            rows.append(("passes, every pixel once", FAMILY_NAMES[fam], npix, passes(every, ones, 1, fam)))
            rows.append(("passes, every 2nd pixel twice", FAMILY_NAMES[fam], half.numel() * 2, passes(half, twos, 2, fam)))
        ms = [[] for _ in rows]
        for rep in range(3 + args.reps):
            for i, (_, _, _, fn) in enumerate(rows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 3:
                    ms[i].append(e0.elapsed_time(e1))
        t_frame = statistics.median(ms[0])
        for (what, fam, units, _), m in zip(rows, ms):
            t = statistics.median(m)
            log(f"{name:16s} {what:42s} {fam:6s} {units:12d} {t:8.2f}  {t / t_frame:6.3f}")


if __name__ == "__main__":
    main()
