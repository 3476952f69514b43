"""Cost and quality of the denoised previews on the GPU.

  python tools/denoise_probe.py time  [--sizes 600x450,1920x1080] [--reps 30] [--log profiles/denoise_probe.log]
      Per scene and size, HIP events (torch.cuda.Event on the stream the calls are enqueued on) around, after a
      warm-up of every shape and as the median of --reps calls: rt_render_device at 16 spp (the plain frame: unchanged
      product code), rt_render_features_device, and rt_denoise_device at levels 0 .. L (L = DENOISE_DEFAULTS levels,
      same sigmas, RGB8 output only). Level i >= 1 is the difference T(i + 1) - T(i) and is given as GB/s against the
      minimum traffic of 64 B per pixel (48 read, 16 written); T(1) holds level 0 together with the c0 and RGB8
      passes, which only a kernel trace separates (the `trace` mode). The ratio reported is
      (features + denoise at L levels) / (16-spp render).
  python tools/denoise_probe.py run SCENE WxH [calls]
      Just the calls (one warm-up, then `calls` x rt_denoise_device at L levels), for
      `rocprofv3 --kernel-trace --output-format csv -- python tools/denoise_probe.py run ...`.
  python tools/denoise_probe.py trace KERNEL_TRACE_CSV WxH [--log FILE]
      Per-kernel times of such a trace: k_atrous_init, each k_atrous_level in launch order, k_atrous_out (median over
      the calls after the warm-up), each level as GB/s against 64 B per pixel.
  python tools/denoise_probe.py grid [--log profiles/denoise_grid.log]
      The grid DENOISE_DEFAULTS were picked from: linear RMSE of the denoised 96 x 72, 16-spp frame against a
      1024-spp frame of another seed, over the noisy frame's, per scene and grid point.
  python tools/denoise_probe.py var-grid [--log profiles/denoise_var_grid.log]
      The grid DENOISE_VAR_DEFAULTS were picked from: 96 x 72, accumulated frames of 2 x 8, 4 x 16 and
      8 x 128 spp, linear RMSE of rt_denoise_var's frame against a 4096-spp frame of another seed over the noisy
      frame's, per scene, sample count and grid point, beside rt_denoise's with DENOISE_DEFAULTS.
  python tools/denoise_probe.py var-time [--sizes 600x450,1920x1080] [--reps 30] [--log profiles/denoise_var_time.log]
      HIP events in one process around rt_accum_add_sub_device, rt_accum_resolve_device, rt_render_device at 16 spp and
      rt_denoise_var_device / rt_denoise_device at levels 0 .. L; the two streaming kernels as a share of the
      achievable HBM rate, the new level kernel against k_atrous_level.
"""
import argparse
import csv
import ctypes
import itertools
import os
import statistics
import sys

import numpy as np

import torch  # before rt_amd, as bench.py: the process's HIP runtime is the one torch brings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracer-server_amd"))
import rt_amd  # noqa: E402

SCENES = ("cornell_box", "cubes", "flying_unicorn")
MIN_BYTES_PER_PIXEL = 64  # a level reads colour (16) + features (32) and writes colour (16)


class Log:
    def __init__(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.f = open(path, "w")

    def __call__(self, line=""):
        print(line, flush=True)
        self.f.write(line + "\n")
        self.f.flush()


def _scene(name):
    return rt_amd.Scene.from_toml(os.path.join(REPO, "scenes", f"{name}.toml"))


def _size(s):
    w, h = s.lower().split("x")
    return int(w), int(h)


class DeviceFrame:
    """Device buffers of one frame (torch tensors) and the three calls on torch's current stream."""

    def __init__(self, scene, w, h, spp=16):
        if rt_amd.device_count() < 1:
            raise RuntimeError("denoise_probe: no HIP device visible (it measures on the GPU only)")
        torch.cuda.set_device(0)
        self.torch = torch
        self.scene, self.w, self.h = scene, w, h
        self.params = rt_amd.make_params(w, h, spp, 0x5EED, None, rt_amd.FLAG_MEGAKERNEL, 0, 1)
        dev = torch.device("cuda:0")
        self.sub = torch.zeros(w * h * 12, dtype=torch.float64, device=dev)
        self.feat = torch.zeros(w * h * 8, dtype=torch.float32, device=dev)
        self.rgb = torch.zeros(w * h * 3, dtype=torch.uint8, device=dev)
        self.rgb2 = torch.zeros(w * h * 3, dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.sig = [float(rt_amd.DENOISE_DEFAULTS[k]) for k in ("sigma_c", "sigma_n", "sigma_z", "sigma_a")]

    def render(self):
        rt_amd.render_device(self.scene, self.params, self.rgb.data_ptr(), self.sub.data_ptr(), self.stream)

    def features(self):
        rt_amd._check(rt_amd.lib.rt_render_features_device(self.scene.handle, ctypes.byref(self.params),
                                                           ctypes.c_void_p(self.feat.data_ptr()),
                                                           ctypes.c_void_p(self.stream) if self.stream else None))

    def denoise(self, levels):
        V = ctypes.c_void_p
        rt_amd._check(rt_amd.lib.rt_denoise_device(0, self.w, self.h, V(self.sub.data_ptr()), V(self.feat.data_ptr()),
                                                   levels, *self.sig, V(self.rgb2.data_ptr()), None,
                                                   V(self.stream) if self.stream else None))

    def timed(self, fn, reps, warm=3):
        """Median and spread (ms) of `fn` between two events on the stream."""
        torch = self.torch
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)


def cmd_time(args):
    log = Log(args.log)
    L = rt_amd.DENOISE_DEFAULTS["levels"]
    log(f"denoise_probe time: reps {args.reps} (median [min, max] ms, HIP events), levels {L}, "
        f"defaults {rt_amd.DENOISE_DEFAULTS}")
    for name in SCENES:
        scene = _scene(name)
        for w, h in args.sizes:
            f = DeviceFrame(scene, w, h)
            r = f.timed(f.render, args.reps)
            ft = f.timed(f.features, args.reps)
            T = [f.timed(lambda k=k: f.denoise(k), args.reps) for k in range(L + 1)]
            npix = w * h
            log(f"{name} {w}x{h}: render 16 spp {r[0]:.3f} [{r[1]:.3f}, {r[2]:.3f}]  features {ft[0]:.3f} "
                f"[{ft[1]:.3f}, {ft[2]:.3f}]")
            for k, t in enumerate(T):
                log(f"  denoise levels={k}: {t[0]:.3f} [{t[1]:.3f}, {t[2]:.3f}]")
            for i in range(1, L):
                d = T[i + 1][0] - T[i][0]
                gbs = npix * MIN_BYTES_PER_PIXEL / (d * 1e-3) / 1e9 if d > 0 else float("nan")
                log(f"  level {i} (step {1 << i}) = T({i + 1}) - T({i}): {d * 1e3:.1f} us, {gbs:.0f} GB/s of the "
                    f"64 B/pixel minimum")
            total = ft[0] + T[L][0]
            log(f"  features + denoise = {total:.3f} ms; / render 16 spp = {total / r[0]:.3f}")


def cmd_run(args):
    f = DeviceFrame(_scene(args.scene), *args.size)
    f.render()
    f.features()
    L = rt_amd.DENOISE_DEFAULTS["levels"]
    for _ in range(1 + args.calls):
        f.denoise(L)
    f.torch.cuda.synchronize()
    print(f"run: {args.scene} {args.size[0]}x{args.size[1]}, 1 + {args.calls} calls of {L} levels")


def cmd_trace(args):
    log = Log(args.log)
    L = rt_amd.DENOISE_DEFAULTS["levels"]
    rows = [r for r in csv.DictReader(open(args.csv)) if "k_atrous_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call = 2 + L
    calls = [rows[i:i + per_call] for i in range(0, len(rows) - per_call + 1, per_call)][1:]  # [0]: the warm-up
    if not calls:
        raise SystemExit("trace: no k_atrous_* dispatches after the warm-up")
    npix = args.size[0] * args.size[1]
    log(f"denoise_probe trace: {args.size[0]}x{args.size[1]}, {len(calls)} calls of {L} levels (median kernel time)")
    for j in range(per_call):
        kname = calls[0][j]["Kernel_Name"]
        stem = "k_atrous_init" if "init" in kname else "k_atrous_out" if "out" in kname else f"k_atrous_level {j - 1}"
        assert all(c[j]["Kernel_Name"] == kname for c in calls)
        us = statistics.median((int(c[j]["End_Timestamp"]) - int(c[j]["Start_Timestamp"])) * 1e-3 for c in calls)
        extra = ""
        if "level" in stem:
            extra = f", {npix * MIN_BYTES_PER_PIXEL / (us * 1e-6) / 1e9:.0f} GB/s of the 64 B/pixel minimum"
        log(f"  {stem}: {us:.1f} us{extra}")


GRID = dict(levels=(3, 4, 5), sigma_c=(0.3, 0.6, 1.2), sigma_n=(0.15, 0.3, 0.6), sigma_z=(0.05, 0.1, 0.3),
            sigma_a=(0.05, 0.1, 0.3))


def cmd_grid(args):
    log = Log(args.log)
    w, h = 96, 72
    frames = {}
    for name in SCENES:
        scene = _scene(name)
        _, sub, _ = rt_amd.render(scene, w, h, 16, 0x5EED, megakernel=True, want_sub=True)
        _, ref, _ = rt_amd.render(scene, w, h, 1024, 0x5EED + 77, megakernel=True, want_sub=True)
        c0 = lambda s: (np.clip(s, 0, 1) * 0.25).sum(2)
        truth = c0(ref)
        frames[name] = (sub, rt_amd.render_features(scene, w, h), truth,
                        float(np.sqrt(np.mean((c0(sub) - truth) ** 2))))
        log(f"{name}: noisy RMSE {frames[name][3]:.5f}")
    log(f"grid {GRID}")
    keys = list(GRID)
    results = []
    for vals in itertools.product(*(GRID[k] for k in keys)):
        p = dict(zip(keys, vals))
        ratios = []
        for name in SCENES:
            sub, feat, truth, noisy = frames[name]
            _, lin = rt_amd.denoise(sub, feat, want_linear=True, **p)
            ratios.append(float(np.sqrt(np.mean((lin.astype(np.float64) - truth) ** 2))) / noisy)
        results.append((float(np.mean(ratios)), p, ratios))
        log(" ".join(f"{k}={v}" for k, v in p.items()) + "  ratios " + " ".join(f"{r:.4f}" for r in ratios))
    results.sort(key=lambda r: r[0])
    log("best by mean ratio:")
    for mean, p, ratios in results[:5]:
        log(f"  {p} mean {mean:.4f} " + " ".join(f"{n}={r:.4f}" for n, r in zip(SCENES, ratios)))
    d = rt_amd.DENOISE_DEFAULTS
    for mean, p, ratios in results:
        if all(p[k] == d[k] for k in keys):
            log(f"DENOISE_DEFAULTS {d}: mean {mean:.4f} " + " ".join(f"{n}={r:.4f}" for n, r in zip(SCENES, ratios)))


# Progressive accumulation ------------------------------------------------------------------

VAR_GRID = dict(levels=(3, 4), sigma_c=(1.0, 2.0, 4.0, 8.0, 16.0, 32.0), sigma_n=(0.3,), sigma_z=(0.05,),
                sigma_a=(0.0, 0.1, 0.3))
VAR_INPUTS = ((2, 8), (4, 16), (8, 128))  # passes x spp
PASS_STEP = rt_amd.PASS_SEED_STEP
HBM_ACHIEVABLE = 6.3e12  # B/s: a float4 copy's measured rate on the MI355X


def _c0(s):
    return (np.clip(s, 0, 1) * 0.25).sum(2)


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - b) ** 2)))


def cmd_var_grid(args):
    log = Log(args.log)
    w, h = 96, 72
    frames = {}
    for name in SCENES:
        scene = _scene(name)
        _, ref, _ = rt_amd.render(scene, w, h, 4096, 0x5EED + 77, megakernel=True, want_sub=True)
        truth = _c0(ref)
        feat = rt_amd.render_features(scene, w, h)
        for passes, spp in VAR_INPUTS:
            with rt_amd.Accumulator(w, h) as acc:
                for k in range(passes):
                    acc.add(scene, spp, (0x5EED + k * PASS_STEP) % (1 << 64))
                sub, var, _ = acc.resolve(want_var=True, want_rgb=False)
            noisy = _rmse(_c0(sub), truth)
            _, lin = rt_amd.denoise(sub, feat, want_linear=True)
            fixed = _rmse(lin, truth)
            frames[name, passes * spp] = (sub, feat, var, truth, noisy, fixed)
            log(f"{name} {passes} x {spp} spp: noisy RMSE {noisy:.5f}, rt_denoise DENOISE_DEFAULTS {fixed:.5f} "
                f"(ratio {fixed / noisy:.4f})")
    log(f"grid {VAR_GRID}")
    keys = list(VAR_GRID)
    cols = [(n, passes * spp) for n in SCENES for passes, spp in VAR_INPUTS]
    results = []
    for vals in itertools.product(*(VAR_GRID[k] for k in keys)):
        p = dict(zip(keys, vals))
        ratios = []
        for col in cols:
            sub, feat, var, truth, noisy, _ = frames[col]
            _, lin = rt_amd.denoise_var(sub, feat, var, want_linear=True, **p)
            ratios.append(_rmse(lin, truth) / noisy)
        results.append((float(np.mean(ratios)), p, ratios))
        log(" ".join(f"{k}={v}" for k, v in p.items()) + "  ratios " + " ".join(f"{r:.4f}" for r in ratios))
    log("columns: " + " ".join(f"{n}@{s}" for n, s in cols))
    results.sort(key=lambda r: r[0])
    log("best by mean ratio (guided RMSE / noisy RMSE over the columns):")
    for mean, p, ratios in results[:5]:
        log(f"  {p} mean {mean:.4f} " + " ".join(f"{r:.4f}" for r in ratios))
    fixed = [frames[c][5] / frames[c][4] for c in cols]
    log(f"rt_denoise DENOISE_DEFAULTS: mean {np.mean(fixed):.4f} " + " ".join(f"{r:.4f}" for r in fixed))
    d = rt_amd.DENOISE_VAR_DEFAULTS
    for mean, p, ratios in results:
        if all(p[k] == d[k] for k in keys):
            log(f"DENOISE_VAR_DEFAULTS {d}: mean {mean:.4f} " + " ".join(f"{r:.4f}" for r in ratios))
            for (n, s), r, fx in zip(cols, ratios, fixed):
                log(f"  {n} {s} spp: guided / noisy {r:.4f}, fixed / noisy {fx:.4f}" +
                    ("  ** guided >= noisy" if r >= 1 else "") + ("  ** guided >= fixed" if s == 1024 and r >= fx else ""))


def cmd_var_time(args):
    log = Log(args.log)
    V = ctypes.c_void_p
    d = rt_amd.DENOISE_VAR_DEFAULTS
    L = d["levels"]
    sig = [float(d[k]) for k in ("sigma_c", "sigma_n", "sigma_z", "sigma_a")]
    log(f"denoise_probe var-time: reps {args.reps} (median [min, max] ms, HIP events; every rt_accum_* and rt_denoise_* "
        f"call also waits for its stream), levels {L}, defaults {d}")
    scene = _scene("cornell_box")
    for w, h in args.sizes:
        f = DeviceFrame(scene, w, h)
        npix = w * h
        dev = torch.device("cuda:0")
        var = torch.zeros(npix * 4, dtype=torch.float32, device=dev)
        sub2 = torch.zeros(npix * 12, dtype=torch.float64, device=dev)
        st = V(f.stream) if f.stream else None
        f.render()
        f.features()
        torch.cuda.synchronize()
        acc = rt_amd.Accumulator(w, h)

        def add():
            rt_amd._check(rt_amd.lib.rt_accum_add_sub_device(acc.handle, V(f.sub.data_ptr()), 4, st))

        def resolve(rgb):
            rt_amd._check(rt_amd.lib.rt_accum_resolve_device(acc.handle, V(sub2.data_ptr()), V(var.data_ptr()),
                                                             V(f.rgb2.data_ptr()) if rgb else None, st))

        def denoise_var(levels):
            rt_amd._check(rt_amd.lib.rt_denoise_var_device(0, w, h, V(sub2.data_ptr()), V(f.feat.data_ptr()),
                                                           V(var.data_ptr()), levels, *sig, V(f.rgb2.data_ptr()), None,
                                                           None, st))

        add()  # the first pass stores; the timed ones read and write the sums
        t_add = f.timed(add, args.reps)
        t_res = f.timed(lambda: resolve(False), args.reps)
        t_res_rgb = f.timed(lambda: resolve(True), args.reps)
        t_render = f.timed(f.render, args.reps)
        TV = [f.timed(lambda k=k: denoise_var(k), args.reps) for k in range(L + 1)]
        TF = [f.timed(lambda k=k: f.denoise(k), args.reps) for k in range(L + 1)]
        add_bytes, res_bytes = npix * (96 + 192 + 192), npix * (192 + 96 + 16)
        fmt = lambda t: f"{t[0]:.3f} [{t[1]:.3f}, {t[2]:.3f}]"
        log(f"cornell_box {w}x{h}:")
        log(f"  rt_accum_add_sub_device: {fmt(t_add)}; 480 B/pixel = {add_bytes / (t_add[0] * 1e-3) / 1e9:.0f} GB/s, "
            f"{100 * add_bytes / (t_add[0] * 1e-3) / HBM_ACHIEVABLE:.0f}% of 6.3 TB/s")
        log(f"  rt_accum_resolve_device (sub + var): {fmt(t_res)}; 304 B/pixel = "
            f"{res_bytes / (t_res[0] * 1e-3) / 1e9:.0f} GB/s, {100 * res_bytes / (t_res[0] * 1e-3) / HBM_ACHIEVABLE:.0f}% "
            f"of 6.3 TB/s")
        log(f"  rt_accum_resolve_device (sub + var + RGB8): {fmt(t_res_rgb)}")
        log(f"  rt_render_device 16 spp: {fmt(t_render)}")
        for k in range(L + 1):
            log(f"  levels={k}: rt_denoise_var_device {fmt(TV[k])}   rt_denoise_device {fmt(TF[k])}")
        for i in range(1, L):
            dv, df = TV[i + 1][0] - TV[i][0], TF[i + 1][0] - TF[i][0]
            log(f"  level {i} (step {1 << i}) = T({i + 1}) - T({i}): k_atrous_level_var {dv * 1e3:.1f} us, k_atrous_level "
                f"{df * 1e3:.1f} us, ratio {dv / df if df > 0 else float('nan'):.2f}")
        acc.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sp = ap.add_subparsers(dest="cmd", required=True)
    t = sp.add_parser("time")
    t.add_argument("--sizes", type=lambda s: [_size(x) for x in s.split(",")], default=[(600, 450), (1920, 1080)])
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--log", default=os.path.join(REPO, "profiles", "denoise_probe.log"))
    r = sp.add_parser("run")
    r.add_argument("scene")
    r.add_argument("size", type=_size)
    r.add_argument("calls", type=int, nargs="?", default=10)
    tr = sp.add_parser("trace")
    tr.add_argument("csv")
    tr.add_argument("size", type=_size)
    tr.add_argument("--log", default=os.path.join(REPO, "profiles", "denoise_probe_trace.log"))
    g = sp.add_parser("grid")
    g.add_argument("--log", default=os.path.join(REPO, "profiles", "denoise_grid.log"))
    vg = sp.add_parser("var-grid")
    vg.add_argument("--log", default=os.path.join(REPO, "profiles", "denoise_var_grid.log"))
    vt = sp.add_parser("var-time")
    vt.add_argument("--sizes", type=lambda s: [_size(x) for x in s.split(",")], default=[(600, 450), (1920, 1080)])
    vt.add_argument("--reps", type=int, default=30)
    vt.add_argument("--log", default=os.path.join(REPO, "profiles", "denoise_var_time.log"))
    args = ap.parse_args()
    {"time": cmd_time, "run": cmd_run, "trace": cmd_trace, "grid": cmd_grid, "var-grid": cmd_var_grid,
     "var-time": cmd_var_time}[args.cmd](args)


if __name__ == "__main__":
    main()
