"""Cost and benefit of rendering to a per-pixel error target on the GPU.

  python tools/adapt_probe.py time [--size 1920x1080] [--reps 30] [--log profiles/adapt_time.log]
      cornell_box at 16 spp, HIP events (torch.cuda.Event on the stream the calls are enqueued on) in one process, after
      a warm-up and as the median of --reps calls: rt_render_pixels_device for lists of 100 %, 50 %, 10 % and 1 % of the
      pixels, both every k-th pixel and the ids rt_accum_select returns at the threshold that leaves that fraction
      active, each interleaved with rt_render_device of the full frame at 16 spp; then rt_accum_select_device and
      rt_accum_add_sub_pixels_device. Reports Msamples/s, the 100 % list's rate over the full-frame megakernel's, and the
      break-even fraction (the list size at which a sparse pass costs a full pass).
  python tools/adapt_probe.py time --scene cubes|flying_unicorn [--family both|fused|pool|auto] [--log ...]
      DESIGN.md §16, the same protocol for one scene and chosen kernel families (rt_render_pixels_with_device): lists of
      every pixel and every 2nd, 10th, 100th and 1000th pixel (--strides) at 16 spp, each family's list render interleaved with
      rt_render_device of the full frame; `both` runs the fused megakernel's list instance (k_render_list_f64) and the
      scene's pool side by side and reports the
      shortest list from which the pool is never slower (the automatic choice's threshold).
  python tools/adapt_probe.py target [--size 96x72] [--log profiles/adapt_target.log]
      The three scenes with abs_tol in {0.03, 0.04, 0.06}: two full 8-spp passes, up to 30 sparse passes of 16 spp; mean
      and max spp, passes, and the linear RMSE against a 4096-spp frame of seed 999 over that of a uniform accumulation
      with the same pass sizes taken to the first total at or above the mean spp. These figures choose
      rt_amd.ERROR_TARGET_DEFAULTS.
  python tools/adapt_probe.py batch [--size 1920x1080] [--scenes cornell_box,cubes,flying_unicorn] [--batch C --gain g]
                                    [--family auto|fused] [--log profiles/batch_time.log]
      DESIGN.md §17, §18: the sequential error-target loop (rt_accum_select_device, rt_render_pixels_device with the
      scene's own list family, rt_accum_add_sub_pixels_device) and the batched one (rt_accum_refine: the passes instance
      of the scene's own family) side by side in one process, a step of each in turn, on two accumulators that start from the
      same two 8-spp passes; abs_tol 0.04, pass_spp 16, max_spp 496. Per loop: render launches, the wall time from the
      first selection to the last merge (every call waits for its work), the renders' device time (HIP events around
      the render kernels, rt_render_stats.device_ms), Msamples/s per launch (median, first, last), mean spp.
      --family fused: the batched loop's renders on the fused body's k_render_passes_f64 for every scene, as before the
      pools had passes instances. rt_accum_refine has no family argument, so this loop is its restatement in public
      calls: rt_accum_plan_device, rt_render_pixel_passes_with_device(RT_LIST_FUSED), then per pass i one
      rt_accum_add_sub_pixels_device of the entries with counts[e] > i (the bits of the run merge, in more launches:
      compare the render time; the wall time carries those merges and the gathers between them).
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

SCENES = ("cornell_box", "cubes", "flying_unicorn")
V = ctypes.c_void_p


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


def _timed_pair(fn_a, fn_b, reps, warm=3):
    """Medians (ms) of fn_a and fn_b, called alternately between events on torch's current stream."""
    for _ in range(warm):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(reps):
        for fn, ms in zip((fn_a, fn_b), out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return statistics.median(out[0]), statistics.median(out[1])


def _c_of(sub):
    px = np.zeros(sub.shape[:2] + (3,))
    for j in range(4):
        px = px + np.clip(sub[:, :, j], 0.0, 1.0) * 0.25
    return px


FAMILY_NAMES = {rt_amd.LIST_AUTO: "auto", rt_amd.LIST_FUSED: "fused", rt_amd.LIST_FPOOL: "fpool", rt_amd.LIST_ROLES: "roles"}


def cmd_time_families(args):
    """One scene, strided lists, the chosen kernel families against the full frame."""
    log = Log(args.log)
    w, h = _size(args.size)
    npix, spp = w * h, 16
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    st = V(stream) if stream else None
    sc = _scene(args.scene)
    p = rt_amd.make_params(w, h, spp, 0x5EED, None, rt_amd.FLAG_MEGAKERNEL, 0, 1)
    pool = rt_amd.render_pixels_path(sc, w, h, spp, npix)[1]
    fams = {"both": [rt_amd.LIST_FUSED, pool], "fused": [rt_amd.LIST_FUSED], "pool": [pool],
            "auto": [rt_amd.LIST_AUTO]}[args.family]
    fams = list(dict.fromkeys(fams))  # a scene without a pool: the fused kernel once
    rgb = torch.zeros(npix * 3, dtype=torch.uint8, device=dev)
    sub = torch.zeros(npix * 12, dtype=torch.float64, device=dev)
    lsub = torch.zeros(npix * 12, dtype=torch.float64, device=dev)
    ids_d = torch.zeros(npix, dtype=torch.int32, device=dev)

    def full():
        rt_amd.render_device(sc, p, rgb.data_ptr(), sub.data_ptr(), stream)

    def listed(n, fam):
        def fn():
            rt_amd._check(rt_amd.lib.rt_render_pixels_with_device(sc.handle, ctypes.byref(p), V(ids_d.data_ptr()), n, fam,
                                                                  None, V(lsub.data_ptr()), st, None))
        return fn

    log(f"# adapt_probe time: {args.scene} {w}x{h}, {spp} spp, median of {args.reps} after 3 warm-up calls (HIP events, "
        f"one process, each list interleaved with the full frame); the scene's pool: {FAMILY_NAMES[pool]}")
    log("every k-th  n_pixels  family   list ms   full ms  list Ms/s  full Ms/s  list/full time  auto takes")
    times = {}
    for k in [int(x) for x in args.strides.split(",")]:
        ids = np.arange(0, npix, k, dtype=np.uint32)
        n = int(ids.size)
        ids_d[:n] = torch.from_numpy(ids.astype(np.int32)).to(dev)
        torch.cuda.synchronize()
        auto = FAMILY_NAMES[rt_amd.render_pixels_path(sc, w, h, spp, n)[0]]
        for fam in fams:
            t_list, t_full = _timed_pair(listed(n, fam), full, args.reps)
            times[(n, fam)] = t_list
            log(f"{k:10d} {n:9d}  {FAMILY_NAMES[fam]:6s} {t_list:9.3f} {t_full:9.3f} {n * spp / t_list / 1e3:10.1f} "
                f"{npix * spp / t_full / 1e3:10.1f} {t_list / t_full:14.3f}  {auto}")
    if args.family == "both" and pool != rt_amd.LIST_FUSED:
        ns = sorted({n for n, _ in times})
        slower = [n for n in ns if times[(n, pool)] > times[(n, rt_amd.LIST_FUSED)]]
        ok = [n for n in ns if not slower or n > max(slower)]
        log(f"the pool is slower than k_render_list_f64 at n_pixels in {slower}; never slower from "
            + (f"{min(ok)} on" if ok else "no measured length on"))


def cmd_time(args):
    if rt_amd.device_count() < 1:
        raise RuntimeError("adapt_probe: no HIP device visible (it measures on the GPU only)")
    if args.scene != "cornell_box" or args.family != "auto":
        return cmd_time_families(args)
    log = Log(args.log)
    w, h = _size(args.size)
    npix, spp = w * h, 16
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    st = V(stream) if stream else None
    sc = _scene("cornell_box")
    p = rt_amd.make_params(w, h, spp, 0x5EED, None, rt_amd.FLAG_MEGAKERNEL, 0, 1)
    rgb = torch.zeros(npix * 3, dtype=torch.uint8, device=dev)
    sub = torch.zeros(npix * 12, dtype=torch.float64, device=dev)
    lsub = torch.zeros(npix * 12, dtype=torch.float64, device=dev)
    ids_d = torch.zeros(npix, dtype=torch.int32, device=dev)

    def full():
        rt_amd.render_device(sc, p, rgb.data_ptr(), sub.data_ptr(), stream)

    def listed(n):
        def fn():
            rt_amd._check(rt_amd.lib.rt_render_pixels_device(sc.handle, ctypes.byref(p), V(ids_d.data_ptr()), n, None,
                                                             V(lsub.data_ptr()), st, None))
        return fn

    log(f"# adapt_probe time: cornell_box {w}x{h}, {spp} spp, median of {args.reps} (HIP events, one process, "
        "each list interleaved with the full frame)")
    # an accumulator with two 8-spp passes: the selection's input
    acc = rt_amd.Accumulator(w, h)
    acc.add(sc, 8, 1)
    acc.add(sc, 8, 2)
    log("fraction  list            n_pixels   list ms   full ms  list Ms/s  full Ms/s  list/full time")
    rate100 = None
    rows = []
    for frac in (1.0, 0.5, 0.1, 0.01):
        k = max(1, int(round(1.0 / frac)))
        strided = np.arange(0, npix, k, dtype=np.uint32)
        # the threshold that leaves about `frac` of the pixels active: bisect abs_tol on the device's own count
        lo, hi = 0.0, 1.0
        for _ in range(30):
            mid = 0.5 * (lo + hi)
            n = acc.select(mid, 0.0, 0, cap=0)[1]
            if n > frac * npix:
                lo = mid
            else:
                hi = mid
        selected = acc.select(hi if frac < 1.0 else 0.0, 0.0, 0)[0]
        for name, ids in (("every k-th", strided), ("rt_accum_select", selected)):
            n = int(ids.size)
            if n == 0:
                continue
            ids_d[:n] = torch.from_numpy(ids.astype(np.int32)).to(dev)
            torch.cuda.synchronize()
            t_list, t_full = _timed_pair(listed(n), full, args.reps)
            r_list, r_full = n * spp / t_list / 1e3, npix * spp / t_full / 1e3
            log(f"{frac:7.2f}   {name:15s} {n:9d} {t_list:9.3f} {t_full:9.3f} {r_list:10.1f} {r_full:10.1f} "
                f"{t_list / t_full:9.3f}")
            rows.append((n / npix, t_list, t_full, name))
            if frac == 1.0 and name == "every k-th":
                rate100 = r_list / r_full
    log(f"100 % list rate over the full-frame megakernel's: {rate100:.3f}")
    # break-even: the fraction at which the list's time reaches the full frame's (linear between measured points)
    for name in ("every k-th", "rt_accum_select"):
        pts = sorted((f, tl / tf) for f, tl, tf, nm in rows if nm == name)
        be = None
        for (f0, r0), (f1, r1) in zip(pts, pts[1:]):
            if r0 < 1.0 <= r1:
                be = f0 + (1.0 - r0) * (f1 - f0) / (r1 - r0)
        log(f"break-even fraction ({name}): " + (f"{be:.2f}" if be is not None else
                                                 "none below 100 % (a sparse pass never costs more than a full pass)"
                                                 if pts and pts[-1][1] < 1.0 else "below the smallest list measured"))
    # the selection and the sparse merge
    n_out = ctypes.c_int64()

    def select():
        rt_amd._check(rt_amd.lib.rt_accum_select_device(acc.handle, 0.04, 0.0, 0, V(ids_d.data_ptr()), npix,
                                                        ctypes.byref(n_out), st))

    half = np.arange(0, npix, 2, dtype=np.uint32)
    ids_h = torch.from_numpy(half.astype(np.int32)).to(dev)

    def merge():
        rt_amd._check(rt_amd.lib.rt_accum_add_sub_pixels_device(acc.handle, V(ids_h.data_ptr()), half.size,
                                                                V(lsub.data_ptr()), 4, st))

    t_sel, t_merge = _timed_pair(select, merge, args.reps)
    log(f"rt_accum_select_device (resolve of the variance + 3 kernels + the count's read-back): {t_sel:.3f} ms")
    log(f"rt_accum_add_sub_pixels_device, 50 % list: {t_merge:.3f} ms "
        f"({half.size * 500 / t_merge / 1e6:.0f} GB/s of its minimum traffic: 500 B per entry, the pass 96, S and Q "
        "read and written 384, the counts 16, the id 4)")
    acc.close()


def cmd_target(args):
    if rt_amd.device_count() < 1:
        raise RuntimeError("adapt_probe: no HIP device visible (it measures on the GPU only)")
    log = Log(args.log)
    w, h = _size(args.size)
    seed = 77
    log(f"# adapt_probe target: {w}x{h}, two 8-spp passes + up to 30 sparse passes of 16 spp, seeds pass_seed({seed}, k); "
        "uniform: pass_seed(1077, k); truth: 4096 spp, seed 999")
    log("scene            abs_tol  mean spp  max spp  mean/max  passes  RMSE adaptive  RMSE uniform (spp)  ratio")
    for name in SCENES:
        sc = _scene(name)
        _, tsub, _ = rt_amd.render(sc, w, h, 4096, 999, megakernel=True, want_sub=True)
        truth = _c_of(tsub)
        for abs_tol in (0.03, 0.04, 0.06):
            with rt_amd.Accumulator(w, h) as acc:
                acc.add(sc, 8, rt_amd.pass_seed(seed, 0))
                acc.add(sc, 8, rt_amd.pass_seed(seed, 1))
                passes = 0
                for k in range(2, 32):
                    ids, n = acc.select(abs_tol, 0.0, 0)
                    if n == 0:
                        break
                    acc.add_pixels(sc, ids, 16, rt_amd.pass_seed(seed, k))
                    passes += 1
                n_p = acc.counts()[1].astype(np.float64)
                rmse_a = float(np.sqrt(np.mean((_c_of(acc.resolve()[0]) - truth) ** 2)))
            mean_spp, max_spp = 4 * n_p.mean(), 4 * n_p.max()
            with rt_amd.Accumulator(w, h) as uni:
                k, spp = 0, 0
                while spp < mean_spp:
                    size = 8 if k < 2 else 16
                    uni.add(sc, size, rt_amd.pass_seed(seed + 1000, k))
                    spp += size
                    k += 1
                rmse_u = float(np.sqrt(np.mean((_c_of(uni.resolve()[0]) - truth) ** 2)))
            log(f"{name:16s} {abs_tol:7.2f} {mean_spp:9.1f} {max_spp:8.0f} {mean_spp / max_spp:9.3f} {passes:7d} "
                f"{rmse_a:14.5f} {rmse_u:13.5f} ({spp:3d}) {rmse_a / rmse_u:6.3f}")


def cmd_batch(args):
    import time

    if rt_amd.device_count() < 1:
        raise RuntimeError("adapt_probe: no HIP device visible (it measures on the GPU only)")
    log = Log(args.log)
    w, h = _size(args.size)
    npix, spp, abs_tol, max_n, seed = w * h, 16, 0.04, 496 // 4, 77
    d = rt_amd.ERROR_TARGET_BATCH_DEFAULTS
    C = args.batch if args.batch else d["batch"]
    gain = args.gain if args.gain else d["gain"]
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    st = V(stream) if stream else None
    ids_d = torch.zeros(npix, dtype=torch.int32, device=dev)
    lsub = torch.zeros(npix * 12, dtype=torch.float64, device=dev)
    log(f"# adapt_probe batch: {w}x{h}, abs_tol {abs_tol}, two 8-spp passes, then passes of {spp} spp to max_spp 496; "
        f"batched: C = {C}, gain = {gain}, family {args.family}; seeds pass_seed({seed}, k); one process, a step of each loop in turn")
    log("scene            loop        list family  launches  wall ms  render ms  Ms/s per launch median (first, last)  "
        "mean spp")
    for name in args.scenes.split(","):
        sc = _scene(name)
        fam = FAMILY_NAMES[rt_amd.render_pixels_path(sc, w, h, spp, npix)[0]]
        p = rt_amd.make_params(w, h, spp, 0, None, rt_amd.FLAG_MEGAKERNEL, 0, 1)
        seq, bat = rt_amd.Accumulator(w, h), rt_amd.Accumulator(w, h)
        for acc in (seq, bat):
            acc.add(sc, 8, rt_amd.pass_seed(seed, 0))
            acc.add(sc, 8, rt_amd.pass_seed(seed, 1))
        # warm-up on a third accumulator: both paths' kernels loaded, the workspaces allocated
        with rt_amd.Accumulator(w, h) as warm:
            warm.add(sc, 8, 1)
            warm.add(sc, 8, 2)
            ids, _ = warm.select(abs_tol, 0.0, max_n)
            warm.add_pixels(sc, ids, spp, 3)
            warm.refine(sc, spp, [4, 5], abs_tol, 0.0, max_n, gain)
        torch.cuda.synchronize()
        stats = rt_amd.RenderStats()
        n_out = ctypes.c_int64()
        run = {"sequential": dict(k=2, wall=0.0, ms=[], samples=[], done=False),
               "batched": dict(k=2, wall=0.0, ms=[], samples=[], done=False)}

        def step_seq(r):
            t0 = time.perf_counter()
            rt_amd._check(rt_amd.lib.rt_accum_select_device(seq.handle, abs_tol, 0.0, max_n, V(ids_d.data_ptr()), npix,
                                                            ctypes.byref(n_out), st))
            n = n_out.value
            if n:
                p.seed = rt_amd.pass_seed(seed, r["k"])
                rt_amd._check(rt_amd.lib.rt_render_pixels_device(sc.handle, ctypes.byref(p), V(ids_d.data_ptr()), n, None,
                                                                 V(lsub.data_ptr()), st, ctypes.byref(stats)))
                rt_amd._check(rt_amd.lib.rt_accum_add_sub_pixels_device(seq.handle, V(ids_d.data_ptr()), n,
                                                                        V(lsub.data_ptr()), spp // 4, st))
                r["k"] += 1
            r["wall"] += time.perf_counter() - t0
            return n, stats.device_ms, stats.samples

        cnt_d = torch.zeros(npix, dtype=torch.uint8, device=dev)
        units_out, used_out = ctypes.c_int64(), ctypes.c_int64()

        def step_bat_fused(r):
            t0 = time.perf_counter()
            rt_amd._check(rt_amd.lib.rt_accum_plan_device(bat.handle, abs_tol, 0.0, max_n, spp // 4, gain, C,
                                                          V(ids_d.data_ptr()), V(cnt_d.data_ptr()), npix,
                                                          ctypes.byref(n_out), ctypes.byref(units_out),
                                                          ctypes.byref(used_out), st))
            n, units, used = n_out.value, units_out.value, used_out.value
            if n:
                sd = np.array([rt_amd.pass_seed(seed, r["k"] + i) % (1 << 64) for i in range(C)], dtype=np.uint64)
                rt_amd._check(rt_amd.lib.rt_render_pixel_passes_with_device(
                    sc.handle, ctypes.byref(p), V(ids_d.data_ptr()), V(cnt_d.data_ptr()), n, units,
                    sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), C, rt_amd.LIST_FUSED, None, V(lsub.data_ptr()), st,
                    ctypes.byref(stats)))
                cnt = cnt_d[:n].to(torch.int64)
                off = torch.cumsum(cnt, 0) - cnt
                sub = lsub.view(-1, 12)
                for i in range(used):
                    m = cnt > i
                    ids_i = ids_d[:n][m].contiguous()
                    sub_i = sub[off[m] + i].contiguous()
                    rt_amd._check(rt_amd.lib.rt_accum_add_sub_pixels_device(bat.handle, V(ids_i.data_ptr()), ids_i.numel(),
                                                                            V(sub_i.data_ptr()), spp // 4, st))
                    torch.cuda.synchronize()
                r["k"] += used
            r["wall"] += time.perf_counter() - t0
            return n, stats.device_ms, stats.samples

        def step_bat(r):
            if args.family == "fused":
                return step_bat_fused(r)
            t0 = time.perf_counter()
            out = bat.refine(sc, spp, [rt_amd.pass_seed(seed, r["k"] + i) for i in range(C)], abs_tol, 0.0, max_n, gain)
            r["wall"] += time.perf_counter() - t0
            r["k"] += out["refine"][2]
            return out["refine"][0], out["device_ms"], out["samples"]

        while not (run["sequential"]["done"] and run["batched"]["done"]):
            for key, fn in (("sequential", step_seq), ("batched", step_bat)):
                r = run[key]
                if r["done"]:
                    continue
                n, ms, samples = fn(r)
                if n == 0 or len(r["ms"]) >= 400:
                    r["done"] = True
                else:
                    r["ms"].append(ms)
                    r["samples"].append(samples)
        for key, acc in (("sequential", seq), ("batched", bat)):
            r = run[key]
            rates = [s_ / m / 1e3 for s_, m in zip(r["samples"], r["ms"]) if m > 0]
            mean_spp = 4.0 * float(acc.counts()[1].mean())
            log(f"{name:16s} {key:11s} {fam if key == 'sequential' or args.family == 'auto' else 'fused':11s} {len(r['ms']):9d} "
                f"{r['wall'] * 1e3:8.1f} {sum(r['ms']):10.1f}  {statistics.median(rates):10.1f} ({rates[0]:.1f}, "
                f"{rates[-1]:.1f})" + " " * 12 + f"{mean_spp:8.2f}")
        s_, b_ = run["sequential"], run["batched"]
        log(f"{name}: batched / sequential wall time {b_['wall'] / s_['wall']:.3f}, render time "
            f"{sum(b_['ms']) / sum(s_['ms']):.3f}, launches {len(b_['ms'])} / {len(s_['ms'])}")
        seq.close()
        bat.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sp = ap.add_subparsers(dest="cmd", required=True)
    t = sp.add_parser("time")
    t.add_argument("--size", default="1920x1080")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--scene", default="cornell_box", choices=SCENES)
    t.add_argument("--family", default="auto", choices=("auto", "fused", "pool", "both"))
    t.add_argument("--strides", default="1,2,10,100,1000", help="with --scene / --family: list k = every k-th pixel")
    t.add_argument("--log", default=os.path.join(REPO, "profiles", "adapt_time.log"))
    t.set_defaults(fn=cmd_time)
    g = sp.add_parser("target")
    g.add_argument("--size", default="96x72")
    g.add_argument("--log", default=os.path.join(REPO, "profiles", "adapt_target.log"))
    g.set_defaults(fn=cmd_target)
    b = sp.add_parser("batch")
    b.add_argument("--size", default="1920x1080")
    b.add_argument("--scenes", default="cornell_box,cubes,flying_unicorn")
    b.add_argument("--batch", type=int, default=0, help="C (default: rt_amd.ERROR_TARGET_BATCH_DEFAULTS)")
    b.add_argument("--gain", type=float, default=0.0)
    b.add_argument("--family", default="auto", choices=("auto", "fused"),
                   help="the batched loop's kernel family: the scene's own (auto) or k_render_passes_f64 for every scene")
    b.add_argument("--log", default=os.path.join(REPO, "profiles", "batch_time.log"))
    b.set_defaults(fn=cmd_batch)
    args = ap.parse_args()
    args.fn(args)


if __name__ == "__main__":
    main()
