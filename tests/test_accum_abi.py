"""Progressive accumulation, the part that needs no GPU: the new C entry points are exported, declared for Rust and
mirrored in rt_amd; bad arguments are RT_E_INVAL with a message before any device call; the numpy restatement the GPU
tests compare against (tests/accum_ref.py) has the defining properties; and the variance estimator is valid against
the CPU oracle."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import accum_ref as aref
import denoise_ref as ref
from conftest import REPO, scene_path

NAMES = ("rt_accum_create", "rt_accum_destroy", "rt_accum_reset", "rt_accum_info", "rt_accum_add", "rt_accum_add_sub",
         "rt_accum_add_sub_device", "rt_accum_resolve", "rt_accum_resolve_device", "rt_denoise_var",
         "rt_denoise_var_device")
INVAL, NODEVICE = -1, -6


def test_exported_declared_and_mirrored(rt):
    header = open(os.path.join(REPO, "include", "rt_ffi.h")).read()
    rust = open(os.path.join(REPO, "ffi", "raytracer_ffi.rs")).read()
    for n in NAMES:
        assert hasattr(rt.lib, n), f"missing export {n}"
        assert re.search(rf"^(int|void) {n}\(", header, re.M), f"{n} not declared in rt_ffi.h"
        assert re.search(rf"pub fn {n}\s*\(", rust), f"{n} not declared in raytracer_ffi.rs"
        assert n in rt._EXPORTS
    assert rt.lib.rt_abi_version() == 3
    for f in ("Accumulator", "denoise_var", "render_progressive", "progressive_passes"):
        assert callable(getattr(rt, f))
    for m in ("add", "add_sub", "resolve", "info", "reset", "close"):
        assert callable(getattr(rt.Accumulator, m))
    assert set(rt.DENOISE_VAR_DEFAULTS) == {"levels", "sigma_c", "sigma_n", "sigma_z", "sigma_a"}
    assert 0 <= rt.DENOISE_VAR_DEFAULTS["levels"] <= 8
    from rt_amd import server
    assert callable(server.ProgressiveJob)


def test_pass_plan():
    """first/2, first/2, then doubling, the last cut to reach 4 floor(spp / 4); every pass a multiple of 4."""
    import rt_amd as rt

    assert rt.progressive_passes(64, 8) == [4, 4, 8, 16, 32]
    assert rt.progressive_passes(67, 8) == [4, 4, 8, 16, 32]
    assert rt.progressive_passes(100, 16) == [8, 8, 16, 32, 36]
    assert rt.progressive_passes(4, 8) == [4]
    assert rt.progressive_passes(20, 8) == [4, 4, 8, 4]
    for spp, first in ((1000, 8), (257, 24), (9, 1)):
        p = rt.progressive_passes(spp, first)
        assert sum(p) == 4 * (spp // 4) and all(x % 4 == 0 and x > 0 for x in p)
    with pytest.raises(ValueError):
        rt.progressive_passes(3)


def _is_inval(rt, rc):
    assert rc == INVAL, rc
    assert len(rt.lib.rt_last_error()) > 0


def _new_accum(rt, w=4, h=3, device=0):
    a = ctypes.c_void_p()
    assert rt.lib.rt_accum_create(device, w, h, ctypes.byref(a)) == 0  # no device call: also without a GPU
    return a


def test_accum_bad_arguments_are_inval(rt):
    """Nulls, sizes < 1, n < 1, tile != frame, row_step > 1, spp < 4, a device mismatch and var_out with K < 2 are
    RT_E_INVAL with a message, checked before any device call (so also without a GPU)."""
    L = rt.lib
    h = ctypes.c_void_p()
    _is_inval(rt, L.rt_accum_create(0, 4, 3, None))
    for dev, w, hh in ((0, 0, 3), (0, 4, 0), (0, -1, 3), (0, 4, -7), (-1, 4, 3), (0, 65536, 32768)):
        _is_inval(rt, L.rt_accum_create(dev, w, hh, ctypes.byref(h)))
        assert not h.value
    L.rt_accum_destroy(None)  # a no-op
    _is_inval(rt, L.rt_accum_reset(None))
    info = np.zeros(4, dtype=np.int64)
    I64 = ctypes.POINTER(ctypes.c_int64)
    _is_inval(rt, L.rt_accum_info(None, info.ctypes.data_as(I64)))

    a = _new_accum(rt)
    _is_inval(rt, L.rt_accum_info(a, None))
    assert L.rt_accum_info(a, info.ctypes.data_as(I64)) == 0 and info.tolist() == [0, 0, 4, 3]
    sub = np.zeros((3, 4, 4, 3))
    D = ctypes.POINTER(ctypes.c_double)
    _is_inval(rt, L.rt_accum_add_sub(None, sub.ctypes.data_as(D), 1))
    _is_inval(rt, L.rt_accum_add_sub(a, None, 1))
    _is_inval(rt, L.rt_accum_add_sub_device(None, ctypes.c_void_p(16), 1, None))
    _is_inval(rt, L.rt_accum_add_sub_device(a, None, 1, None))
    for n in (0, -1, -(2 ** 31)):
        _is_inval(rt, L.rt_accum_add_sub(a, sub.ctypes.data_as(D), n))
        _is_inval(rt, L.rt_accum_add_sub_device(a, ctypes.c_void_p(16), n, None))

    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    good = rt.make_params(4, 3, 8, 1, None, rt.FLAG_MEGAKERNEL, 0, 1)
    _is_inval(rt, L.rt_accum_add(None, sc.handle, ctypes.byref(good), None, None))
    _is_inval(rt, L.rt_accum_add(a, None, ctypes.byref(good), None, None))
    _is_inval(rt, L.rt_accum_add(a, sc.handle, None, None, None))
    bad = [rt.make_params(4, 3, 8, 1, (0, 0, 4, 2)),       # tile != frame
           rt.make_params(4, 3, 8, 1, (1, 0, 3, 3)),
           rt.make_params(4, 3, 8, 1, (0, 1, 4, 2)),
           rt.make_params(8, 6, 8, 1, (0, 0, 4, 3)),       # a tile of a larger frame
           rt.make_params(5, 3, 8, 1),                     # another frame
           rt.make_params(4, 3, 8, 1, row_step=2),
           rt.make_params(4, 3, 8, 1, row_step=-1),
           rt.make_params(4, 3, 3, 1), rt.make_params(4, 3, 0, 1), rt.make_params(4, 3, -8, 1),  # spp < 4
           rt.make_params(4, 3, 8, 1, device=1)]           # device mismatch
    for p in bad:
        _is_inval(rt, L.rt_accum_add(a, sc.handle, ctypes.byref(p), None, None))
    assert L.rt_accum_info(a, info.ctypes.data_as(I64)) == 0 and info.tolist() == [0, 0, 4, 3]

    # K = 0: nothing to resolve; and var_out needs K >= 2 (K = 1 is checked on the device, tests/test_gpu_accum.py)
    var = np.zeros((3, 4, 4), dtype=np.float32)
    rgb = np.zeros((3, 4, 3), dtype=np.uint8)
    F, U8 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)
    _is_inval(rt, L.rt_accum_resolve(None, None, None, rgb.ctypes.data_as(U8)))
    _is_inval(rt, L.rt_accum_resolve(a, sub.ctypes.data_as(D), None, rgb.ctypes.data_as(U8)))
    _is_inval(rt, L.rt_accum_resolve(a, None, var.ctypes.data_as(F), None))
    _is_inval(rt, L.rt_accum_resolve_device(None, ctypes.c_void_p(16), None, None, None))
    _is_inval(rt, L.rt_accum_resolve_device(a, ctypes.c_void_p(16), ctypes.c_void_p(16), None, None))
    L.rt_accum_destroy(a)


def _denoise_var_args(w=4, h=3, levels=2, sig=(0.5, 0.5, 0.5, 0.5)):
    sub = np.zeros((h, w, 4, 3))
    feat = np.zeros((h, w, 8), dtype=np.float32)
    var = np.zeros((h, w, 4), dtype=np.float32)
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    lin = np.zeros((h, w, 3), dtype=np.float32)
    vout = np.zeros((h, w), dtype=np.float32)
    keep = (sub, feat, var, rgb, lin, vout)
    P = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    F = ctypes.c_float
    return keep, [0, w, h, P(sub, ctypes.c_double), P(feat, F), P(var, F), levels, *sig, P(rgb, ctypes.c_uint8),
                  P(lin, F), P(vout, F)]


PTRS = (3, 4, 5, 11, 12, 13)  # the buffer arguments of rt_denoise_var


def _dev_form(args):
    return [ctypes.cast(x, ctypes.c_void_p) if i in PTRS and x is not None else x for i, x in enumerate(args)]


def test_denoise_var_bad_arguments_are_inval(rt):
    """Null buffers, sizes < 1, width * height beyond int32, levels outside 0..8 and a non-finite sigma, for the host
    and the device entry point."""
    def both(args):
        _is_inval(rt, rt.lib.rt_denoise_var(*args))
        _is_inval(rt, rt.lib.rt_denoise_var_device(*_dev_form(args), None))

    for null_at in (3, 4, 5, 11):  # sub, feat, var, rgb_out (lin_out and var_out are optional)
        keep, a = _denoise_var_args()
        a[null_at] = None
        both(a)
    for w, h in ((0, 3), (4, 0), (-1, 3), (4, -7), (65536, 32768), (2 ** 31 - 1, 2)):
        keep, a = _denoise_var_args()
        a[1], a[2] = w, h
        both(a)
    for levels in (-1, 9, 1 << 20):
        keep, a = _denoise_var_args(levels=levels)
        both(a)
    for bad in (math.nan, math.inf, -math.inf):
        for k in range(4):
            sig = [0.5] * 4
            sig[k] = bad
            keep, a = _denoise_var_args(sig=sig)
            both(a)


def test_valid_arguments_without_a_gpu_are_nodevice(rt):
    """Valid arguments on a host without a GPU: RT_E_NODEVICE (-6), like the rest of the ABI. (With a device the
    calls run; tests/test_gpu_accum.py and tests/test_gpu_denoise_var.py check what they compute.)"""
    if rt.device_count() > 0:
        keep, a = _denoise_var_args()
        assert rt.lib.rt_denoise_var(*a) == 0
        return
    L = rt.lib
    a = _new_accum(rt)
    sub = np.zeros((3, 4, 4, 3))
    assert L.rt_accum_add_sub(a, sub.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1) == NODEVICE
    assert b"no HIP device" in L.rt_last_error()
    assert L.rt_accum_add_sub_device(a, ctypes.c_void_p(16), 1, None) == NODEVICE
    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    p = rt.make_params(4, 3, 8, 1, None, rt.FLAG_MEGAKERNEL, 0, 1)
    assert L.rt_accum_add(a, sc.handle, ctypes.byref(p), None, None) == NODEVICE
    info = np.zeros(4, dtype=np.int64)
    assert L.rt_accum_info(a, info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == 0 and info.tolist() == [0, 0, 4, 3]
    L.rt_accum_destroy(a)
    keep, args = _denoise_var_args()
    assert L.rt_denoise_var(*args) == NODEVICE
    assert L.rt_denoise_var_device(*_dev_form(args), None) == NODEVICE
    with pytest.raises(rt.RtError) as e:
        with rt.Accumulator(4, 3) as acc:
            acc.add_sub(sub, 1)
    assert e.value.code == NODEVICE


# The restatement's own checks ------------------------------------------------------------------------------

def test_ref_weighted_variance_is_the_direct_one():
    """S and Q with n = (1, 2, 5) give the weighted variance a direct two-pass computation gives, and its mean."""
    ns = (1, 2, 5)
    passes = aref.synthetic_passes(7, 5, ns)
    acc = aref.Accum(7, 5)
    for m, n in zip(passes, ns):
        acc.add_sub(m, n)
    assert (acc.K, acc.N) == (3, 8)
    want, mean = aref.direct_variance(passes, ns)
    m = acc.sub()
    assert np.abs(m - mean).max() <= 1e-15
    vs = np.maximum(acc.Q / acc.N - m * m, 0.0) / (acc.K - 1)
    assert np.abs(vs - want).max() <= 1e-14 and want.max() > 0.05
    # the pixel variance: the subpixels inside (0, 1) only, over 16; [3] is the channels' sum
    inside = (m > 0) & (m < 1)
    assert 0.3 < inside.mean() < 0.8
    v = (np.where(inside, want, 0.0).sum(2) / 16.0)
    got = acc.var()
    assert got.dtype == np.float32 and np.abs(got[..., :3] - v).max() <= 1e-7 * v.max()
    assert np.abs(got[..., 3] - v.sum(-1)).max() <= 1e-7 * v.sum(-1).max()


def test_ref_first_pass_and_reset():
    passes = aref.synthetic_passes(3, 2)
    a, b = aref.Accum(3, 2), aref.Accum(3, 2)
    a.add_sub(passes[0], 2)
    assert np.array_equal(a.sub(), (2.0 * passes[0]) / 2.0) and np.array_equal(a.sub(), passes[0])
    a.add_sub(passes[1], 3)
    a.reset()
    for acc in (a, b):
        acc.add_sub(passes[2], 1)
        acc.add_sub(passes[1], 5)
    assert np.array_equal(a.sub(), b.sub()) and np.array_equal(a.var(), b.var())


def test_ref_levels_zero_is_identity():
    sub, feat = ref.synthetic(23, 11)
    var = aref.synthetic_var(23, 11)
    c, v = aref.atrous_var(sub, feat, var, 0, **ref.SIGMA_ON)
    assert np.array_equal(c, ref.c0_of(sub)) and np.array_equal(v, var[..., 3].astype(np.float64))


@pytest.mark.parametrize("levels", (1, 2, 3))
def test_ref_dependency_radius(levels):
    """Changing one input pixel (colour, features and variance) leaves every output farther than 2 (2^levels - 1)
    away bit-identical: the variance tent's reach (1 step) stays inside the filter's (2 steps)."""
    w, h = 40, 33
    sub, feat = ref.synthetic(w, h)
    var = aref.synthetic_var(w, h)
    base_c, base_v = aref.atrous_var(sub, feat, var, levels, **ref.SIGMA_ON)
    py, px = 15, 19
    sub2, feat2, var2 = sub.copy(), feat.copy(), var.copy()
    sub2[py, px] = 1.0 - np.clip(sub[py, px], 0, 1)
    feat2[py, px] = feat[(py + 5) % h, (px + 7) % w]
    var2[py, px] = var[py, px] * 7.0
    out_c, out_v = aref.atrous_var(sub2, feat2, var2, levels, **ref.SIGMA_ON)
    r = 2 * (2 ** levels - 1)
    yy, xx = np.mgrid[0:h, 0:w]
    far = np.maximum(np.abs(yy - py), np.abs(xx - px)) > r
    assert far.any() and np.array_equal(out_c[far], base_c[far]) and np.array_equal(out_v[far], base_v[far])
    near = ~far
    assert not np.array_equal(out_c[near], base_c[near])
    edge = np.maximum(np.abs(yy - py), np.abs(xx - px)) == r
    assert not np.array_equal(out_c[edge], base_c[edge])  # and the radius is reached


def test_ref_huge_variance_is_the_filter_without_colour_term():
    """v = 1e30 makes the colour term vanish: denoise_ref.atrous(sigma_c = 0) to 1e-12."""
    sub, feat = ref.synthetic(37, 21)
    var = np.full((21, 37, 4), 1e30, dtype=np.float32)
    for levels in (1, 3):
        c, _ = aref.atrous_var(sub, feat, var, levels, **ref.SIGMA_ON)
        want = ref.atrous(sub, feat, levels, **dict(ref.SIGMA_ON, sigma_c=0.0))
        assert np.abs(c - want).max() <= 1e-12


def test_ref_zero_variance_moves_nothing():
    """v = 0: the colour term is |c_p - c_q|^2 * 1e10, so a tap pulls by at most D exp(-D^2 1e10) <= 4.3e-6
    (D = 7.07e-6) times its h h / (9/64) <= 1; over the 24 taps and the levels here that stays below the derived
    bound of 1e-4 (every other term off, so nothing else stops the taps)."""
    sub, feat = ref.synthetic(37, 21)
    var = np.zeros((21, 37, 4), dtype=np.float32)
    off = dict(sigma_c=1.0, sigma_n=0.0, sigma_z=0.0, sigma_a=0.0)
    for dtype in (np.float64, np.float32):
        c, v = aref.atrous_var(sub, feat, var, 3, dtype=dtype, **off)
        assert np.abs(c.astype(np.float64) - ref.c0_of(sub)).max() <= 1e-4
        assert np.array_equal(v, np.zeros_like(v))
    # smooth inputs, where neighbours do differ by about 1e-5: still within the bound
    ramp = np.zeros((21, 37, 4, 3)) + (np.arange(37) * 7e-6)[None, :, None, None] + 0.3
    c, _ = aref.atrous_var(ramp, feat, var, 3, **off)
    d = np.abs(c - ref.c0_of(ramp)).max()
    assert 0 < d <= 1e-4


def test_d32v_is_the_recorded_value():
    """The GPU filter test's tolerance inputs: the largest f32-vs-f64 difference of the restatement over that test's
    cases, for the colour (absolute) and the filtered variance (relative). The recorded constants are this measurement
    (numpy's f32 exp may differ by an ulp between builds, hence the factor)."""
    d32v, dvar = aref.measure_d32v()
    print(f"d32v = {d32v:.3e}, relative variance difference = {dvar:.3e}")
    assert aref.D32V / 1.5 <= d32v <= aref.D32V * 1.5
    assert aref.D32V_VAR_REL / 1.5 <= dvar <= aref.D32V_VAR_REL * 1.5


# The estimator against the oracle ----------------------------------------------------------------------------

# re-measured here (test_variance_estimate_is_valid prints them): frame-sum ratio per group, mean and sd over the groups
FRAME_RATIO_MEAN, FRAME_RATIO_SD = 0.821, 0.037


def test_variance_estimate_is_valid(oracle_scenes):
    """cornell_box 48 x 36, 128 oracle passes of 16 spp, seeds 1000 + k 0x9E3779B9, in 16 groups of 8. Each group's
    passes accumulate to a frame and a variance estimate; the truth is the sample variance of the 16 accumulated clamped
    frames (channels summed). The per-pixel median of (mean group estimate / sample variance) lies in [0.9, 1.1];
    each group's ratio of frame sums lies within the recorded mean +- 6 sd.
    Measured: median 0.985; frame-sum ratio 0.821 +- 0.037 over the groups (0.776 .. 0.893), recorded below and in
    DESIGN.md §12."""
    w, h, groups, per = 48, 36, 16, 8
    sc = oracle_scenes["cornell_box"]
    est, frames = [], []
    for g in range(groups):
        acc = aref.Accum(w, h)
        for k in range(g * per, (g + 1) * per):
            _, sub, _ = sc.render(w, h, 16, 1000 + k * 0x9E3779B9)
            acc.add_sub(sub, 4)
        est.append(acc.var()[..., 3].astype(np.float64))
        frames.append(aref.c_of(acc.sub()))
    est, frames = np.stack(est), np.stack(frames)
    truth = frames.var(axis=0, ddof=1).sum(-1)
    ok = truth > 0
    assert ok.mean() > 0.9
    median = float(np.median(est.mean(0)[ok] / truth[ok]))
    ratios = est.reshape(groups, -1).sum(1) / truth.sum()
    print(f"per-pixel median ratio {median:.3f}; frame-sum ratio mean {ratios.mean():.3f} sd {ratios.std(ddof=1):.3f} "
          f"range {ratios.min():.3f}..{ratios.max():.3f}")
    assert 0.9 <= median <= 1.1
    assert np.all(np.abs(ratios - FRAME_RATIO_MEAN) <= 6 * FRAME_RATIO_SD)
