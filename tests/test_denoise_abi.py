"""Denoised previews, the part that needs no GPU: the four C entry points are exported, declared for Rust and
mirrored in rt_amd; bad arguments are RT_E_INVAL with a message before any device call; and the numpy
restatement the GPU tests compare against (tests/denoise_ref.py) has the filter's defining properties."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import denoise_ref as ref
from conftest import REPO, scene_path

NAMES = ("rt_render_features", "rt_render_features_device", "rt_denoise", "rt_denoise_device")
SCENE_CASES = (("cornell_box", False), ("cubes", False), ("flying_unicorn", False), ("flying_unicorn", True))
FW, FH = 96, 72  # the feature tests' frame (tests/test_gpu_features.py)


def test_exported_declared_and_mirrored(rt):
    header = open(os.path.join(REPO, "include", "rt_ffi.h")).read()
    rust = open(os.path.join(REPO, "ffi", "raytracer_ffi.rs")).read()
    for n in NAMES:
        assert hasattr(rt.lib, n), f"missing export {n}"
        assert re.search(rf"^int {n}\(", header, re.M), f"{n} not declared in rt_ffi.h"
        assert re.search(rf"pub fn {n}\s*\(", rust), f"{n} not declared in raytracer_ffi.rs"
    assert "additive" in header
    for f in ("render_features", "denoise", "render_denoised"):
        assert callable(getattr(rt, f))
    assert set(rt.DENOISE_DEFAULTS) == {"levels", "sigma_c", "sigma_n", "sigma_z", "sigma_a"}
    assert 0 <= rt.DENOISE_DEFAULTS["levels"] <= 8
    from rt_amd import server
    assert callable(server.gpu_denoised_frame_renderer)


def _denoise_args(rt, w=4, h=3, levels=2, sig=(0.5, 0.5, 0.5, 0.5)):
    sub = np.zeros((h, w, 4, 3))
    feat = np.zeros((h, w, 8), dtype=np.float32)
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    lin = np.zeros((h, w, 3), dtype=np.float32)
    keep = (sub, feat, rgb, lin)
    P = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    return keep, [0, w, h, P(sub, ctypes.c_double), P(feat, ctypes.c_float), levels, *sig, P(rgb, ctypes.c_uint8),
                  P(lin, ctypes.c_float)]


def _is_inval(rt, rc):
    assert rc == -1, rc
    assert len(rt.lib.rt_last_error()) > 0


def test_denoise_bad_arguments_are_inval(rt):
    """Null buffers, sizes < 1, width * height beyond int32, levels outside 0..8 and a non-finite sigma are RT_E_INVAL
    with a message, for the host and the device entry point, checked before any device call (so also without a GPU)."""
    def both(args):
        _is_inval(rt, rt.lib.rt_denoise(*args))
        dev = list(args)
        for i in (3, 4, 10, 11):  # the device form takes the buffers as void*
            dev[i] = ctypes.cast(dev[i], ctypes.c_void_p) if dev[i] is not None else None
        _is_inval(rt, rt.lib.rt_denoise_device(*dev, None))

    for null_at in (3, 4, 10):  # sub, feat, rgb_out (lin_out is optional)
        keep, a = _denoise_args(rt)
        a[null_at] = None
        both(a)
    for w, h in ((0, 3), (4, 0), (-1, 3), (4, -7), (65536, 32768), (2 ** 31 - 1, 2)):
        keep, a = _denoise_args(rt)
        a[1], a[2] = w, h
        both(a)
    for levels in (-1, 9, 1 << 20):
        keep, a = _denoise_args(rt, levels=levels)
        both(a)
    for bad in (math.nan, math.inf, -math.inf):
        for k in range(4):
            sig = [0.5] * 4
            sig[k] = bad
            keep, a = _denoise_args(rt, sig=sig)
            both(a)


def test_features_bad_arguments_are_inval(rt):
    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    p = rt.make_params(8, 6, 0, 0, None, 0, 0, 1)
    out = np.zeros((6, 8, 8), dtype=np.float32)
    F = ctypes.POINTER(ctypes.c_float)
    _is_inval(rt, rt.lib.rt_render_features(None, ctypes.byref(p), out.ctypes.data_as(F)))
    _is_inval(rt, rt.lib.rt_render_features(sc.handle, None, out.ctypes.data_as(F)))
    _is_inval(rt, rt.lib.rt_render_features(sc.handle, ctypes.byref(p), None))
    _is_inval(rt, rt.lib.rt_render_features_device(None, ctypes.byref(p), ctypes.c_void_p(16), None))
    _is_inval(rt, rt.lib.rt_render_features_device(sc.handle, None, ctypes.c_void_p(16), None))
    _is_inval(rt, rt.lib.rt_render_features_device(sc.handle, ctypes.byref(p), None, None))
    for bad in (rt.make_params(0, 6, 0, 0, (0, 0, 1, 1)), rt.make_params(8, 6, 0, 0, (4, 0, 8, 6)),
                rt.make_params(8, 6, 0, 0, (0, 0, 8, 3), row_step=3)):
        _is_inval(rt, rt.lib.rt_render_features(sc.handle, ctypes.byref(bad), out.ctypes.data_as(F)))


def test_valid_arguments_without_a_gpu_are_nodevice(rt):
    """Valid arguments on a host without a GPU: RT_E_NODEVICE (-6) from all four, like the rest of the ABI. (With a
    device the host forms run: RT_OK; tests/test_gpu_denoise.py checks what they compute.)"""
    keep, a = _denoise_args(rt)
    if rt.device_count() > 0:
        assert rt.lib.rt_denoise(*a) == 0
        assert rt.render_features(rt.Scene.from_toml(scene_path("cornell_box")), 8, 6).shape == (6, 8, 8)
        return
    assert rt.lib.rt_denoise(*a) == -6 and b"no HIP device" in rt.lib.rt_last_error()
    dev = [ctypes.cast(x, ctypes.c_void_p) if i in (3, 4, 10, 11) else x for i, x in enumerate(a)]
    assert rt.lib.rt_denoise_device(*dev, None) == -6
    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    p = rt.make_params(8, 6, 0, 0, None, 0, 0, 1)
    out = np.zeros((6, 8, 8), dtype=np.float32)
    assert rt.lib.rt_render_features(sc.handle, ctypes.byref(p), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == -6
    assert rt.lib.rt_render_features_device(sc.handle, ctypes.byref(p), ctypes.c_void_p(16), None) == -6
    with pytest.raises(rt.RtError) as e:
        rt.render_features(sc, 8, 6)
    assert e.value.code == -6


# The restatement's own checks ------------------------------------------------------------------------------

def test_ref_levels_zero_is_identity():
    sub, feat = ref.synthetic(23, 11)
    assert np.array_equal(ref.atrous(sub, feat, 0, **ref.SIGMA_ON), ref.c0_of(sub))
    assert np.all(ref.c0_of(sub) <= 1.0) and ref.c0_of(sub).max() > 0.6


def test_ref_constant_image_is_a_fixed_point():
    sub, feat = ref.synthetic(23, 11)
    sub[:] = (0.25, 0.5, 0.75)
    out = ref.atrous(sub, feat, 4, **ref.SIGMA_ON)
    assert np.abs(out - np.array([0.25, 0.5, 0.75])).max() < 1e-14


@pytest.mark.parametrize("levels", (1, 2, 3))
def test_ref_dependency_radius(levels):
    """Changing one input pixel leaves every output farther than 2 (2^levels - 1) away (Chebyshev) bit-identical."""
    w, h = 40, 33
    sub, feat = ref.synthetic(w, h)
    base = ref.atrous(sub, feat, levels, **ref.SIGMA_ON)
    py, px = 15, 19
    sub2, feat2 = sub.copy(), feat.copy()
    sub2[py, px] = 1.0 - np.clip(sub[py, px], 0, 1)
    feat2[py, px] = feat[(py + 5) % h, (px + 7) % w]
    out = ref.atrous(sub2, feat2, levels, **ref.SIGMA_ON)
    r = 2 * (2 ** levels - 1)
    yy, xx = np.mgrid[0:h, 0:w]
    far = np.maximum(np.abs(yy - py), np.abs(xx - px)) > r
    assert far.any() and np.array_equal(out[far], base[far])
    assert not np.array_equal(out[~far], base[~far])


def test_d32_is_the_recorded_value():
    """The GPU filter test's tolerance input: the largest f32-vs-f64 difference of the restatement over that test's
    cases. The recorded constant (denoise_ref.D32) is this measurement (numpy's f32 exp may differ by an ulp between
    builds, hence the factor)."""
    d32 = ref.measure_d32()
    print(f"d32 = {d32:.3e}")
    assert ref.D32 / 1.5 <= d32 <= ref.D32 * 1.5


# The feature test's exclusion cap, on the CPU --------------------------------------------------------------

@pytest.mark.parametrize("name,nearest", SCENE_CASES)
def test_oracle_hit_objects_stable_under_one_ulp(oracle, name, nearest):
    """tests/test_gpu_features.py excludes pixels where the device and the oracle hit different objects, at most
    6 of 6,912. The oracle alone stays inside that cap when every direction component moves by one ulp: pixels whose
    hit objects change: cornell_box 0, cubes 0, flying_unicorn 0, flying_unicorn nearest-triangle 0."""
    sc = oracle.OracleScene(scene_path(name), mesh_nearest=nearest)
    o, d = ref.centre_rays(*ref.camera_of(scene_path(name)), FW, FH)
    _, ids, _, _ = ref.trace_parallel(sc, o, d)
    _, ids2, _, _ = ref.trace_parallel(sc, o, ref.nudged(d))
    changed = int((ids.reshape(-1, 4) != ids2.reshape(-1, 4)).any(-1).sum())
    print(f"{name} nearest={nearest}: {changed} pixels change their hit objects")
    assert (ids >= 0).mean() > 0.5
    assert changed <= 6
