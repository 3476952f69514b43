"""The batch query diagnostics (include/rt_diag.h rt_diag_trace / rt_diag_visible), the part that needs no GPU:
bad arguments are RT_E_INVAL with a message before any device call, n == 0 is RT_OK, valid arguments on a host
without a GPU are RT_E_NODEVICE, and rt_amd mirrors both entry points."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO, scene_path

D, I32, U8, U32 = ctypes.c_double, ctypes.c_int32, ctypes.c_uint8, ctypes.c_uint32
FORMS = ("DIAG_FUSED", "DIAG_FUSED_G0", "DIAG_SPLIT_SLOTS", "DIAG_SPLIT_KIDS", "DIAG_SPLIT_FLAT", "DIAG_FUSED_G1")
# the forms each reference scene admits (flags 0)
ADMITS = {"cornell_box": {"DIAG_FUSED", "DIAG_FUSED_G0"},
          "cubes": {"DIAG_FUSED", "DIAG_FUSED_G1", "DIAG_SPLIT_SLOTS", "DIAG_SPLIT_KIDS", "DIAG_SPLIT_FLAT"},
          "flying_unicorn": {"DIAG_FUSED", "DIAG_FUSED_G1", "DIAG_SPLIT_SLOTS", "DIAG_SPLIT_KIDS"}}


@pytest.fixture(scope="module")
def scenes(rt):
    return {n: rt.Scene.from_toml(scene_path(n)) for n in ADMITS}


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _trace_args(sc, form=0, flags=0, n=3):
    o = np.full((max(n, 1), 3), 50.0)
    d = np.tile([0.0, 0.0, -1.0], (max(n, 1), 1))
    t, obj, prim = np.zeros(max(n, 1)), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    pos, nrm = np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3))
    keep = (o, d, t, obj, prim, pos, nrm)
    return keep, [sc.handle, 0, form, flags, n, _p(o, D), _p(d, D), _p(t, D), _p(obj, I32), _p(prim, I32), _p(pos, D),
                  _p(nrm, D)]


def _vis_args(sc, form=0, flags=0, n=3):
    x = np.full((max(n, 1), 3), 50.0)
    y = np.full((max(n, 1), 3), 40.0)
    vis, near = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32)
    keep = (x, y, vis, near)
    return keep, [sc.handle, 0, form, flags, n, _p(x, D), _p(y, D), _p(vis, U8), _p(near, U32)]


def _is_inval(rt, rc):
    assert rc == -1, rc
    assert len(rt.lib.rt_last_error()) > 0


def test_mirrored(rt):
    assert [getattr(rt, f) for f in FORMS] == [0, 1, 2, 3, 4, 5]
    assert callable(rt.Scene.diag_trace) and callable(rt.Scene.diag_visible)
    text = open(os.path.join(REPO, "include", "rt_diag.h")).read()
    for k, f in enumerate(FORMS):
        assert f"#define RT_{f} {k}\n" in text


def test_bad_arguments_are_inval(rt, scenes):
    sc = scenes["cubes"]
    for null_at in (0, 5, 6, 7, 8, 9, 10, 11):  # scene, o, d, t, obj, prim, pos, nrm
        keep, a = _trace_args(sc)
        a[null_at] = None
        _is_inval(rt, rt.lib.rt_diag_trace(*a))
    for null_at in (0, 5, 6, 7):  # scene, x, y, vis (near_mask is optional)
        keep, a = _vis_args(sc)
        a[null_at] = None
        _is_inval(rt, rt.lib.rt_diag_visible(*a))
    for n in (-1, -(1 << 40)):
        keep, a = _trace_args(sc)
        a[4] = n
        _is_inval(rt, rt.lib.rt_diag_trace(*a))
        keep, a = _vis_args(sc)
        a[4] = n
        _is_inval(rt, rt.lib.rt_diag_visible(*a))
    for form in (-1, 6, 1 << 20):
        _is_inval(rt, rt.lib.rt_diag_trace(*_trace_args(sc, form=form)[1]))
        _is_inval(rt, rt.lib.rt_diag_visible(*_vis_args(sc, form=form)[1]))
    # RT_FLAG_MESH_NEAREST (8) is the only flag, and only the fused forms have a nearest-triangle mode
    for flags in (1, 2, 4, 16, 8 | 1, 1 << 31):
        _is_inval(rt, rt.lib.rt_diag_trace(*_trace_args(sc, flags=flags)[1]))
        _is_inval(rt, rt.lib.rt_diag_visible(*_vis_args(sc, flags=flags)[1]))
    for form in (rt.DIAG_SPLIT_SLOTS, rt.DIAG_SPLIT_KIDS, rt.DIAG_SPLIT_FLAT):
        _is_inval(rt, rt.lib.rt_diag_trace(*_trace_args(sc, form=form, flags=8)[1]))
        _is_inval(rt, rt.lib.rt_diag_visible(*_vis_args(sc, form=form, flags=8)[1]))


def test_forms_a_scene_does_not_admit_are_inval(rt, scenes):
    """FUSED_G0 needs a scene without meshes, FUSED_G1 and the split forms one with meshes, SPLIT_FLAT flat octrees."""
    for name, ok in ADMITS.items():
        for f in FORMS:
            if f in ok:
                continue
            _is_inval(rt, rt.lib.rt_diag_trace(*_trace_args(scenes[name], form=getattr(rt, f))[1]))
            _is_inval(rt, rt.lib.rt_diag_visible(*_vis_args(scenes[name], form=getattr(rt, f))[1]))
            with pytest.raises(rt.RtError) as e:
                scenes[name].diag_trace(np.zeros((1, 3)), np.ones((1, 3)), form=getattr(rt, f))
            assert e.value.code == -1


def test_no_queries_is_ok_and_valid_arguments_need_a_device(rt, scenes):
    """n == 0 needs no device: RT_OK. Valid arguments: RT_E_NODEVICE (-6) on a host without a GPU (with one they
    run: RT_OK; tests/test_gpu_queries.py checks what they compute). A near_mask of NULL is valid."""
    for name, ok in ADMITS.items():
        for f in sorted(ok):
            form = getattr(rt, f)
            for flags in ((0, 8) if f in ("DIAG_FUSED", "DIAG_FUSED_G1") else (0,)):
                assert rt.lib.rt_diag_trace(*_trace_args(scenes[name], form=form, flags=flags, n=0)[1]) == 0
                assert rt.lib.rt_diag_visible(*_vis_args(scenes[name], form=form, flags=flags, n=0)[1]) == 0
    t, ids, prim, pos, nrm = scenes["cubes"].diag_trace(np.zeros((0, 3)), np.zeros((0, 3)))
    assert t.shape == (0,) and pos.shape == (0, 3)
    want = 0 if rt.device_count() > 0 else -6
    sc = scenes["cornell_box"]
    for form in (rt.DIAG_FUSED, rt.DIAG_FUSED_G0):
        keep, a = _trace_args(sc, form=form)
        assert rt.lib.rt_diag_trace(*a) == want
        keep, a = _vis_args(sc, form=form)
        a[8] = None
        assert rt.lib.rt_diag_visible(*a) == want
        if want:
            assert b"no HIP device" in rt.lib.rt_last_error()
    if want:
        with pytest.raises(rt.RtError) as e:
            sc.diag_visible(np.zeros((2, 3)), np.ones((2, 3)))
        assert e.value.code == -6
