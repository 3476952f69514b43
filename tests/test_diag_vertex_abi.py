"""The batch vertex diagnostics (include/rt_diag.h rt_diag_vertex / rt_diag_sincos), the part that needs no GPU: the
ctypes signatures match the header, bad arguments are RT_E_INVAL with a message before any device call, n == 0 is
RT_OK, valid arguments on a host without a GPU are RT_E_NODEVICE, and rt_amd mirrors both entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, scene_path

D, I32, U64 = ctypes.c_double, ctypes.c_int32, ctypes.c_uint64
# the forms each reference scene admits
ADMITS = {"cornell_box": {"DIAG_FUSED", "DIAG_FUSED_G0", "DIAG_FUSED_LDS"},
          "cubes": {"DIAG_FUSED", "DIAG_FUSED_G1", "DIAG_FUSED_LDS", "DIAG_SPLIT_SLOTS", "DIAG_SPLIT_KIDS",
                    "DIAG_SPLIT_FLAT", "DIAG_SPLIT_ROLES"},
          "flying_unicorn": {"DIAG_FUSED", "DIAG_FUSED_G1", "DIAG_FUSED_LDS", "DIAG_SPLIT_SLOTS", "DIAG_SPLIT_KIDS",
                             "DIAG_SPLIT_ROLES"}}
FORMS = ("DIAG_FUSED", "DIAG_FUSED_G0", "DIAG_SPLIT_SLOTS", "DIAG_SPLIT_KIDS", "DIAG_SPLIT_FLAT", "DIAG_FUSED_G1",
         "DIAG_FUSED_LDS", "DIAG_SPLIT_ROLES")
NEAREST_OK = ("DIAG_FUSED", "DIAG_FUSED_G1", "DIAG_FUSED_LDS")


@pytest.fixture(scope="module")
def scenes(rt):
    return {n: rt.Scene.from_toml(scene_path(n)) for n in ADMITS}


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _args(sc, form=0, flags=0, n=3):
    m = max(n, 1)
    st, rng, dk = np.zeros((m, 19)), np.ones((m, 2), np.uint64), np.zeros((m, 2), np.int32)
    st[:, 0:3], st[:, 3:6], st[:, 6:9] = [50.0, 52.0, 295.6], [0.0, 0.0, -1.0], 1.0
    so, ro, do, info = np.zeros((m, 19)), np.zeros((m, 2), np.uint64), np.zeros((m, 2), np.int32), np.zeros((m, 4), np.int32)
    keep = (st, rng, dk, so, ro, do, info)
    return keep, [sc.handle, 0, form, flags, n, _p(st, D), _p(rng, U64), _p(dk, I32), _p(so, D), _p(ro, U64), _p(do, I32),
                  _p(info, I32)]


def _is_inval(rt, rc):
    assert rc == -1, rc
    assert len(rt.lib.rt_last_error()) > 0


def test_signatures_match_the_header(rt):
    text = open(os.path.join(REPO, "include", "rt_diag.h")).read()
    assert "#define RT_DIAG_FUSED_LDS 6\n" in text and rt.DIAG_FUSED_LDS == 6
    assert "#define RT_DIAG_SPLIT_ROLES 7\n" in text and rt.DIAG_SPLIT_ROLES == 7
    ctype = {"const struct rt_scene*": ctypes.c_void_p, "int32_t": I32, "uint32_t": ctypes.c_uint32,
             "int64_t": ctypes.c_int64, "const double*": ctypes.POINTER(D), "double*": ctypes.POINTER(D),
             "const uint64_t*": ctypes.POINTER(U64), "uint64_t*": ctypes.POINTER(U64),
             "const int32_t*": ctypes.POINTER(I32), "int32_t*": ctypes.POINTER(I32)}
    for fn in ("rt_diag_vertex", "rt_diag_sincos"):
        m = re.search(r"\bint " + fn + r"\(([^;]*)\);", text)
        assert m, fn
        want = [ctype[re.sub(r"\s*\w+$", "", a.strip())] for a in " ".join(m.group(1).split()).split(",")]
        assert list(getattr(rt.lib, fn).argtypes) == want, fn
    assert callable(rt.Scene.diag_vertex) and callable(rt.diag_sincos)


def test_bad_arguments_are_inval(rt, scenes):
    sc = scenes["cubes"]
    for null_at in (0, 5, 6, 7, 8, 9, 10, 11):  # scene and every array
        keep, a = _args(sc)
        a[null_at] = None
        _is_inval(rt, rt.lib.rt_diag_vertex(*a))
    for n in (-1, -(1 << 40)):
        keep, a = _args(sc)
        a[4] = n
        _is_inval(rt, rt.lib.rt_diag_vertex(*a))
    for form in (-1, 8, 1 << 20):
        _is_inval(rt, rt.lib.rt_diag_vertex(*_args(sc, form=form)[1]))
    # the deferred-shadow forms walk octrees only: no nearest-triangle mode
    for form in (rt.DIAG_SPLIT_SLOTS, rt.DIAG_SPLIT_KIDS, rt.DIAG_SPLIT_FLAT, rt.DIAG_SPLIT_ROLES):
        _is_inval(rt, rt.lib.rt_diag_vertex(*_args(sc, form=form, flags=8)[1]))
        _is_inval(rt, rt.lib.rt_diag_vertex(*_args(sc, form=form, flags=9)[1]))
    # RT_FLAG_MIS (1) and RT_FLAG_MESH_NEAREST (8) are the only flags
    for flags in (2, 4, 16, 8 | 2, 1 << 31):
        _is_inval(rt, rt.lib.rt_diag_vertex(*_args(sc, flags=flags)[1]))
    x = np.zeros(4)
    for null_at in (2, 3, 4):
        a = [0, 4, _p(x, D), _p(x, D), _p(x, D)]
        a[null_at] = None
        _is_inval(rt, rt.lib.rt_diag_sincos(*a))
    _is_inval(rt, rt.lib.rt_diag_sincos(0, -1, _p(x, D), _p(x, D), _p(x, D)))


def test_forms_a_scene_does_not_admit_are_inval(rt, scenes):
    """FUSED_G0 needs a scene without meshes (and takes no mesh flag), FUSED_G1 and the split forms one with meshes,
    SPLIT_FLAT flat octrees."""
    for name, ok in ADMITS.items():
        for f in FORMS:
            if f in ok:
                continue
            _is_inval(rt, rt.lib.rt_diag_vertex(*_args(scenes[name], form=getattr(rt, f))[1]))
            with pytest.raises(rt.RtError) as e:
                scenes[name].diag_vertex(np.zeros((1, 19)), np.ones((1, 2), np.uint64), np.zeros((1, 2), np.int32),
                                         form=getattr(rt, f))
            assert e.value.code == -1
    _is_inval(rt, rt.lib.rt_diag_vertex(*_args(scenes["cornell_box"], form=rt.DIAG_FUSED_G0, flags=8)[1]))


def test_no_vertices_is_ok_and_valid_arguments_need_a_device(rt, scenes):
    for name, ok in ADMITS.items():
        for f in sorted(ok):
            for flags in ((0, 1, 8, 9) if f in NEAREST_OK else (0, 1)):
                assert rt.lib.rt_diag_vertex(*_args(scenes[name], form=getattr(rt, f), flags=flags, n=0)[1]) == 0
    out = scenes["cubes"].diag_vertex(np.zeros((0, 19)), np.zeros((0, 2), np.uint64), np.zeros((0, 2), np.int32))
    assert out["st"].shape == (0, 19) and out["info"].shape == (0, 4)
    x = np.zeros(1)
    assert rt.lib.rt_diag_sincos(0, 0, _p(x, D), _p(x, D), _p(x, D)) == 0
    want = 0 if rt.device_count() > 0 else -6
    keep, a = _args(scenes["cornell_box"], form=rt.DIAG_FUSED_LDS, flags=1)
    assert rt.lib.rt_diag_vertex(*a) == want
    assert rt.lib.rt_diag_sincos(0, 1, _p(x, D), _p(x, D), _p(x, D)) == want
    if want:
        assert b"no HIP device" in rt.lib.rt_last_error()
        with pytest.raises(rt.RtError) as e:
            rt.diag_sincos(np.zeros(2))
        assert e.value.code == -6
