"""The hole fill after a reprojection (rt_accum_holes, rt_accum_fill), the part that needs no GPU: the
new C entry points are exported, declared for Rust and mirrored in rt_amd; every bad argument is RT_E_INVAL with a
message before any device call; the server's RT_REPROJECT_FILL; and the numpy restatement the GPU tests compare
against (tests/fill_ref.py) has the defining properties."""
import ctypes
import os
import re

import numpy as np
import pytest

import fill_ref as fr
from conftest import REPO, scene_path

NAMES = ("rt_accum_holes", "rt_accum_holes_device", "rt_accum_fill")
INVAL = -1
U32 = ctypes.POINTER(ctypes.c_uint32)
I64 = ctypes.POINTER(ctypes.c_int64)


def _is_inval(rt, rc, word=None):
    assert rc == INVAL, rc
    msg = rt.lib.rt_last_error()
    assert len(msg) > 0
    if word is not None:
        assert word in msg, msg


def _new_accum(rt, w=8, h=6, device=0):
    a = ctypes.c_void_p()
    assert rt.lib.rt_accum_create(device, w, h, ctypes.byref(a)) == 0
    return a


def test_exported_declared_and_mirrored(rt):
    header = open(os.path.join(REPO, "include", "rt_ffi.h")).read()
    rust = open(os.path.join(REPO, "ffi", "raytracer_ffi.rs")).read()
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for n in NAMES:
        assert hasattr(rt.lib, n), f"missing export {n}"
        assert re.search(rf"^int {n}\(", header, re.M), f"{n} not declared in rt_ffi.h"
        assert re.search(rf"pub fn {n}\s*\(", rust), f"{n} not declared in raytracer_ffi.rs"
        assert n in rt._EXPORTS
        assert getattr(rt.lib, n).argtypes is not None
        assert n in text, f"{n} not in INTEGRATION.md"
    assert rt.lib.rt_abi_version() == 3  # additive
    for m in ("holes", "fill"):
        assert callable(getattr(rt.Accumulator, m))
    import inspect

    sig = inspect.signature(rt.render_interactive).parameters
    assert sig["fill_spp"].default == 0 and sig["refresh"].default == 0  # off unless asked for
    assert set(rt.FILL_DEFAULTS) == {"fill_spp", "refresh"}
    assert rt.FILL_DEFAULTS["fill_spp"] >= 4 and rt.FILL_DEFAULTS["fill_spp"] % 4 == 0 and rt.FILL_DEFAULTS["refresh"] >= 0
    # on by default only where it won: scenes without meshes
    off = dict(fill_spp=0, refresh=0)
    assert rt.fill_defaults_for(rt.Scene.from_toml(scene_path("cornell_box"))) == rt.FILL_DEFAULTS
    assert rt.fill_defaults_for(rt.Scene.from_toml(scene_path("cubes"))) == off
    assert rt.fill_defaults_for(rt.Scene.from_toml(scene_path("flying_unicorn"))) == off


def test_holes_bad_arguments_are_inval(rt):
    """Null handles, a negative or too small cap, a negative period, a phase outside 0 .. max(period, 1) - 1 and an
    accumulator that no reprojection seeded: RT_E_INVAL before any device call (so also without a GPU). The seeded
    state is asked for last, so every other check is reachable here."""
    L = rt.lib
    a = _new_accum(rt)
    out = np.full(48, 7, dtype=np.uint32)
    n, nh = ctypes.c_int64(-5), ctypes.c_int64(-6)
    P = out.ctypes.data_as(U32)
    dptr = ctypes.c_void_p(16)

    def host(acc=a, period=0, phase=0, ptr=P, cap=48, n_out=ctypes.byref(n)):
        return L.rt_accum_holes(acc, period, phase, ptr, cap, n_out, ctypes.byref(nh))

    def dev(acc=a, period=0, phase=0, ptr=dptr, cap=48, n_out=ctypes.byref(n)):
        return L.rt_accum_holes_device(acc, period, phase, ptr, cap, n_out, ctypes.byref(nh), None)

    try:
        for f in (host, dev):
            _is_inval(rt, f(acc=None), b"null")
            _is_inval(rt, f(n_out=None), b"null")
            _is_inval(rt, f(cap=-1), b"output buffer")
            _is_inval(rt, f(ptr=None), b"output buffer")
            for period in (-1, -7):
                _is_inval(rt, f(period=period), b"period")
            for period, phase in ((0, 1), (0, -1), (1, 1), (4, 4), (4, -1), (3, 1 << 20)):
                _is_inval(rt, f(period=period, phase=phase), b"phase")
            # every argument good: only the seeded state is missing
            for period, phase in ((0, 0), (1, 0), (4, 3)):
                _is_inval(rt, f(period=period, phase=phase), b"not seeded")
            _is_inval(rt, f(ptr=None, cap=0), b"not seeded")  # no buffer is needed for the counts alone
        assert n.value == -5 and nh.value == -6 and (out == 7).all()  # never written on failure
    finally:
        L.rt_accum_destroy(a)


def test_fill_bad_arguments_are_inval(rt):
    """rt_accum_fill: nulls, params that are not the accumulator's whole frame or device, spp < 4, RT_FLAG_FP32 and
    RT_FLAG_MESH_NEAREST, a bad period or phase, and an unseeded accumulator, all before any device call."""
    L = rt.lib
    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    a = _new_accum(rt)
    MK = rt.FLAG_MEGAKERNEL
    good = rt.make_params(8, 6, 8, 1, None, MK, 0, 1)
    st = rt.RenderStats()
    lens = (ctypes.c_int64 * 2)(-3, -4)

    def fill(p=good, acc=a, scene=sc.handle, period=0, phase=0):
        return L.rt_accum_fill(acc, scene, ctypes.byref(p) if p is not None else None, 99, period, phase, None,
                               ctypes.byref(st), lens)

    try:
        _is_inval(rt, fill(acc=None), b"null")
        _is_inval(rt, fill(scene=None), b"null")
        _is_inval(rt, fill(p=None), b"null")
        for p in (rt.make_params(8, 6, 8, 1, (0, 0, 8, 5), MK),      # partial frames
                  rt.make_params(8, 6, 8, 1, (1, 0, 7, 6), MK),
                  rt.make_params(8, 6, 8, 1, (0, 1, 8, 5), MK),
                  rt.make_params(16, 12, 8, 1, (0, 0, 8, 6), MK),
                  rt.make_params(8, 5, 8, 1, None, MK)):             # another frame than the accumulator's
            _is_inval(rt, fill(p), b"whole frame")
        _is_inval(rt, fill(rt.make_params(8, 6, 8, 1, None, MK, row_step=2)), b"row_step")
        for spp in (0, 3, -4):
            _is_inval(rt, fill(rt.make_params(8, 6, spp, 1, None, MK)), b"spp")
        _is_inval(rt, fill(rt.make_params(8, 6, 8, 1, None, MK, device=1)), b"device")
        for flag in (rt.FLAG_FP32, rt.FLAG_MESH_NEAREST):
            _is_inval(rt, fill(rt.make_params(8, 6, 8, 1, None, MK | flag)), b"not supported")
        _is_inval(rt, fill(period=-1), b"period")
        for period, phase in ((0, 1), (2, 2), (5, -1)):
            _is_inval(rt, fill(period=period, phase=phase), b"phase")
        # good arguments, RT_FLAG_MIS included: only the seeded state is missing
        for p in (good, rt.make_params(8, 6, 4, 1, None, MK | rt.FLAG_MIS), rt.make_params(8, 6, 36, 1, None, 0)):
            for period, phase in ((0, 0), (4, 1)):
                _is_inval(rt, fill(p, period=period, phase=phase), b"not seeded")
        assert list(lens) == [-3, -4]  # never written on failure
        info = np.zeros(4, dtype=np.int64)
        assert L.rt_accum_info(a, info.ctypes.data_as(I64)) == 0 and info.tolist() == [0, 0, 8, 6]
    finally:
        L.rt_accum_destroy(a)


def test_parse_fill(monkeypatch):
    """RT_REPROJECT_FILL=<spp>[,<refresh>]; unset leaves InteractiveJob as it was."""
    from rt_amd import server

    assert server.parse_fill(None) == (0, 0)
    assert server.parse_fill("16") == (16, 0) and server.parse_fill("8,4") == (8, 4) and server.parse_fill(" 4 , 1 ") == (4, 1)
    for bad in ("", "x", "3", "0", "8,-1", "8,4,2", "8,", "8.5"):
        with pytest.raises(ValueError):
            server.parse_fill(bad)

    async def send(_):
        pass

    monkeypatch.delenv("RT_REPROJECT_FILL", raising=False)
    job = server.InteractiveJob(send, max_n=16)
    assert (job.fill_spp, job.refresh) == (0, 0)
    monkeypatch.setenv("RT_REPROJECT_FILL", "16,4")
    job = server.InteractiveJob(send, max_n=16)
    assert (job.fill_spp, job.refresh) == (16, 4)


# The restatement against its own properties ----------------------------------------------------------------

def test_check_args():
    assert fr.check_args(0, 0) and fr.check_args(1, 0) and fr.check_args(4, 3)
    for period, phase in ((-1, 0), (0, 1), (0, -1), (1, 1), (4, 4), (4, -1)):
        assert not fr.check_args(period, phase)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 35)])
def test_hole_predicate(w, h):
    """period 0 lists exactly K_p < 2; period 1 lists everything; the R phases of period R partition the pixels with
    K_p >= 2, every phase holding all the holes; along a row and along a column consecutive pixels change phase (3 is
    coprime to the periods used, so a refresh never takes a whole row or column at once for R > 1)."""
    rng = np.random.default_rng(w * 100 + h)
    K = rng.integers(0, 5, size=(h, w))
    ids, count, n_holes = fr.holes(K)
    assert np.array_equal(ids, np.flatnonzero(K.reshape(-1) < 2)) and count == ids.size == n_holes
    assert ids.dtype == np.uint32
    ids1, count1, nh1 = fr.holes(K, 1, 0)
    assert count1 == w * h and nh1 == n_holes and np.array_equal(ids1, np.arange(w * h))
    for R in (2, 4, 5):
        seen = np.zeros((h, w), dtype=np.int64)
        for ph in range(R):
            m = fr.hole_mask(K, R, ph)
            assert m[K < 2].all()
            seen += m & (K >= 2)
            got, cnt, nh = fr.holes(K, R, ph, cap=3)
            assert cnt == int(m.sum()) and nh == n_holes and np.array_equal(got, np.flatnonzero(m)[:3])
        assert (seen[K >= 2] == 1).all()
        # the definition, pixel by pixel in plain Python integers
        for row in range(h):
            for col in range(w):
                want = K[row, col] < 2 or (col + 3 * row) % R == 1 % R
                assert fr.hole_mask(K, R, 1 % R)[row, col] == want


def _render(seed):
    def render(k, ids):
        rng = np.random.default_rng(seed + k)
        return rng.uniform(-0.2, 1.6, size=(len(ids), 4, 3))
    return render


def test_fill_gives_a_hole_what_two_full_passes_give_it():
    """A hole's sums are zeros: after the fill it holds n m1 + n m2 with counts (2, 2 n), bit for bit what two
    full-frame merges of the same passes give that pixel; a pixel with history is untouched at period 0."""
    w, h, n = 7, 5, 3
    rng = np.random.default_rng(3)
    K = np.array(rng.integers(0, 2, size=(h, w)) * 3)  # 0 or 3 passes
    N = K * 4
    S = np.where((K > 0)[..., None, None], rng.uniform(0.0, 9.0, size=(h, w, 4, 3)), 0.0)
    Q = S * 1.5
    full = [rng.uniform(-0.2, 1.6, size=(h, w, 4, 3)) for _ in range(2)]
    a, b = fr.Accum(w, h), fr.Accum(w, h)
    a.seed(S, Q, K, N)
    b.seed(S, Q, K, N)
    assert a.may("fill") and not a.may("resolve") and not a.may("select") and not a.may("reproject_src")
    lens = a.fill(lambda k, ids: full[k].reshape(-1, 4, 3)[ids], n)
    hole = K == 0
    assert lens == (int(hole.sum()), int(hole.sum())) and 0 < lens[0] < w * h
    assert a.covered and a.passes == 0 and all(a.may(x) for x in ("resolve", "var", "select", "sparse", "reproject_src"))
    for m in full:
        b.add_sub(m, n)
    assert not b.covered and b.passes == 2 and b.may("var")
    assert np.array_equal(a.S[hole], b.S[hole]) and np.array_equal(a.Q[hole], b.Q[hole])
    assert (a.K[hole] == 2).all() and (a.N[hole] == 2 * n).all()
    assert np.array_equal(a.sub()[hole], b.sub()[hole]) and np.array_equal(a.var()[hole], b.var()[hole])
    assert np.array_equal(a.S[~hole], S[~hole]) and np.array_equal(a.K[~hole], K[~hole])
    assert np.isfinite(a.var()).all()
    # the second fill of a covered accumulator lists nothing at period 0
    assert a.fill(_render(5), n) == (0, 0)
    a.reset()
    assert not a.seeded and not a.covered and not a.may("fill") and not a.K.any()


def test_refresh_and_cancel():
    """period R: a listed pixel with history gains exactly (1, n), the others nothing, the holes (2, 2 n). A pass
    cancelled merges nothing and leaves the accumulator uncovered; the next fill completes it."""
    w, h, n, R = 9, 4, 2, 4
    rng = np.random.default_rng(8)
    K = np.array(rng.integers(0, 2, size=(h, w)) * 5)
    N = K * 2
    S = np.where((K > 0)[..., None, None], rng.uniform(0.0, 9.0, size=(h, w, 4, 3)), 0.0)
    a = fr.Accum(w, h)
    a.seed(S, S, K, N)
    lens = a.fill(_render(1), n, R, 2)
    hole = K == 0
    listed = fr.hole_mask(K, R, 2)
    assert lens == (int(listed.sum()), int(hole.sum()))
    assert np.array_equal(a.K - K, np.where(hole, 2, np.where(listed, 1, 0)))
    assert np.array_equal(a.N - N, np.where(hole, 2 * n, np.where(listed, n, 0)))
    for cancel_pass in (0, 1):
        c = fr.Accum(w, h)
        c.seed(S, S, K, N)
        got = c.fill(_render(1), n, 0, 0, cancel_pass=cancel_pass)
        assert not c.covered and not c.may("resolve")
        assert got == ((int(hole.sum()), 0) if cancel_pass == 0 else (int(hole.sum()),) * 2)
        assert (c.K[hole] == cancel_pass).all()
        got = c.fill(_render(1), n)
        assert c.covered and (c.K >= 2).all()
        assert got == ((int(hole.sum()),) * 2 if cancel_pass == 0 else (int(hole.sum()), 0))
