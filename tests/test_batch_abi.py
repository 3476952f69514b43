"""Batched error-target passes (rt_render_pixel_passes, rt_accum_plan, rt_accum_add_passes, rt_accum_refine; DESIGN.md
§17), the part that needs no GPU: the new C entry points are exported, declared for Rust and mirrored in rt_amd; every
bad argument is RT_E_INVAL with a message before any device call; the server's RT_TARGET_BATCH; and the numpy
restatement the GPU tests compare against (tests/batch_ref.py) has the defining properties."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import accum_ref as aref
import adapt_ref as dref
import batch_ref as br
from conftest import REPO, scene_path

NAMES = ("rt_render_pixel_passes", "rt_render_pixel_passes_device", "rt_accum_plan", "rt_accum_plan_device",
         "rt_accum_add_passes", "rt_accum_refine")
INVAL, NODEVICE = -1, -6
U8 = ctypes.POINTER(ctypes.c_uint8)
U32 = ctypes.POINTER(ctypes.c_uint32)
U64 = ctypes.POINTER(ctypes.c_uint64)
I64 = ctypes.POINTER(ctypes.c_int64)
D = ctypes.POINTER(ctypes.c_double)
NAN = float("nan")


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
    assert re.search(r"#define RT_PASSES_MAX\s+16\b", header) and rt.PASSES_MAX == br.PASSES_MAX == 16
    assert callable(rt.render_pixel_passes)
    for m in ("plan", "add_passes", "refine"):
        assert callable(getattr(rt.Accumulator, m))
    sig = inspect.signature(rt.render_to_error).parameters
    assert sig["batch"].default == 0 and sig["gain"].default is None  # the sequential loop unless asked for
    d = rt.ERROR_TARGET_BATCH_DEFAULTS
    assert set(d) == {"batch", "gain"} and 1 <= d["batch"] <= 16 and 0.0 < d["gain"] <= 1.0


def test_render_pixel_passes_bad_arguments_are_inval(rt):
    """Nulls, a count of 0 or above n_seeds, n_seeds of 0 or 17, more than width * height units, the FP32 and NEAREST
    flags, a partial frame and an unsorted list: RT_E_INVAL before any device call. Valid arguments without a device
    are RT_E_NODEVICE."""
    L = rt.lib
    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    MK = rt.FLAG_MEGAKERNEL
    good = rt.make_params(8, 6, 8, 1, None, MK, 0, 1)
    px = np.array([0, 5, 47], dtype=np.uint32)
    ct = np.array([1, 3, 2], dtype=np.uint8)
    sd = np.arange(1, 17, dtype=np.uint64)
    sub = np.full((6, 4, 3), 7.0)
    rgb = np.zeros((6, 3), dtype=np.uint8)

    def host(p=good, ids=px, counts=ct, scene=sc.handle, seeds=sd, n_seeds=3, n=None):
        return L.rt_render_pixel_passes(scene, ctypes.byref(p) if p is not None else None,
                                        ids.ctypes.data_as(U32) if ids is not None else None,
                                        counts.ctypes.data_as(U8) if counts is not None else None,
                                        (0 if ids is None else ids.size) if n is None else n,
                                        seeds.ctypes.data_as(U64) if seeds is not None else None, n_seeds,
                                        rgb.ctypes.data_as(U8), sub.ctypes.data_as(D), None, None)

    def dev(p=good, n=3, units=6, scene=sc.handle, ptr=ctypes.c_void_p(16), cptr=ctypes.c_void_p(32), seeds=sd, n_seeds=3):
        return L.rt_render_pixel_passes_device(scene, ctypes.byref(p) if p is not None else None, ptr, cptr, n, units,
                                               seeds.ctypes.data_as(U64) if seeds is not None else None, n_seeds, None,
                                               ctypes.c_void_p(64), None, None)

    for f in (host, dev):
        _is_inval(rt, f(scene=None), b"null")
        _is_inval(rt, f(p=None), b"null")
        _is_inval(rt, f(seeds=None), b"null seeds")
        for ns in (0, 17, -1):
            _is_inval(rt, f(n_seeds=ns), b"n_seeds")
        for p in (rt.make_params(8, 6, 8, 1, (0, 0, 8, 5), MK), rt.make_params(8, 6, 8, 1, (1, 0, 7, 6), MK),
                  rt.make_params(16, 12, 8, 1, (0, 0, 8, 6), MK)):
            _is_inval(rt, f(p=p), b"whole frame")
        _is_inval(rt, f(p=rt.make_params(8, 6, 8, 1, None, MK, row_step=2)))
        for flag in (rt.FLAG_FP32, rt.FLAG_MESH_NEAREST):
            _is_inval(rt, f(p=rt.make_params(8, 6, 8, 1, None, MK | flag)), b"not supported")
    _is_inval(rt, host(ids=None, n=3), b"null pixel list")
    _is_inval(rt, host(counts=None), b"null count list")
    _is_inval(rt, dev(ptr=None), b"null pixel list")
    _is_inval(rt, dev(cptr=None), b"null count list")
    for counts in ([0, 1, 1], [1, 4, 1], [1, 1, 255]):
        _is_inval(rt, host(counts=np.array(counts, dtype=np.uint8)), b"count")
    _is_inval(rt, host(n_seeds=2), b"count")  # a count of 3 with two seeds
    for ids, word in (([5, 3, 47], b"ascending"), ([3, 3, 4], b"ascending"), ([0, 1, 48], b"outside")):
        _is_inval(rt, host(ids=np.array(ids, dtype=np.uint32)), word)
    # more than width * height units: 4 x 3 pixels with 2 passes each fit, 13 units do not
    small = rt.make_params(4, 3, 8, 1, None, MK, 0, 1)
    ids12 = np.arange(12, dtype=np.uint32)
    many = np.ones(12, dtype=np.uint8)
    many[3] = 2
    _is_inval(rt, host(p=small, ids=ids12, counts=many, n_seeds=16), b"units")
    for units in (2, 10, 49):  # below n_pixels, above n_pixels * n_seeds, above the frame
        _is_inval(rt, dev(units=units, n_seeds=3 if units != 49 else 16, n=3 if units != 49 else 48), b"units")
    assert np.all(sub == 7.0) and np.all(rgb == 0)  # never written on failure
    # an empty list is RT_OK without a launch
    assert host(ids=np.zeros(0, dtype=np.uint32), counts=np.zeros(0, dtype=np.uint8)) == 0
    assert dev(n=0, units=0, ptr=None, cptr=None) == 0
    if rt.device_count() == 0:
        assert host() == NODEVICE and dev() == NODEVICE
        assert host(p=rt.make_params(8, 6, 8, 1, None, MK | rt.FLAG_MIS), n_seeds=16) == NODEVICE
        with pytest.raises(rt.RtError) as e:
            rt.render_pixel_passes(sc, 8, 6, [0, 5], [1, 2], 8, [11, 12])
        assert e.value.code == NODEVICE


def test_plan_bad_arguments_are_inval(rt):
    """rt_accum_plan and its device form: nulls, bad tolerances, gain of 0, above 1 or NaN, n < 1, max_passes of 0 or
    17, a bad output buffer, and K < 2 (asked for last, so every other check is reachable here)."""
    L = rt.lib
    a = _new_accum(rt)
    ids = np.full(48, 7, dtype=np.uint32)
    cnt = np.full(48, 9, dtype=np.uint8)
    n, units, passes = ctypes.c_int64(-5), ctypes.c_int64(-6), ctypes.c_int64(-7)

    def host(acc=a, abs_tol=0.04, rel_tol=0.0, max_n=0, nn=4, gain=1.0, C=16, p=ids.ctypes.data_as(U32),
             c=cnt.ctypes.data_as(U8), cap=48, n_out=ctypes.byref(n)):
        return L.rt_accum_plan(acc, abs_tol, rel_tol, max_n, nn, gain, C, p, c, cap, n_out, ctypes.byref(units),
                               ctypes.byref(passes))

    def dev(acc=a, abs_tol=0.04, rel_tol=0.0, max_n=0, nn=4, gain=1.0, C=16, p=ctypes.c_void_p(16), c=ctypes.c_void_p(32),
            cap=48, n_out=ctypes.byref(n)):
        return L.rt_accum_plan_device(acc, abs_tol, rel_tol, max_n, nn, gain, C, p, c, cap, n_out, ctypes.byref(units),
                                      ctypes.byref(passes), None)

    try:
        for f in (host, dev):
            _is_inval(rt, f(acc=None), b"null")
            _is_inval(rt, f(n_out=None), b"null")
            for tol in (-1.0, NAN):
                _is_inval(rt, f(abs_tol=tol), b"tolerances")
                _is_inval(rt, f(rel_tol=tol), b"tolerances")
            for gain in (0.0, -0.5, 1.5, NAN):
                _is_inval(rt, f(gain=gain), b"gain")
            for nn in (0, -4):
                _is_inval(rt, f(nn=nn), b"n must be")
            for C in (0, 17, -1):
                _is_inval(rt, f(C=C), b"max_passes")
            _is_inval(rt, f(cap=-1), b"output buffer")
            _is_inval(rt, f(p=None), b"output buffer")
            _is_inval(rt, f(c=None), b"output buffer")
            # every argument good: only the two passes are missing
            for kw in (dict(), dict(gain=0.25, C=1, nn=1), dict(max_n=124, rel_tol=0.1), dict(p=None, c=None, cap=0)):
                _is_inval(rt, f(**kw), b"two passes")
        assert (n.value, units.value, passes.value) == (-5, -6, -7) and (ids == 7).all() and (cnt == 9).all()
    finally:
        L.rt_accum_destroy(a)


def test_add_passes_and_refine_bad_arguments_are_inval(rt):
    """rt_accum_add_passes and rt_accum_refine: nulls, params that are not the accumulator's whole frame or device,
    spp < 4, the FP32 and NEAREST flags, bad seeds, counts and lists, a bad gain, and K < 2 last."""
    L = rt.lib
    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    a = _new_accum(rt)
    MK = rt.FLAG_MEGAKERNEL
    good = rt.make_params(8, 6, 8, 1, None, MK, 0, 1)
    px = np.array([0, 5, 47], dtype=np.uint32)
    ct = np.array([1, 3, 2], dtype=np.uint8)
    sd = np.arange(1, 17, dtype=np.uint64)
    st = rt.RenderStats()
    out3 = (ctypes.c_int64 * 3)(-3, -4, -5)

    def add(p=good, acc=a, scene=sc.handle, ids=px, counts=ct, seeds=sd, n_seeds=3):
        return L.rt_accum_add_passes(acc, scene, ctypes.byref(p) if p is not None else None,
                                     seeds.ctypes.data_as(U64) if seeds is not None else None, n_seeds,
                                     ids.ctypes.data_as(U32) if ids is not None else None,
                                     counts.ctypes.data_as(U8) if counts is not None else None, px.size, None,
                                     ctypes.byref(st))

    def refine(p=good, acc=a, scene=sc.handle, abs_tol=0.04, rel_tol=0.0, max_n=0, gain=0.5, seeds=sd, n_seeds=8):
        return L.rt_accum_refine(acc, scene, ctypes.byref(p) if p is not None else None, abs_tol, rel_tol, max_n, gain,
                                 seeds.ctypes.data_as(U64) if seeds is not None else None, n_seeds, None,
                                 ctypes.byref(st), out3)

    try:
        for f in (add, refine):
            _is_inval(rt, f(acc=None), b"null")
            _is_inval(rt, f(scene=None), b"null")
            _is_inval(rt, f(p=None), b"null")
            _is_inval(rt, f(seeds=None), b"null seeds")
            for p in (rt.make_params(8, 6, 8, 1, (0, 0, 8, 5), MK), rt.make_params(8, 6, 8, 1, (1, 0, 7, 6), MK),
                      rt.make_params(16, 12, 8, 1, (0, 0, 8, 6), MK), rt.make_params(8, 5, 8, 1, None, MK)):
                _is_inval(rt, f(p), b"whole frame")
            _is_inval(rt, f(rt.make_params(8, 6, 8, 1, None, MK, row_step=2)), b"row_step")
            for spp in (0, 3, -4):
                _is_inval(rt, f(rt.make_params(8, 6, spp, 1, None, MK)), b"spp")
            _is_inval(rt, f(rt.make_params(8, 6, 8, 1, None, MK, device=1)), b"device")
            for flag in (rt.FLAG_FP32, rt.FLAG_MESH_NEAREST):
                _is_inval(rt, f(rt.make_params(8, 6, 8, 1, None, MK | flag)), b"not supported")
            for ns in (0, 17):
                _is_inval(rt, f(n_seeds=ns), b"n_seeds")
        _is_inval(rt, add(ids=None), b"null pixel list")
        _is_inval(rt, add(counts=None), b"null count list")
        for counts in ([0, 1, 1], [1, 4, 1]):
            _is_inval(rt, add(counts=np.array(counts, dtype=np.uint8)), b"count")
        for ids, word in (([5, 3, 47], b"ascending"), ([0, 1, 48], b"outside")):
            _is_inval(rt, add(ids=np.array(ids, dtype=np.uint32)), word)
        _is_inval(rt, add(counts=np.array([16, 16, 16], dtype=np.uint8), n_seeds=15), b"count")
        _is_inval(rt, add(counts=np.array([17, 16, 16], dtype=np.uint8), n_seeds=16), b"count")
        for tol in (-1.0, NAN):
            _is_inval(rt, refine(abs_tol=tol), b"tolerances")
        for gain in (0.0, 1.25, NAN):
            _is_inval(rt, refine(gain=gain), b"gain")
        # good arguments, RT_FLAG_MIS included: only the two full-frame passes are missing
        for p in (good, rt.make_params(8, 6, 4, 1, None, MK | rt.FLAG_MIS), rt.make_params(8, 6, 36, 1, None, 0)):
            _is_inval(rt, add(p), b"two")
            _is_inval(rt, refine(p), b"two passes")
            _is_inval(rt, refine(p, n_seeds=1, gain=1.0, max_n=9), b"two passes")
        assert list(out3) == [-3, -4, -5]  # never written on failure
        info = np.zeros(4, dtype=np.int64)
        assert L.rt_accum_info(a, info.ctypes.data_as(I64)) == 0 and info.tolist() == [0, 0, 8, 6]
    finally:
        L.rt_accum_destroy(a)


def test_units_above_the_frame_are_inval(rt):
    """rt_accum_add_passes: 24 pixels of a 6 x 4 frame with one count of 2 make 25 units."""
    L = rt.lib
    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    a = _new_accum(rt, 6, 4)
    p = rt.make_params(6, 4, 8, 1, None, rt.FLAG_MEGAKERNEL, 0, 1)
    ids = np.arange(24, dtype=np.uint32)
    ct = np.ones(24, dtype=np.uint8)
    ct[7] = 2
    sd = np.arange(16, dtype=np.uint64)
    try:
        rc = L.rt_accum_add_passes(a, sc.handle, ctypes.byref(p), sd.ctypes.data_as(U64), 16, ids.ctypes.data_as(U32),
                                   ct.ctypes.data_as(U8), 24, None, None)
        _is_inval(rt, rc, b"units")
    finally:
        L.rt_accum_destroy(a)


def test_parse_batch_and_adaptive_job(rt, monkeypatch):
    """RT_TARGET_BATCH=<C>[,<gain>]; AdaptiveJob hands the two values to render_to_error only when set."""
    import asyncio

    from rt_amd import server

    assert server.parse_batch(None) == (0, None)
    assert server.parse_batch("8") == (8, None) and server.parse_batch("16,0.5") == (16, 0.5)
    assert server.parse_batch(" 4 , 1 ") == (4, 1.0)
    for bad in ("", "x", "0", "17", "-1", "8,0", "8,1.5", "8,nan", "8,0.5,2", "8,", "8.5"):
        with pytest.raises(ValueError):
            server.parse_batch(bad)
    seen = {}

    def fake(scene, width, height, **kw):
        seen.clear()
        seen.update(kw)
        yield np.zeros((height, width, 3), dtype=np.uint8), 16.0, 0.0

    monkeypatch.setattr(rt, "render_to_error", fake)

    async def send(msg):
        pass

    job = server.AdaptiveJob(send, 0.04, first=16)
    assert asyncio.run(job.run(None, 8, 3, 64, 9)) is False
    assert "batch" not in seen and "gain" not in seen and seen["abs_tol"] == 0.04
    job = server.AdaptiveJob(send, 0.04, first=16, batch=8)
    assert asyncio.run(job.run(None, 8, 3, 64, 9)) is False
    assert seen["batch"] == 8 and "gain" not in seen
    job = server.AdaptiveJob(send, 0.04, first=16, batch=4, gain=0.25)
    assert asyncio.run(job.run(None, 8, 3, 64, 9)) is False
    assert seen["batch"] == 4 and seen["gain"] == 0.25 and seen["max_spp"] == 64


# The restatement against its own properties ----------------------------------------------------------------

def _two_passes(w, h, seed=5):
    acc = dref.Accum(w, h)
    rng = np.random.default_rng(seed)
    acc.add_sub(rng.uniform(0.0, 1.2, size=(h, w, 4, 3)), 2)
    acc.add_sub(rng.uniform(0.0, 1.2, size=(h, w, 4, 3)), 2)
    return acc


def test_check_args():
    assert br.check_args(1, 1.0, 1) and br.check_args(4, 0.25, 16)
    for n, gain, C in ((0, 1.0, 4), (4, 0.0, 4), (4, 1.5, 4), (4, NAN, 4), (4, 0.5, 0), (4, 0.5, 17)):
        assert not br.check_args(n, gain, C)


def test_counts_all_one_is_the_sparse_merge():
    """add_runs with every count 1 is adapt_ref's sparse merge; with mixed counts, the pass-by-pass loop."""
    w, h, n = 7, 5, 3
    rng = np.random.default_rng(2)
    ids = np.array([0, 3, 4, 17, 34], dtype=np.uint32)
    a, b = _two_passes(w, h), _two_passes(w, h)
    m = rng.uniform(-0.2, 1.6, size=(ids.size, 4, 3))
    br.add_runs(a, ids, np.ones(ids.size, dtype=np.uint8), m, n)
    b.add_sub_pixels(ids, m, n)
    assert np.array_equal(a.S, b.S) and np.array_equal(a.Q, b.Q) and np.array_equal(a.cnt, b.cnt)
    ct = np.array([1, 3, 2, 1, 3], dtype=np.uint8)
    off = br.offsets(ct)
    assert off.tolist() == [0, 1, 4, 6, 7]
    m = rng.uniform(-0.2, 1.6, size=(int(ct.sum()), 4, 3))
    before = a.S.copy()
    br.add_runs(a, ids, ct, m, n)
    for i in range(3):
        has = ct > i
        b.add_sub_pixels(ids[has], m[off[has] + i], n)
    assert np.array_equal(a.S, b.S) and np.array_equal(a.Q, b.Q) and np.array_equal(a.cnt, b.cnt)
    k, nn = a.counts()
    assert k.reshape(-1)[ids].tolist() == [2 + 1 + c for c in ct] and nn.reshape(-1)[ids].tolist() == [4 + n + n * c for c in ct]
    rest = np.setdiff1d(np.arange(w * h), ids)
    assert np.array_equal(a.S.reshape(-1, 4, 3)[rest], before.reshape(-1, 4, 3)[rest])


def test_plan_ids_are_the_selection_and_counts_follow_the_need():
    w, h = 9, 7
    acc = _two_passes(w, h)
    v = acc.var()[..., 3].astype(np.float64)
    abs_tol = float(np.sqrt(np.median(dref.tent(v))))
    for gain, C, n in ((1.0, 16, 1), (0.5, 4, 2), (0.25, 1, 4)):
        ids, counts, units, passes = br.plan(acc, abs_tol, 0.0, 0, n, gain, C)
        assert np.array_equal(ids, dref.select(acc, abs_tol)) and 0 < ids.size < w * h
        assert counts.dtype == np.uint8 and counts.min() >= 1 and counts.max() <= C and passes == counts.max()
        assert units == int(counts.astype(np.int64).sum())
        # the definition, pixel by pixel in plain Python floats
        g = dref.tent(v).reshape(-1)
        thr = np.float64(np.float32(abs_tol))
        c1, _ = br.cap_of(br.wanted(acc.var(), acc.sub(), acc.counts()[1], abs_tol, 0.0, 0, n, gain, C), w * h, C)
        for e, p in enumerate(ids):
            x = (float(np.float32(gain)) * (4.0 * (g[p] / (thr * thr)) - 4.0)) / n
            want = C if x >= C else max(1, int(np.ceil(x)))
            assert counts[e] == min(want, c1)
    # thr = 0: every pixel with variance wants everything
    ids, counts, _, _ = br.plan(acc, 0.0, 0.0, 0, 4, 0.5, 1)
    assert ids.size == np.count_nonzero(dref.tent(v) > 0) and (counts == 1).all()
    want = br.wanted(acc.var(), acc.sub(), acc.counts()[1], 0.0, 0.0, 0, 4, 0.5, 16)
    assert set(np.unique(want)) <= {0, 16}


def test_max_n_clip():
    """max_n > 0: no pixel is planned past max_n + n - 1 samples, a pixel at max_n is not listed, and the clip is at
    least 1 for every listed pixel."""
    w, h, n = 6, 5, 3
    acc = _two_passes(w, h)                 # N = 4 everywhere
    ids = np.array([1, 2, 8], dtype=np.uint32)
    acc.add_sub_pixels(ids, np.random.default_rng(1).uniform(0, 1, size=(3, 4, 3)), 5)  # N_p = 9 there
    for max_n in (5, 9, 10, 12, 40):
        want = br.wanted(acc.var(), acc.sub(), acc.counts()[1], 0.0, 0.0, max_n, n, 1.0, 16)
        N = acc.counts()[1].astype(np.int64)
        listed = want > 0
        assert not listed[N >= max_n].any()
        assert (want[listed] >= 1).all() and (N[listed] + (want[listed] - 1) * n < max_n).all()
        room = (max_n - N + n - 1) // n
        assert (want[listed] == np.minimum(16, room[listed])).all()  # thr = 0: every listed pixel wants 16


def _want_6x4(k, c):
    want = np.zeros((4, 6), dtype=np.int64)
    want.reshape(-1)[np.arange(k) * 3 % 24 if k <= 8 else np.arange(k)] = c
    return want


def test_frame_cap():
    """The cap on a 6 x 4 frame: every pixel wanting 16 gives C' = 1; eight pixels wanting 4 give 24 units at C' = 3
    and 32 at C' = 4, so C' = 3; six pixels wanting 4 give C' = 4."""
    for k, c, C, want_c1, want_units in ((24, 16, 16, 1, 24), (8, 4, 16, 3, 24), (6, 4, 16, 4, 24), (8, 4, 2, 2, 16)):
        want = _want_6x4(k, c)
        assert np.count_nonzero(want) == k
        assert br.cap_of(want, 24, C) == (want_c1, want_units)
        ids, counts, units, passes = br.plan_of(want, C)
        assert ids.size == k and (counts == want_c1).all() and units == want_units and passes == want_c1
        assert units <= 24
    assert int(np.minimum(_want_6x4(8, 4), 4).sum()) == 32  # what C' = 4 would have needed
    # mixed: 20 pixels wanting 1 and 4 wanting 16 -> 20 + 4 C' <= 24 gives C' = 1
    want = np.ones((4, 6), dtype=np.int64)
    want.reshape(-1)[[0, 7, 14, 21]] = 16
    assert br.cap_of(want, 24, 16) == (1, 24)
    want.reshape(-1)[[1, 2, 3, 4, 5, 6, 8, 9]] = 0  # 12 + 4 C' <= 24 gives C' = 3
    assert br.cap_of(want, 24, 16) == (3, 24)
    ids, counts, units, passes = br.plan_of(np.zeros((4, 6), dtype=np.int64), 16)
    assert ids.size == 0 and counts.size == 0 and units == 0 and passes == 0
