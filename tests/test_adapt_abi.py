"""Rendering to a per-pixel error target, the part that needs no GPU: the new C entry points are exported, declared for
Rust and mirrored in rt_amd; every bad argument is RT_E_INVAL with a message before any device call; and the numpy
restatement the GPU tests compare against (tests/adapt_ref.py) has the defining properties."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import accum_ref as aref
import adapt_ref as dref
from conftest import REPO, scene_path

NAMES = ("rt_render_pixels", "rt_render_pixels_device", "rt_accum_add_pixels", "rt_accum_add_sub_pixels",
         "rt_accum_add_sub_pixels_device", "rt_accum_counts", "rt_accum_select", "rt_accum_select_device")
INVAL, NODEVICE = -1, -6
U32 = ctypes.POINTER(ctypes.c_uint32)
D = ctypes.POINTER(ctypes.c_double)
I64 = ctypes.POINTER(ctypes.c_int64)


def _u32(*ids):
    return np.array(ids, dtype=np.uint32)


def _is_inval(rt, rc, word=None):
    assert rc == INVAL, rc
    msg = rt.lib.rt_last_error()
    assert len(msg) > 0
    if word is not None:
        assert word in msg, msg


def test_exported_declared_and_mirrored(rt):
    header = open(os.path.join(REPO, "include", "rt_ffi.h")).read()
    rust = open(os.path.join(REPO, "ffi", "raytracer_ffi.rs")).read()
    for n in NAMES:
        assert hasattr(rt.lib, n), f"missing export {n}"
        assert re.search(rf"^int {n}\(", header, re.M), f"{n} not declared in rt_ffi.h"
        assert re.search(rf"pub fn {n}\s*\(", rust), f"{n} not declared in raytracer_ffi.rs"
        assert n in rt._EXPORTS
        assert getattr(rt.lib, n).argtypes is not None
    assert rt.lib.rt_abi_version() == 3
    for f in ("render_pixels", "render_to_error", "pass_seed"):
        assert callable(getattr(rt, f))
    for m in ("select", "add_pixels", "add_sub_pixels", "counts"):
        assert callable(getattr(rt.Accumulator, m))
    assert set(rt.ERROR_TARGET_DEFAULTS) == {"abs_tol", "rel_tol", "first", "pass_spp"}
    assert rt.ERROR_TARGET_DEFAULTS["rel_tol"] == 0 and rt.ERROR_TARGET_DEFAULTS["abs_tol"] > 0
    assert rt.pass_seed(77, 3) == aref.pass_seed(77, 3)


def test_render_pixels_bad_arguments_are_inval(rt):
    """Nulls, a partial-frame tile, row_step > 1, FP32 / MESH_NEAREST, and an unsorted, duplicate or out-of-range list:
    RT_E_INVAL before any device call (so also without a GPU); the device form checks everything but the list."""
    L = rt.lib
    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    good = rt.make_params(8, 6, 8, 1, None, rt.FLAG_MEGAKERNEL, 0, 1)
    px = _u32(0, 5, 47)
    sub = np.zeros((3, 4, 3))
    rgb = np.zeros((3, 3), dtype=np.uint8)
    U8 = ctypes.POINTER(ctypes.c_uint8)

    def host(p, ids, scene=sc.handle):
        return L.rt_render_pixels(scene, ctypes.byref(p) if p is not None else None,
                                  ids.ctypes.data_as(U32) if ids is not None else None, 0 if ids is None else ids.size,
                                  rgb.ctypes.data_as(U8), sub.ctypes.data_as(D), None, None)

    def dev(p, n, scene=sc.handle, ptr=ctypes.c_void_p(16)):
        return L.rt_render_pixels_device(scene, ctypes.byref(p) if p is not None else None, ptr, n, None,
                                         ctypes.c_void_p(16), None, None)

    _is_inval(rt, host(good, px, None))
    _is_inval(rt, host(None, px))
    _is_inval(rt, dev(good, 3, None))
    _is_inval(rt, dev(None, 3))
    _is_inval(rt, dev(good, 3, ptr=None), b"null pixel list")
    _is_inval(rt, L.rt_render_pixels(sc.handle, ctypes.byref(good), None, 3, None, None, None, None), b"null pixel list")
    bad = [rt.make_params(8, 6, 8, 1, (0, 0, 8, 5), rt.FLAG_MEGAKERNEL),     # partial frames
           rt.make_params(8, 6, 8, 1, (1, 0, 7, 6), rt.FLAG_MEGAKERNEL),
           rt.make_params(8, 6, 8, 1, (0, 1, 8, 5), rt.FLAG_MEGAKERNEL),
           rt.make_params(16, 12, 8, 1, (0, 0, 8, 6), rt.FLAG_MEGAKERNEL),
           rt.make_params(8, 6, 8, 1, None, rt.FLAG_MEGAKERNEL, row_step=2),
           rt.make_params(8, 6, 8, 1, None, rt.FLAG_MEGAKERNEL, row_step=-1),
           rt.make_params(0, 6, 8, 1, None, rt.FLAG_MEGAKERNEL),
           rt.make_params(8, 6, 8, 1, None, rt.FLAG_MEGAKERNEL | rt.FLAG_FP32),
           rt.make_params(8, 6, 8, 1, None, rt.FLAG_MEGAKERNEL | rt.FLAG_MESH_NEAREST)]
    for p in bad:
        _is_inval(rt, host(p, px))
        _is_inval(rt, dev(p, 3))
    for flag in (rt.FLAG_FP32, rt.FLAG_MESH_NEAREST):
        _is_inval(rt, host(rt.make_params(8, 6, 8, 1, None, flag), px), b"not supported")
    for n in (-1, 49, 1 << 40):  # more entries than pixels cannot be strictly ascending
        _is_inval(rt, dev(good, n), b"n_pixels")
    for ids, word in ((_u32(5, 3, 47), b"ascending"), (_u32(3, 3), b"ascending"), (_u32(0, 48), b"outside"),
                      (_u32(0xFFFFFFFF), b"outside"), (_u32(47, 0), b"ascending")):
        _is_inval(rt, host(good, ids), word)
    # an empty list is RT_OK without a launch (also without a GPU); the outputs stay untouched
    sub[:] = 7.0
    assert host(good, _u32()) == 0 and dev(good, 0) == 0 and dev(good, 0, ptr=None) == 0
    assert np.all(sub == 7.0) and np.all(rgb == 0)


def _new_accum(rt, w=4, h=3):
    a = ctypes.c_void_p()
    assert rt.lib.rt_accum_create(0, w, h, ctypes.byref(a)) == 0
    return a


def test_accum_sparse_bad_arguments_are_inval(rt):
    """K < 2, nulls, n < 1, bad lists, partial-frame params, FP32 / NEAREST flags and bad tolerances are RT_E_INVAL
    before any device call."""
    L = rt.lib
    a = _new_accum(rt)
    px = _u32(0, 5, 11)
    sub = np.zeros((3, 4, 3))
    P = lambda x: x.ctypes.data_as(U32)
    # K = 0: a sparse merge and a selection need two passes
    _is_inval(rt, L.rt_accum_add_sub_pixels(a, P(px), 3, sub.ctypes.data_as(D), 1), b"two full-frame passes")
    _is_inval(rt, L.rt_accum_add_sub_pixels_device(a, ctypes.c_void_p(16), 3, ctypes.c_void_p(16), 1, None),
              b"two full-frame passes")
    n_out = ctypes.c_int64(-5)
    out = np.zeros(12, dtype=np.uint32)
    _is_inval(rt, L.rt_accum_select(a, 0.04, 0.0, 0, P(out), 12, ctypes.byref(n_out)), b"two passes")
    _is_inval(rt, L.rt_accum_select_device(a, 0.04, 0.0, 0, ctypes.c_void_p(16), 12, ctypes.byref(n_out), None),
              b"two passes")
    assert n_out.value == -5
    # nulls and sizes
    _is_inval(rt, L.rt_accum_add_sub_pixels(None, P(px), 3, sub.ctypes.data_as(D), 1))
    _is_inval(rt, L.rt_accum_add_sub_pixels(a, None, 3, sub.ctypes.data_as(D), 1), b"null pixel list")
    _is_inval(rt, L.rt_accum_add_sub_pixels(a, P(px), 3, None, 1))
    _is_inval(rt, L.rt_accum_add_sub_pixels_device(a, None, 3, ctypes.c_void_p(16), 1, None))
    _is_inval(rt, L.rt_accum_add_sub_pixels_device(a, ctypes.c_void_p(16), 3, None, 1, None))
    for n in (0, -1):
        _is_inval(rt, L.rt_accum_add_sub_pixels(a, P(px), 3, sub.ctypes.data_as(D), n), b"n must be")
        _is_inval(rt, L.rt_accum_add_sub_pixels_device(a, ctypes.c_void_p(16), 3, ctypes.c_void_p(16), n, None))
    for cnt in (-1, 13):
        _is_inval(rt, L.rt_accum_add_sub_pixels(a, P(px), cnt, sub.ctypes.data_as(D), 1), b"n_pixels")
        _is_inval(rt, L.rt_accum_add_sub_pixels_device(a, ctypes.c_void_p(16), cnt, ctypes.c_void_p(16), 1, None))
    for ids, word in ((_u32(5, 0, 11), b"ascending"), (_u32(5, 5), b"ascending"), (_u32(0, 12), b"outside")):
        _is_inval(rt, L.rt_accum_add_sub_pixels(a, P(ids), ids.size, sub.ctypes.data_as(D), 1), word)
    _is_inval(rt, L.rt_accum_counts(None, None, None))
    # selection: tolerances, cap, nulls
    for at, rl in ((-0.01, 0.0), (0.04, -1.0), (math.nan, 0.0), (0.04, math.nan), (-math.inf, 0.0)):
        _is_inval(rt, L.rt_accum_select(a, at, rl, 0, P(out), 12, ctypes.byref(n_out)), b"tolerances")
        _is_inval(rt, L.rt_accum_select_device(a, at, rl, 0, ctypes.c_void_p(16), 12, ctypes.byref(n_out), None))
    _is_inval(rt, L.rt_accum_select(None, 0.04, 0.0, 0, P(out), 12, ctypes.byref(n_out)))
    _is_inval(rt, L.rt_accum_select(a, 0.04, 0.0, 0, P(out), 12, None))
    _is_inval(rt, L.rt_accum_select(a, 0.04, 0.0, 0, None, 12, ctypes.byref(n_out)), b"output buffer")
    _is_inval(rt, L.rt_accum_select(a, 0.04, 0.0, 0, P(out), -1, ctypes.byref(n_out)), b"output buffer")

    # rt_accum_add_pixels: rt_accum_add's and rt_render_pixels' rules, then the list, then K >= 2
    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    good = rt.make_params(4, 3, 8, 1, None, rt.FLAG_MEGAKERNEL, 0, 1)

    def add(p, ids, scene=sc.handle, acc=a):
        return L.rt_accum_add_pixels(acc, scene, ctypes.byref(p) if p is not None else None,
                                     P(ids) if ids is not None else None, 0 if ids is None else ids.size, None, None)

    _is_inval(rt, add(good, px, acc=None))
    _is_inval(rt, add(good, px, scene=None))
    _is_inval(rt, add(None, px))
    _is_inval(rt, L.rt_accum_add_pixels(a, sc.handle, ctypes.byref(good), None, 3, None, None), b"null pixel list")
    for p in (rt.make_params(4, 3, 8, 1, (0, 0, 4, 2), rt.FLAG_MEGAKERNEL), rt.make_params(8, 6, 8, 1, (0, 0, 4, 3)),
              rt.make_params(4, 3, 8, 1, row_step=2), rt.make_params(4, 3, 3, 1), rt.make_params(4, 3, 8, 1, device=1),
              rt.make_params(4, 3, 8, 1, None, rt.FLAG_FP32), rt.make_params(4, 3, 8, 1, None, rt.FLAG_MESH_NEAREST)):
        _is_inval(rt, add(p, px))
    _is_inval(rt, add(good, _u32(5, 0)), b"ascending")
    _is_inval(rt, add(good, _u32(0, 12)), b"outside")
    _is_inval(rt, add(good, px), b"two full-frame passes")

    # the counts of an accumulator without a sparse pass need no device: K and N everywhere
    k = np.full(12, 9, dtype=np.uint32)
    n = np.full(12, 9, dtype=np.uint32)
    assert L.rt_accum_counts(a, P(k), P(n)) == 0 and not k.any() and not n.any()
    info = np.zeros(4, dtype=np.int64)
    assert L.rt_accum_info(a, info.ctypes.data_as(I64)) == 0 and info.tolist() == [0, 0, 4, 3]
    L.rt_accum_destroy(a)


def test_valid_arguments_without_a_gpu_are_nodevice(rt):
    """Valid arguments on a host without a GPU: RT_E_NODEVICE (-6), like the rest of the ABI. (With a device the calls
    run; tests/test_gpu_render_pixels.py and tests/test_gpu_adapt.py check what they compute.)"""
    sc = rt.Scene.from_toml(scene_path("cornell_box"))
    if rt.device_count() > 0:
        rgb, sub, st = rt.render_pixels(sc, 8, 6, [], 8, want_sub=True)
        assert rgb.shape == (0, 3) and sub.shape == (0, 4, 3) and st["samples"] == 0
        return
    with pytest.raises(rt.RtError) as e:
        rt.render_pixels(sc, 8, 6, [0, 5], 8)
    assert e.value.code == NODEVICE


def test_adaptive_job_sends_every_frame_and_stops(rt, monkeypatch):
    """AdaptiveJob over a stand-in for render_to_error: every yielded frame goes out as the reference's chunk messages,
    the job ends after the frame with nothing active, and a stop between frames ends it early."""
    import asyncio

    from rt_amd import server

    w, h = 70, 3
    seen = {}

    def fake(scene, width, height, **kw):
        seen.update(kw, size=(width, height))
        for i, active in enumerate((0.5, 0.25, 0.0, 0.0)):
            yield np.full((height, width, 3), 10 * (i + 1), dtype=np.uint8), 16.0 * (i + 1), active

    monkeypatch.setattr(rt, "render_to_error", fake)
    sent = []

    async def send(msg):
        sent.append(msg)

    job = server.AdaptiveJob(send, 0.04, first=16)
    assert not job.running()
    assert asyncio.run(job.run(None, w, h, 64, 9)) is False and not job.running()
    per_frame = h * 2  # 70 pixels: two 60-pixel windows per row
    assert len(sent) == 3 * per_frame and sent[0][:2] == bytes([0, 60]) and sent[-1][6] == 30
    assert seen["abs_tol"] == 0.04 and seen["max_spp"] == 64 and seen["first"] == 16 and seen["seed"] == 9
    assert seen["size"] == (w, h)

    async def send_and_stop(msg):
        sent.append(msg)
        job.stop()

    del sent[:]
    job.send = send_and_stop
    assert asyncio.run(job.run(None, w, h, 64, 9)) is True and len(sent) == per_frame  # the frame in hand goes out


# The restatement's own checks ------------------------------------------------------------------------------

def _two_passes(w, h):
    acc = dref.Accum(w, h)
    passes = aref.synthetic_passes(w, h, (1, 2, 5))
    acc.add_sub(passes[0], 1)
    acc.add_sub(passes[1], 2)
    return acc, passes


def test_ref_without_sparse_pass_is_accum_ref():
    """No sparse pass: accum_ref.Accum's bits (one K and N for the frame)."""
    w, h = 7, 5
    acc, passes = _two_passes(w, h)
    old = aref.Accum(w, h)
    old.add_sub(passes[0], 1)
    old.add_sub(passes[1], 2)
    assert np.array_equal(acc.sub(), old.sub()) and np.array_equal(acc.var(), old.var())
    k, n = acc.counts()
    assert np.all(k == 2) and np.all(n == 3)


def test_ref_sparse_merge_touches_only_the_list():
    w, h = 7, 5
    acc, passes = _two_passes(w, h)
    before_sub, before_var = acc.sub(), acc.var()
    ids = np.arange(0, w * h, 2, dtype=np.uint32)
    acc.add_sub_pixels(ids, dref.gather(passes[2], ids), 5)
    k, n = acc.counts()
    inside = np.zeros(w * h, dtype=bool)
    inside[ids] = True
    inside = inside.reshape(h, w)
    assert np.all(k[inside] == 3) and np.all(n[inside] == 8) and np.all(k[~inside] == 2) and np.all(n[~inside] == 3)
    assert np.array_equal(acc.sub()[~inside], before_sub[~inside]) and np.array_equal(acc.var()[~inside], before_var[~inside])
    # the listed pixels are what a full accumulation of the three passes gives there
    full = aref.Accum(w, h)
    for m, nn in zip(passes, (1, 2, 5)):
        full.add_sub(m, nn)
    assert np.array_equal(acc.sub()[inside], full.sub()[inside]) and np.array_equal(acc.var()[inside], full.var()[inside])
    assert (acc.K, acc.N) == (2, 3)  # the full-frame passes only
    # a later full-frame pass bumps every pixel
    acc.add_sub(passes[0], 4)
    k, n = acc.counts()
    assert np.all(k[inside] == 4) and np.all(n[inside] == 12) and np.all(k[~inside] == 3) and np.all(n[~inside] == 7)


def test_ref_select_properties():
    """An all-zero variance selects nothing; a zero tolerance selects every pixel near a positive variance; max_n
    excludes pixels; the list is strictly ascending; rel_tol raises the threshold with the pixel's colour."""
    w, h = 9, 6
    sub = np.full((h, w, 4, 3), 0.5)
    n_p = np.full((h, w), 4, dtype=np.uint32)
    zero = np.zeros((h, w, 4), dtype=np.float32)
    assert not dref.select_mask(zero, sub, n_p, 0.0).any()
    assert not dref.select_mask(zero, sub, n_p, 0.04).any()
    var = zero.copy()
    var[2, 3, 3] = 1.0
    m = dref.select_mask(var, sub, n_p, 0.0)
    yy, xx = np.mgrid[0:h, 0:w]
    assert np.array_equal(m, (np.abs(yy - 2) <= 1) & (np.abs(xx - 3) <= 1))  # the tent's reach
    # g at the centre is 1/4, at an edge neighbour 1/8, at a corner neighbour 1/16 (interior weights sum to 1)
    assert dref.select_mask(var, sub, n_p, 0.3).sum() == 5 and dref.select_mask(var, sub, n_p, 0.36).sum() == 1
    assert not dref.select_mask(var, sub, n_p, 0.5).any()  # g = 1/4 is not above 0.5^2
    n2 = n_p.copy()
    n2[2, 3] = 8
    assert dref.select_mask(var, sub, n2, 0.0, max_n=8).sum() == 8 and not dref.select_mask(var, sub, n2, 0.0, max_n=4).any()
    assert dref.select_mask(var, sub, n2, 0.0, max_n=0).sum() == 9 and dref.select_mask(var, sub, n2, 0.0, max_n=-3).sum() == 9
    # y = 1.5 here: thr = rel_tol / 2
    assert dref.select_mask(var, sub, n_p, 0.0, rel_tol=0.6).sum() == 5
    acc, _ = _two_passes(23, 11)
    mid = float(np.sqrt(np.median(dref.tent(acc.var()[..., 3]))))  # about half the pixels lie above it
    ids = dref.select(acc, mid)
    assert ids.dtype == np.uint32 and 0 < ids.size < 23 * 11 and np.all(np.diff(ids.astype(np.int64)) > 0)
    assert dref.select(acc, 0.0).size >= ids.size and dref.select(acc, 10.0).size == 0
