"""The hole fill after a reprojection on the device (rt_accum_holes, rt_accum_fill, k_holes_count)
against tests/fill_ref.py: hole lists, the filled accumulator bit for bit, the refresh pattern, the covered state, the
edge cases, and render_interactive / the server with the fill.

Seeded accumulators come from real reprojections of cornell_box with the moves A and B of tests/reproject_ref.py. Where
the comparison needs the seeded sums it takes them from reproject_ref over the oracle, as tests/test_gpu_reproject.py
does, and leaves out the pixels whose device queries disagree with the oracle's (_disagreeing_pixels; at most 0.1 %)."""
import asyncio
import ctypes
import struct

import numpy as np
import pytest

import accum_ref
import adapt_ref as dref
import fill_ref as fr
import reproject_ref as rr
from conftest import scene_path
from test_gpu_reproject import _disagreeing_pixels, _fill_src, _same

pytestmark = pytest.mark.gpu

SEED = 0x5EED
NAME = "cornell_box"
MOVES = dict(A=rr.MOVE_A, B=rr.MOVE_B)
_classified = {}


def _views(base, move):
    path = scene_path(NAME)
    v0, v1 = rr.scene_view(path), rr.scene_view(path, MOVES[move])
    return v0, v1, base.view(**rr.as_kwargs(v1))


def _classify(oracle_scenes, base, w, h, move):
    """(classification, pixels to keep) of the move at w x h, computed once."""
    key = (w, h, move)
    if key not in _classified:
        path = scene_path(NAME)
        v0, v1, _ = _views(base, move)
        c = rr.classify(oracle_scenes[NAME], rr.brdf_kinds(path), v1, v0, w, h)
        out = _disagreeing_pixels(base, c, v0["pos"], w, h)
        assert out.sum() <= 0.001 * w * h
        _classified[key] = (c, ~out)
    return _classified[key]


def _frames(rt, view, w, h, spp, seeds, mis=False):
    """The device's own rt_render frames of the two passes."""
    return [rt.render(view, w, h, spp, s, megakernel=True, want_sub=True, mis=mis)[1] for s in seeds]


def _gather(frames):
    return lambda k, ids: frames[k].reshape(-1, 4, 3)[np.asarray(ids, dtype=np.int64)]


def _raw_holes(rt, acc, period, phase, cap):
    ids = np.full(max(1, cap), 0xFFFFFFFF, dtype=np.uint32)
    n, nh = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rt._check(rt.lib.rt_accum_holes(acc.handle, period, phase, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap,
                                    ctypes.byref(n), ctypes.byref(nh)))
    return ids, n.value, nh.value


# Hole lists -----------------------------------------------------------------------------------------------------

# 1 x 1; 5 x 3; 67 x 35: no multiple of 64; 300 x 20: rows split across the 256-pixel blocks; 600 x 450: 1055 blocks,
# more than k_select_scan has threads
SIZES = [(1, 1, "A"), (5, 3, "B"), (67, 35, "A"), (67, 35, "B"), (300, 20, "B"), (600, 450, "A")]


@pytest.mark.parametrize("w,h,move", SIZES)
def test_hole_lists_match_the_reference(rt, gpu_scenes, w, h, move):
    """rt_accum_holes on the device's own counts after a real reprojection: ids, count and n_holes are fill_ref's for
    period 0, 1, 4 (every phase) and 5; a cap below the count cuts the list and still reports the full count; the four
    phases of period 4 partition the pixels with history."""
    base = gpu_scenes[NAME]
    _, _, view = _views(base, move)
    src, _ = _fill_src(rt, w, h)
    with src, rt.Accumulator(w, h) as dst:
        n_valid = dst.reproject_from(src, view, base, 6)
        K, _ = dst.counts()
        assert n_valid == int((K >= 2).sum())
        if (w, h) in ((67, 35), (600, 450)):
            assert 0 < n_valid < w * h  # both kinds of pixel
        for period, phase in ((0, 0), (1, 0), (4, 0), (4, 1), (4, 2), (4, 3), (5, 2)):
            want, count, n_holes = fr.holes(K, period, phase)
            ids, nh = dst.holes(period, phase)
            assert ids.dtype == np.uint32 and np.array_equal(ids, want) and nh == n_holes == w * h - n_valid
            cap = count // 2
            got, n, nh2 = _raw_holes(rt, dst, period, phase, cap)
            assert n == count and nh2 == n_holes and np.array_equal(got[:cap], want[:cap])
            assert (got[cap:] == 0xFFFFFFFF).all()  # nothing written past the cap
            _, n, nh2 = _raw_holes(rt, dst, period, phase, 0)
            assert n == count and nh2 == n_holes
        hole = (K < 2).reshape(-1)
        seen = np.zeros(w * h, dtype=np.int64)
        for phase in range(4):
            ids, _ = dst.holes(4, phase)
            assert hole[ids].sum() == hole.sum()  # every phase lists every hole
            seen[ids[~hole[ids]]] += 1
        assert (seen[~hole] == 1).all() and not seen[hole].any()


def _plane_scene(rt):
    """A diffuse floor under a light: every camera ray of a camera above it hits the floor."""
    objs = [dict(geom_kind=1, pos=[0.0, 0.0, 0.0], n=[0.0, 1.0, 0.0], brdf_kind=0, k=[0.6, 0.6, 0.6]),
            dict(geom_kind=0, pos=[30.0, 9.0, 0.0], r=1.0, brdf_kind=0, k=[0.0, 0.0, 0.0], emitted=[9.0, 9.0, 9.0])]
    return rt.Scene.from_desc([0.0, 5.0, 0.0], [0.0, -1.0, 0.0], objs)


def _synthetic_src(rt, w, h):
    src = rt.Accumulator(w, h)
    for m, n in zip(accum_ref.synthetic_passes(w, h, ns=(1, 2)), (1, 2)):
        src.add_sub(m, n)
    return src


def test_identical_views_leave_no_hole_and_a_src_turned_away_only_holes(rt, gpu_scenes):
    """Identical views of a scene whose every first hit is diffuse: n_holes = 0, and the fill launches nothing but the
    refresh. A src view turned away in the cornell box (every hit point lies behind the old camera): every pixel is a
    hole."""
    w, h = 40, 30
    floor = _plane_scene(rt)
    kw = dict(pos=(0.0, 5.0, 0.0), dir=(0.0, -1.0, 0.0))
    with _synthetic_src(rt, w, h) as src, rt.Accumulator(w, h) as dst:
        assert dst.reproject_from(src, floor.view(**kw), floor.view(**kw), 4) == w * h
        ids, n_holes = dst.holes()
        assert ids.size == 0 and n_holes == 0
        ids, n_holes = dst.holes(1, 0)
        assert np.array_equal(ids, np.arange(w * h)) and n_holes == 0
        base = gpu_scenes[NAME]
        v0 = rr.scene_view(scene_path(NAME))
        away = rr.view(v0["pos"], -v0["dir"])
        assert dst.reproject_from(src, base, base.view(**rr.as_kwargs(away)), 4) == 0
        ids, n_holes = dst.holes()
        assert np.array_equal(ids, np.arange(w * h)) and n_holes == w * h


# Fill -----------------------------------------------------------------------------------------------------------

FILLS = [(67, 35, 4, "A"), (67, 35, 36, "B"), (96, 72, 4, "B"), (96, 72, 36, "A")]


@pytest.mark.parametrize("w,h,spp,move", FILLS)
def test_fill_matches_the_reference_and_the_two_full_passes(rt, gpu_scenes, oracle_scenes, w, h, spp, move):
    """period 0. The resolved sub and var and both count maps equal fill_ref's bit for bit (the device's own rt_render
    frames are the passes); on every hole they equal, bit for bit, a second accumulator taken through the current flow
    (the same reprojection, then two rt_accum_add calls with the same seeds); pixels with history keep the
    reprojection's counts and means."""
    base = gpu_scenes[NAME]
    _, _, view = _views(base, move)
    c, keep = _classify(oracle_scenes, base, w, h, move)
    s1, s2 = rt.pass_seed(SEED, 40), rt.pass_seed(SEED, 41)
    frames = _frames(rt, view, w, h, spp, (s1, s2))
    n = spp // 4
    src, src_ref = _fill_src(rt, w, h)
    with src, rt.Accumulator(w, h) as dst, rt.Accumulator(w, h) as full:
        seed_state = rr.reproject(src_ref.S, src_ref.Q, src_ref.K, src_ref.N, c, 6)[:4]
        ref, ref_seeded = fr.Accum(w, h), fr.Accum(w, h)
        ref.seed(*seed_state)
        ref_seeded.seed(*seed_state)
        dst.reproject_from(src, view, base, 6)
        full.reproject_from(src, view, base, 6)
        K0, N0 = dst.counts()
        hole = K0 < 2
        assert 0 < hole.sum() < w * h and np.array_equal(hole[keep], (ref.K < 2)[keep])
        st = dst.fill(view, spp, s1, s2)
        lens = ref.fill(_gather(frames), n)
        print(f"{w} x {h} move {move} spp {spp}: lists {st['fill']} (reference {lens}), {int((~keep).sum())} pixels "
              "left out")
        assert not st["cancelled"] and st["fill"] == (int(hole.sum()),) * 2
        assert abs(st["fill"][0] - lens[0]) <= (~keep).sum()
        assert st["samples"] == sum(st["fill"]) * 4 * n and st["vertices"] > 0
        assert dst.info()["passes"] == 0 and dst.info()["n"] == 0
        sub, var, _ = dst.resolve(want_var=True, want_rgb=False)
        K1, N1 = dst.counts()
        assert _same(sub[keep], ref.sub()[keep]) and _same(var[keep], ref.var()[keep])
        assert np.array_equal(K1[keep], ref.K[keep]) and np.array_equal(N1[keep], ref.N[keep])
        # the current flow on the same seeded state
        for s in (s1, s2):
            full.add(view, spp, s)
        sub_f, var_f, _ = full.resolve(want_var=True, want_rgb=False)
        Kf, Nf = full.counts()
        assert _same(sub[hole], sub_f[hole]) and _same(var[hole], var_f[hole])
        assert np.array_equal(K1[hole], Kf[hole]) and np.array_equal(N1[hole], Nf[hole])
        assert (K1[hole] == 2).all() and (N1[hole] == 2 * n).all()
        # pixels with history are untouched
        assert np.array_equal(K1[~hole], K0[~hole]) and np.array_equal(N1[~hole], N0[~hole])
        m = ~hole & keep
        with np.errstate(invalid="ignore"):  # (0 / 0 on the holes, which m leaves out)
            assert _same(sub[m], ref_seeded.sub()[m])
        assert not _same(sub[~hole], sub_f[~hole])  # (the full passes did change them)


def test_refresh_adds_one_pass_to_the_listed_pixels(rt, gpu_scenes, oracle_scenes):
    """period 4, phase 1, with MIS: a listed pixel with history gains exactly (1, n), a hole (2, 2 n), the others
    nothing; the sums are fill_ref's bit for bit."""
    w, h, spp, move = 67, 35, 8, "A"
    base = gpu_scenes[NAME]
    _, _, view = _views(base, move)
    c, keep = _classify(oracle_scenes, base, w, h, move)
    s1, s2 = rt.pass_seed(SEED, 50), rt.pass_seed(SEED, 51)
    frames = _frames(rt, view, w, h, spp, (s1, s2), mis=True)
    src, src_ref = _fill_src(rt, w, h)
    with src, rt.Accumulator(w, h) as dst:
        ref = fr.Accum(w, h)
        ref.seed(*rr.reproject(src_ref.S, src_ref.Q, src_ref.K, src_ref.N, c, 6)[:4])
        dst.reproject_from(src, view, base, 6)
        K0, N0 = dst.counts()
        hole, listed = K0 < 2, fr.hole_mask(K0, 4, 1)
        st = dst.fill(view, spp, s1, s2, period=4, phase=1, mis=True)
        ref.fill(_gather(frames), 2, 4, 1)
        assert st["fill"] == (int(listed.sum()), int(hole.sum())) and st["fill"][0] > st["fill"][1] > 0
        K1, N1 = dst.counts()
        assert np.array_equal(K1.astype(np.int64) - K0, np.where(hole, 2, np.where(listed, 1, 0)))
        assert np.array_equal(N1.astype(np.int64) - N0, np.where(hole, 4, np.where(listed, 2, 0)))
        sub, var, _ = dst.resolve(want_var=True, want_rgb=False)
        assert _same(sub[keep], ref.sub()[keep]) and _same(var[keep], ref.var()[keep])


# State ----------------------------------------------------------------------------------------------------------

def test_covered_state(rt, gpu_scenes):
    """resolve raises before the fill and works after it; select and add_pixels work on a covered accumulator whose
    info() reports no pass; a full-frame pass keeps the state; reset and a new reprojection clear it."""
    w, h = 67, 35
    base = gpu_scenes[NAME]
    _, _, view = _views(base, "A")
    src, _ = _fill_src(rt, w, h)
    with src, rt.Accumulator(w, h) as dst:
        with pytest.raises(rt.RtError):
            dst.holes()  # not seeded
        with pytest.raises(rt.RtError):
            dst.fill(view, 8, 1, 2)
        dst.reproject_from(src, view, base, 6)
        for call in (dst.resolve, lambda: dst.select(0.0), lambda: dst.add_pixels(view, [0, 1], 8, 3)):
            with pytest.raises(rt.RtError):
                call()
        dst.fill(view, 8, rt.pass_seed(SEED, 60), rt.pass_seed(SEED, 61))
        assert dst.info()["passes"] == 0 and dst.info()["n"] == 0
        sub, var, rgb = dst.resolve(want_var=True)
        K, N = dst.counts()
        assert (K >= 2).all() and np.isfinite(sub).all() and np.isfinite(var).all() and rgb.any()
        # the selection is adapt_ref's on the device's own resolve
        ids, total = dst.select(0.0, 0.0, 5)
        want = np.flatnonzero(dref.select_mask(var, sub, N, 0.0, 0.0, 5)).astype(np.uint32)
        assert total == ids.size > 0 and np.array_equal(ids, want) and (N.reshape(-1)[ids] < 5).all()
        dst.add_pixels(view, ids, 8, rt.pass_seed(SEED, 62))
        K2, N2 = dst.counts()
        gain = np.zeros(w * h, dtype=np.int64)
        gain[ids] = 1
        assert np.array_equal(K2.reshape(-1) - K.reshape(-1), gain) and np.array_equal(N2.reshape(-1) - N.reshape(-1), 2 * gain)
        # a second fill of a covered accumulator lists nothing at period 0
        assert dst.fill(view, 8, 4, 5)["fill"] == (0, 0)
        # a full-frame merge behaves as on a seeded accumulator, and the state stays
        dst.add(view, 4, rt.pass_seed(SEED, 63))
        assert dst.info()["passes"] == 1
        K3, _ = dst.counts()
        assert np.array_equal(K3, K2 + 1)
        dst.resolve(want_var=True)
        # a new reprojection into it clears the state, and so does reset
        dst.reproject_from(src, view, base, 6)
        with pytest.raises(rt.RtError):
            dst.resolve()
        dst.fill(view, 4, 7, 8)
        dst.resolve(want_var=True)
        dst.reset()
        with pytest.raises(rt.RtError):
            dst.resolve()
        with pytest.raises(rt.RtError):
            dst.holes()


def test_chain_of_three_views_reprojects_from_covered_accumulators(rt, gpu_scenes, oracle_scenes):
    """view 0 -> view 1 (move A) -> view 2 (half of move A again): the second reprojection reads a covered accumulator
    that never saw a full-frame pass. Counts, sub and var match fill_ref's chain bit for bit (left out: pixels whose
    queries disagree with the oracle's in either step, and those that fetch from one)."""
    w, h, spp = 67, 35, 8
    base = gpu_scenes[NAME]
    path = scene_path(NAME)
    v0, v1, view1 = _views(base, "A")
    v2 = rr.view(v1["pos"] + np.array([7.0, 3.0, -20.0]), v1["dir"] + np.array([-0.05, -0.025, 0.0]))
    view2 = base.view(**rr.as_kwargs(v2))
    c1, keep1 = _classify(oracle_scenes, base, w, h, "A")
    c2 = rr.classify(oracle_scenes[NAME], rr.brdf_kinds(path), v2, v1, w, h)
    out2 = _disagreeing_pixels(base, c2, v1["pos"], w, h)
    keep2 = ~(out2 | (~keep1).reshape(-1)[c2["q"]].any(-1))
    assert (~keep2).sum() <= 0.005 * w * h
    seeds = [rt.pass_seed(SEED, 70 + k) for k in range(4)]
    f1 = _frames(rt, view1, w, h, spp, seeds[:2])
    f2 = _frames(rt, view2, w, h, spp, seeds[2:])
    src, src_ref = _fill_src(rt, w, h)
    with src, rt.Accumulator(w, h) as a1, rt.Accumulator(w, h) as a2:
        r1, r2 = fr.Accum(w, h), fr.Accum(w, h)
        r1.seed(*rr.reproject(src_ref.S, src_ref.Q, src_ref.K, src_ref.N, c1, 6)[:4])
        r1.fill(_gather(f1), 2, 2, 1)
        assert r1.may("reproject_src") and r1.passes == 0
        r2.seed(*rr.reproject(r1.S, r1.Q, r1.K, r1.N, c2, 6)[:4])
        r2.fill(_gather(f2), 2, 2, 0)
        a1.reproject_from(src, view1, base, 6)
        a1.fill(view1, spp, seeds[0], seeds[1], period=2, phase=1)
        n_valid = a2.reproject_from(a1, view2, view1, 6)
        assert 0 < n_valid < w * h and a1.info()["passes"] == 0
        a2.fill(view2, spp, seeds[2], seeds[3], period=2, phase=0)
        sub, var, _ = a2.resolve(want_var=True, want_rgb=False)
        K, N = a2.counts()
        assert np.array_equal(K[keep2], r2.K[keep2]) and np.array_equal(N[keep2], r2.N[keep2])
        assert _same(sub[keep2], r2.sub()[keep2]) and _same(var[keep2], r2.var()[keep2])
        assert (N > 4).any()  # history arrived through the chain


# Edge cases -----------------------------------------------------------------------------------------------------

def test_no_holes_all_holes_and_cancel(rt, gpu_scenes):
    """No holes: the fill launches nothing (fill = (0, 0)), and the accumulator is covered. All holes: the filled frame
    equals two merged rt_render passes everywhere. A cancel word raised before the call: RT_CANCELLED, nothing merged,
    not covered; a second fill completes it."""
    w, h, spp = 40, 30, 8
    floor = _plane_scene(rt)
    kw = dict(pos=(0.0, 5.0, 0.0), dir=(0.0, -1.0, 0.0))
    base = gpu_scenes[NAME]
    v0 = rr.scene_view(scene_path(NAME))
    away = base.view(**rr.as_kwargs(rr.view(v0["pos"], -v0["dir"])))
    s1, s2 = rt.pass_seed(SEED, 80), rt.pass_seed(SEED, 81)
    with _synthetic_src(rt, w, h) as src, rt.Accumulator(w, h) as dst, rt.Accumulator(w, h) as two:
        fv = floor.view(**kw)
        dst.reproject_from(src, fv, fv, 4)
        K0, N0 = dst.counts()
        st = dst.fill(fv, spp, s1, s2)
        assert st["fill"] == (0, 0) and st["samples"] == 0 and not st["cancelled"]
        K1, N1 = dst.counts()
        assert np.array_equal(K0, K1) and np.array_equal(N0, N1) and (K1 >= 2).all()
        sub, var, _ = dst.resolve(want_var=True, want_rgb=False)  # covered without a single new sample
        assert np.allclose(sub, src.resolve()[0], rtol=1e-15, atol=0)
        # all holes
        dst.reproject_from(src, base, away, 4)
        cancel = ctypes.c_int32(1)
        st = dst.fill(base, spp, s1, s2, cancel=cancel)
        assert st["cancelled"] and st["fill"] == (w * h, 0)
        assert not dst.counts()[0].any() and not dst.counts()[1].any()
        with pytest.raises(rt.RtError):
            dst.resolve()
        st = dst.fill(base, spp, s1, s2)
        assert not st["cancelled"] and st["fill"] == (w * h, w * h) and st["samples"] == 2 * w * h * spp
        for m in _frames(rt, base, w, h, spp, (s1, s2)):
            two.add_sub(m, spp // 4)
        got, want = dst.resolve(want_var=True), two.resolve(want_var=True)
        assert all(_same(a, b) for a, b in zip(got, want))
        K, N = dst.counts()
        assert (K == 2).all() and (N == 2 * (spp // 4)).all()


# End to end -----------------------------------------------------------------------------------------------------

# tools/fill_probe.py quality (CPU: oracle + reproject_ref + fill_ref), cornell_box 96 x 72, move A, src 16 passes of
# 16 spp, max_n 64: all-pixel linear RMSE against a 1024-spp frame after the two full 4-spp passes and after the fill
# at FILL_DEFAULTS = (16 spp, refresh 4; phase 1) (profiles/fill_quality.log): 8.00 and 6.62 camera
# samples per pixel. Their ratio is 0.935; the test asserts its geometric mean with 1, 0.967.
CPU_RMSE_PARENT, CPU_RMSE_FILL = 0.0552, 0.0516


def test_fill_flow_after_a_move(rt, gpu_scenes, tmp_path):
    """cornell 96 x 72, move A, the set-up of test_history_lowers_the_error_after_a_move: the second view through the
    fill at rt.FILL_DEFAULTS traces fewer camera samples than through two full 4-spp passes, and its all-pixel RMSE
    against a 1024-spp frame, relative to the parent flow's, stays below the geometric mean of the ratio measured on the
    CPU and 1."""
    w, h = 96, 72
    path, base = scene_path(NAME), gpu_scenes[NAME]
    v1 = rr.scene_view(path, rr.MOVE_A)
    moved, assets = rr.moved_toml(path, v1, tmp_path)
    view = base.view(**rr.as_kwargs(v1))
    ref = rt.render(rt.Scene.from_toml(moved, assets), w, h, 1024, 0xC0FFEE, megakernel=True, want_sub=True)[1]
    f, r = rt.FILL_DEFAULTS["fill_spp"], rt.FILL_DEFAULTS["refresh"]
    assert (f, r) == (16, 4)  # what the CPU figures above were measured for
    s1, s2 = rt.pass_seed(SEED, 16), rt.pass_seed(SEED, 17)
    with rt.Accumulator(w, h) as src, rt.Accumulator(w, h) as parent, rt.Accumulator(w, h) as fill:
        for k in range(16):
            src.add(base, 16, rt.pass_seed(SEED, k))
        parent.reproject_from(src, view, base, 64)
        fill.reproject_from(src, view, base, 64)
        samples_parent = sum(parent.add(view, 4, s)["samples"] for s in (s1, s2))
        samples_fill = fill.fill(view, f, s1, s2, period=r, phase=1 % r if r else 0)["samples"]
        sub_p, sub_f = parent.resolve()[0], fill.resolve()[0]
    rmse = lambda sub: float(np.sqrt(((rr.pixel_colour(sub) - rr.pixel_colour(ref)) ** 2).mean()))
    ratio, cpu = rmse(sub_f) / rmse(sub_p), CPU_RMSE_FILL / CPU_RMSE_PARENT
    print(f"samples {samples_fill} against {samples_parent}; RMSE fill {rmse(sub_f):.4f}, parent {rmse(sub_p):.4f}, "
          f"ratio {ratio:.4f} (CPU {cpu:.4f})")
    assert samples_fill < samples_parent == 2 * 4 * w * h
    assert cpu < 1.0 and ratio <= (cpu * 1.0) ** 0.5


def test_render_interactive_with_the_fill(rt, gpu_scenes):
    """Two views, cornell 96 x 72, move A. fill_spp = 0 is the flow of DESIGN.md §14 byte for byte (a hand-written loop
    of it); with rt.FILL_DEFAULTS the first view is unchanged, the second traces fewer camera samples and is the frame a
    hand-written reproject / fill / resolve / denoise_var gives."""
    w, h = 96, 72
    base = gpu_scenes[NAME]
    v0, v1 = rr.scene_view(scene_path(NAME)), rr.scene_view(scene_path(NAME), rr.MOVE_A)
    views = [rr.as_kwargs(v0), rr.as_kwargs(v1)]
    f, r = rt.FILL_DEFAULTS["fill_spp"], rt.FILL_DEFAULTS["refresh"]
    today = list(rt.render_interactive(base, views, w, h, first=8, max_n=64, seed=SEED))
    off = list(rt.render_interactive(base, views, w, h, first=8, max_n=64, seed=SEED, fill_spp=0, refresh=0))
    on = list(rt.render_interactive(base, views, w, h, first=8, max_n=64, seed=SEED, **rt.FILL_DEFAULTS))
    for a, b in zip(today, off):
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    assert np.array_equal(on[0][0], today[0][0]) and on[0][1:] == today[0][1:] == (0.0, 2 * 8 * w * h)
    assert on[1][1] == today[1][1] > 0.85 and today[1][2] == 2 * 8 * w * h
    assert on[1][2] < today[1][2] and not np.array_equal(on[1][0], today[1][0])

    def by_hand(fill):
        sv0, sv1 = base.view(**views[0]), base.view(**views[1])
        with rt.Accumulator(w, h) as a0, rt.Accumulator(w, h) as a1:
            for k in range(2):
                a0.add(sv0, 8, rt.pass_seed(SEED, k))
            a1.reproject_from(a0, sv1, sv0, 64)
            if fill:
                st = a1.fill(sv1, f, rt.pass_seed(SEED, 2), rt.pass_seed(SEED, 3), period=r, phase=1 % r if r else 0)
                samples = sum(st["fill"]) * f
            else:
                for k in (2, 3):
                    a1.add(sv1, 8, rt.pass_seed(SEED, k))
                samples = 2 * 8 * w * h
            sub, var, _ = a1.resolve(want_var=True, want_rgb=False)
            return rt.denoise_var(sub, rt.render_features(sv1, w, h), var), samples

    rgb, samples = by_hand(False)
    assert np.array_equal(rgb, today[1][0]) and samples == today[1][2]
    rgb, samples = by_hand(True)
    assert np.array_equal(rgb, on[1][0]) and samples == on[1][2]


def test_interactive_job_reads_the_fill_from_the_environment(rt, gpu_scenes, monkeypatch):
    """server.InteractiveJob with RT_REPROJECT_FILL=16,4: two requests with two cameras send the two frames
    render_interactive(fill_spp=16, refresh=4) yields, the second of which is not the frame of the flow without it."""
    from rt_amd import server

    w, h = 60, 45
    base = gpu_scenes[NAME]
    cams = [dict(pos=(50.0, 52.0, 295.6), dir=(0.0, -0.042612, -1.0)), dict(pos=(64.0, 58.0, 255.6), dir=(-0.1, -0.092612, -1.0))]
    sent = []

    async def send(msg):
        sent.append(msg)

    monkeypatch.setenv("RT_REPROJECT_FILL", "16,4")
    job = server.InteractiveJob(send, max_n=16, first=8)
    assert (job.fill_spp, job.refresh) == (16, 4)

    async def go():
        for cam in cams:
            assert await job.run(base.view(**cam), w, h, 16, SEED) is False

    asyncio.run(go())
    assert len(sent) == 2 * h and not job.running()
    frames = np.zeros((2, h, w, 3), dtype=np.uint8)
    for i, m in enumerate(sent):
        _, n, x, y = struct.unpack("<BBHH", m[:6])
        frames[i // h, y, x:x + n] = np.frombuffer(m[6:], dtype=np.uint8).reshape(n, 3)
    want = list(rt.render_interactive(base, cams, w, h, first=8, max_n=16, seed=SEED, fill_spp=16, refresh=4))
    plain = list(rt.render_interactive(base, cams, w, h, first=8, max_n=16, seed=SEED))
    assert np.array_equal(frames[0], want[0][0]) and np.array_equal(frames[1], want[1][0])
    assert np.array_equal(frames[0], plain[0][0]) and not np.array_equal(frames[1], plain[1][0])
    assert want[1][2] < plain[1][2]
