"""Accumulator reprojection on the device (rt_accum_reproject, k_reproject_f64) against
tests/reproject_ref.py: counts, n_valid and the resolved frame bit for bit; the rejection classes the shipped scenes
lack; the seeded state; identity views; render_interactive and the server's camera message."""
import asyncio
import json
import struct

import numpy as np
import pytest

import accum_ref
import reproject_ref as rr
from conftest import scene_path

pytestmark = pytest.mark.gpu

SEED = 0x5EED


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _disagreeing_pixels(scene, c, src_pos, width, height):
    """Pixels the comparison may leave out: one of their four subpixels' reference rays or shadow segments gets
    another answer from the device's own rt_trace_rays / rt_diag_visible than from the oracle (hit object, or any bit
    of the hit position or normal; visibility)."""
    o, d = c["rays"]
    ids_o, x_o, n_o = c["hits"]
    _, ids, pos, nrm = scene.trace_ray(o, d)
    hit = ids_o >= 0
    bad = ids != ids_o
    bad |= hit & ((pos.view(np.uint64) != x_o.view(np.uint64)).any(1) | (nrm.view(np.uint64) != n_o.view(np.uint64)).any(1))
    if c["asked"].size:
        vis, _ = scene.diag_visible(c["seg"], np.broadcast_to(src_pos, c["seg"].shape).copy())
        bad[c["asked"][vis != c["vis"]]] = True
    return bad.reshape(height, width, 4).any(-1)


def _fill_src(rt, w, h):
    """An accumulator and its restatement after three synthetic passes (n = 1, 2, 5) and one sparse list (n = 3):
    S, Q and the per-pixel counts are known exactly."""
    acc, ref = rt.Accumulator(w, h), rr.Accum(w, h)
    for m, n in zip(accum_ref.synthetic_passes(w, h), (1, 2, 5)):
        acc.add_sub(m, n)
        ref.add_sub(m, n)
    rng = np.random.default_rng(w * 1000 + h)
    ids = np.sort(rng.choice(w * h, size=w * h // 3, replace=False)).astype(np.uint32)
    m = rng.uniform(-0.2, 1.6, size=(ids.size, 4, 3))
    acc.add_sub_pixels(ids, m, 3)
    ref.add_sub_pixels(ids, m, 3)
    return acc, ref


PARITY = [("cornell_box", "A", 96, 72), ("cornell_box", "B", 96, 72), ("flying_unicorn", "A", 64, 48),
          ("cubes", "A", 64, 48)]


@pytest.mark.parametrize("name,move,w,h", PARITY)
def test_reprojection_matches_the_reference(rt, gpu_scenes, oracle_scenes, name, move, w, h):
    """max_n = 6: rt_accum_counts and n_valid are the reference's; after two more synthetic full-frame passes
    rt_accum_resolve's sub and var are the reference's bit for bit. A pixel is left out only where the device's own
    query of the reference's rays / segments disagrees with the oracle (_disagreeing_pixels), at most 0.1 % of the
    pixels; reproject_ref alone leaves none out."""
    path = scene_path(name)
    base = gpu_scenes[name]
    v0, v1 = rr.scene_view(path), rr.scene_view(path, rr.MOVE_A if move == "A" else rr.MOVE_B)
    dst_view = base.view(**rr.as_kwargs(v1))
    c = rr.classify(oracle_scenes[name], rr.brdf_kinds(path), v1, v0, w, h)
    src, src_ref = _fill_src(rt, w, h)
    with src, rt.Accumulator(w, h) as dst:
        want = rr.reproject(src_ref.S, src_ref.Q, src_ref.K, src_ref.N, c, 6)
        n_valid = dst.reproject_from(src, dst_view, base, 6)  # the base itself is the src view
        assert dst.info()["passes"] == 0 and dst.info()["n"] == 0
        k, n = dst.counts()
        out = _disagreeing_pixels(base, c, v0["pos"], w, h)
        keep = ~out
        print(f"{name} {move}: n_valid {n_valid} (reference {want[4]}), {int(out.sum())} pixels left out, "
              f"classes {rr.class_counts(c)}")
        assert out.sum() <= 0.001 * w * h
        assert abs(n_valid - want[4]) <= out.sum() and 0 < want[4] < w * h
        assert np.array_equal(k[keep], want[2][keep]) and np.array_equal(n[keep], want[3][keep])
        assert n_valid == int((n > 0).sum()) and np.array_equal(n > 0, k >= 2)
        assert (n <= 6).all() and n.max() == 6
        dst_ref = rr.Accum(w, h)
        dst_ref.seed(*want[:4])
        for m, nn in zip(accum_ref.synthetic_passes(w, h, ns=(2, 4), seed=7), (2, 4)):
            dst.add_sub(m, nn)
            dst_ref.add_sub(m, nn)
        assert dst.info()["passes"] == 2 and dst.info()["n"] == 6
        sub, var, _ = dst.resolve(want_var=True, want_rgb=False)
        assert _same(sub[keep], dst_ref.sub()[keep]) and _same(var[keep], dst_ref.var()[keep])
        k2, n2 = dst.counts()
        assert np.array_equal(k2, k + 2) and np.array_equal(n2, n + 6)
        # src was only read
        ks, ns = src.counts()
        assert np.array_equal(ks, src_ref.K) and np.array_equal(ns, src_ref.N)
        assert _same(src.resolve()[0], src_ref.sub())


def _small_scene(rt, oracle, tmp_path, cam_pos, cam_dir, objs):
    p = tmp_path / "small.toml"
    p.write_text(rr.toml_of(cam_pos, cam_dir, objs))
    kinds = np.array([o.get("brdf_kind", 0) for o in objs])
    return rt.Scene.from_desc(cam_pos, cam_dir, objs), oracle.OracleScene(str(p)), kinds


def _reproject_small(rt, scene, dst_kw, src_kw, w, h, max_n=4):
    with rt.Accumulator(w, h) as src, rt.Accumulator(w, h) as dst:
        for m, n in zip(accum_ref.synthetic_passes(w, h, ns=(1, 2)), (1, 2)):
            src.add_sub(m, n)
        n_valid = dst.reproject_from(src, scene.view(**dst_kw), scene.view(**src_kw), max_n)
        return n_valid, dst.counts()


def test_back_side_is_rejected_by_the_same_side_test(rt, oracle, tmp_path):
    """A diffuse plane with the two cameras on opposite sides: every dst subpixel's hit projects into the src frame in
    front of the src camera, and the same-side test alone rejects it; with src on dst's side every pixel is valid."""
    w, h = 40, 30
    objs = [dict(geom_kind=1, pos=[0.0, 0.0, 0.0], n=[0.0, 1.0, 0.0], brdf_kind=0, k=[0.6, 0.6, 0.6]),
            dict(geom_kind=0, pos=[30.0, 9.0, 0.0], r=1.0, brdf_kind=0, k=[0.0, 0.0, 0.0], emitted=[9.0, 9.0, 9.0])]
    scene, osc, kinds = _small_scene(rt, oracle, tmp_path, [0.0, 5.0, 0.0], [0.0, -1.0, 0.0], objs)
    dst = rr.view([0.0, -3.0, 0.0], [0.0, 1.0, 0.0])
    above, below = rr.view([0.0, 5.0, 0.0], [0.0, -1.0, 0.0]), rr.view([0.5, -5.0, 0.0], [0.0, 1.0, 0.0])
    c = rr.classify(osc, kinds, dst, above, w, h)
    assert rr.class_counts(c)["back_side"] == w * h * 4  # the only reason, for every subpixel
    n_valid, (k, n) = _reproject_small(rt, scene, rr.as_kwargs(dst), rr.as_kwargs(above), w, h)
    assert n_valid == 0 and not k.any() and not n.any()
    c = rr.classify(osc, kinds, dst, below, w, h)
    assert c["ok"].all()
    n_valid, (k, n) = _reproject_small(rt, scene, rr.as_kwargs(dst), rr.as_kwargs(below), w, h)
    assert n_valid == w * h and (k == 2).all() and (n == 3).all()


def test_points_behind_the_old_camera_and_misses_are_rejected(rt, gpu_scenes, oracle, oracle_scenes, tmp_path):
    """The dst view turned 180 degrees in the cornell box: every ray hits a wall, the floor or the ceiling behind the
    src camera (the planes are unbounded), so n_valid = 0 and "behind" is the only reason. A sphere in empty space: the
    rays beside it miss, and the device's counts are the reference's."""
    w, h = 48, 36
    path = scene_path("cornell_box")
    v0 = rr.scene_view(path)
    back = rr.view(v0["pos"], -v0["dir"])
    c = rr.classify(oracle_scenes["cornell_box"], rr.brdf_kinds(path), back, v0, w, h)
    counts = rr.class_counts(c)
    assert counts["behind"] == w * h * 4
    n_valid, (k, n) = _reproject_small(rt, gpu_scenes["cornell_box"], rr.as_kwargs(back), rr.as_kwargs(v0), w, h)
    assert n_valid == 0 and not k.any() and not n.any()

    objs = [dict(geom_kind=0, pos=[0.0, 0.0, 0.0], r=2.0, brdf_kind=0, k=[0.7, 0.5, 0.3]),
            dict(geom_kind=0, pos=[0.0, 40.0, 0.0], r=1.0, brdf_kind=0, k=[0.0, 0.0, 0.0], emitted=[9.0, 9.0, 9.0])]
    scene, osc, kinds = _small_scene(rt, oracle, tmp_path, [0.0, 0.0, 10.0], [0.0, 0.0, -1.0], objs)
    src, dst = rr.view([0.0, 0.0, 10.0], [0.0, 0.0, -1.0]), rr.view([1.0, 0.5, 9.0], [-0.1, -0.05, -1.0])
    c = rr.classify(osc, kinds, dst, src, w, h)
    counts = rr.class_counts(c)
    valid = c["ok"].all(-1)
    assert counts["miss"] > w * h and 0 < valid.sum() < w * h and counts["non_diffuse"] == 0
    n_valid, (k, n) = _reproject_small(rt, scene, rr.as_kwargs(dst), rr.as_kwargs(src), w, h)
    out = _disagreeing_pixels(scene, c, src["pos"], w, h)
    assert out.sum() == 0
    assert n_valid == valid.sum() and np.array_equal(n > 0, valid) and np.array_equal(k[valid], np.full(valid.sum(), 2))


def test_seeded_accumulator_merges_and_reset_forgets(rt, gpu_scenes, oracle_scenes):
    """rt_accum_add after a reprojection adds to the seeded sums; after rt_accum_reset the accumulator is new."""
    w, h, name = 48, 36, "cornell_box"
    path, base = scene_path(name), gpu_scenes[name]
    v0, v1 = rr.scene_view(path), rr.scene_view(path, rr.MOVE_A)
    dst_view = base.view(**rr.as_kwargs(v1))
    c = rr.classify(oracle_scenes[name], rr.brdf_kinds(path), v1, v0, w, h)
    src, src_ref = _fill_src(rt, w, h)
    passes = [rt.render(dst_view, w, h, 8, rr_seed, megakernel=True, want_sub=True)[1] for rr_seed in (11, 12)]
    with src, rt.Accumulator(w, h) as dst:
        dst.add_sub(passes[0], 9)  # whatever dst held is dropped by the reprojection
        dst.reproject_from(src, dst_view, base, 6)
        keep = ~_disagreeing_pixels(base, c, v0["pos"], w, h)
        with pytest.raises(rt.RtError):
            dst.resolve()  # K = 0: no full-frame pass since the reprojection
        ref = rr.Accum(w, h)
        ref.seed(*rr.reproject(src_ref.S, src_ref.Q, src_ref.K, src_ref.N, c, 6)[:4])
        for seed, m in zip((11, 12), passes):
            dst.add(dst_view, 8, seed)
            ref.add_sub(m, 2)
        sub, var, _ = dst.resolve(want_var=True, want_rgb=False)
        assert _same(sub[keep], ref.sub()[keep]) and _same(var[keep], ref.var()[keep])
        assert not _same(sub, passes[0])  # history is in there
        # sparse passes and the selection work on a seeded accumulator
        # the selection and a sparse pass work on a seeded accumulator: with max_n = 5 only the pixels without
        # history (4 samples per subpixel; the others hold 10) can be active
        ids, total = dst.select(0.0, 0.0, 5)
        n_before = dst.counts()[1].reshape(-1)
        assert total == ids.size > 0 and (n_before[ids] == 4).all() and ids.size <= (n_before == 4).sum()
        dst.add_pixels(dst_view, ids, 8, 13)
        n_after = dst.counts()[1].reshape(-1)
        assert (n_after[ids] == 6).all() and n_after.sum() == n_before.sum() + 2 * ids.size
        dst.reset()
        assert dst.info()["passes"] == 0
        dst.add(dst_view, 8, 11)
        k, n = dst.counts()
        assert (k == 1).all() and (n == 2).all() and _same(dst.resolve()[0], passes[0])


def test_identical_views_keep_the_history(rt, gpu_scenes, oracle_scenes):
    """Real passes (cornell 64 x 48, 4 x 8 spp), dst view = src view, a huge max_n: every valid pixel keeps (K, N),
    and after two more passes sub is the reference's: S_dst = N (S_src / N) with S_src / N the resolve of src."""
    w, h, name = 64, 48, "cornell_box"
    path, base = scene_path(name), gpu_scenes[name]
    v0 = rr.scene_view(path)
    c = rr.classify(oracle_scenes[name], rr.brdf_kinds(path), v0, v0, w, h)
    valid = c["ok"].all(-1)
    more = [rt.render(base, w, h, 8, s, megakernel=True, want_sub=True)[1] for s in (21, 22)]
    with rt.Accumulator(w, h) as src, rt.Accumulator(w, h) as dst:
        for k in range(4):
            src.add(base, 8, rt.pass_seed(SEED, k))
        m_src = src.resolve()[0]
        n_valid = dst.reproject_from(src, base.view(**rr.as_kwargs(v0)), base, 1 << 30)
        out = _disagreeing_pixels(base, c, v0["pos"], w, h)
        assert out.sum() <= 0.001 * w * h and abs(n_valid - valid.sum()) <= out.sum()
        keep = ~out
        k, n = dst.counts()
        assert (k[valid & keep] == 4).all() and (n[valid & keep] == 8).all()
        assert not k[~valid & keep].any() and not n[~valid & keep].any()
        ref = rr.Accum(w, h)
        S = np.where(valid[..., None, None], 8.0 * m_src, 0.0)
        ref.seed(S, S, np.where(valid, 4, 0), np.where(valid, 8, 0))  # (Q is not compared)
        for m in more:
            dst.add_sub(m, 2)
            ref.add_sub(m, 2)
        assert _same(dst.resolve()[0][keep], ref.sub()[keep])


def test_history_lowers_the_error_after_a_move(rt, gpu_scenes, tmp_path):
    """cornell 96 x 72: src holds 16 passes of 16 spp, move A, max_n = 64, then two passes of 4 spp, with the history
    and from an empty accumulator; linear RMSE of the pixel colour against a 1024-spp rt_render of the scene loaded
    from the A-camera TOML (the code path that existed before views).
    Measured RMSE ratio history / empty, on the CPU (oracle renders + reproject_ref, the same seeds): 0.525 over all
    pixels (0.0552 / 0.1050), 0.458 over the valid ones (0.0484 / 0.1056). On the MI355X: 0.525 and 0.458 again (equal
    to 12 digits: the same seeds and the same valid set), bias -0.000164.
    The thresholds are the geometric means of the CPU-measured ratios and 1: 0.725 and 0.677.
    Bias check: the mean signed difference of the reprojected means from the reference on valid pixels, before any
    new pass, was -0.00016 on the CPU (their RMSE 0.050: a 256-spp frame's own noise, magnified because move A goes
    closer, so a dst pixel's four subpixels often fetch the same src subpixel). It must stay within three standard
    errors of a mean over the 6,266 valid pixels of differences that scatter by 0.050: 3 x 0.050 / sqrt(6266) = 0.002
    (the channels of a pixel counted as one observation)."""
    w, h, name = 96, 72, "cornell_box"
    path, base = scene_path(name), gpu_scenes[name]
    v1 = rr.scene_view(path, rr.MOVE_A)
    moved, assets = rr.moved_toml(path, v1, tmp_path)
    loaded = rt.Scene.from_toml(moved, assets)
    view = base.view(**rr.as_kwargs(v1))
    ref = rt.render(loaded, w, h, 1024, 0xC0FFEE, megakernel=True, want_sub=True)[1]
    with rt.Accumulator(w, h) as src, rt.Accumulator(w, h) as hist, rt.Accumulator(w, h) as empty:
        for k in range(16):
            src.add(base, 16, rt.pass_seed(SEED, k))
        n_valid = hist.reproject_from(src, view, base, 64)
        k_seed, n_seed = hist.counts()
        valid = n_seed > 0
        assert n_valid == valid.sum() and (n_seed[valid] == 64).all() and (k_seed[valid] == 16).all()
        for k in (16, 17):
            hist.add(view, 4, rt.pass_seed(SEED, k))
            empty.add(view, 4, rt.pass_seed(SEED, k))
        sub_hist, sub_empty = hist.resolve()[0], empty.resolve()[0]
    q = rr.quality_figures(sub_hist, sub_empty, ref, valid)
    # the reprojected means alone: S_hist = S_seed + 1 m_16 + 1 m_17 and S_empty = m_16 + m_17, N_seed = 64
    m_seed = (sub_hist * 66.0 - sub_empty * 2.0) / 64.0
    bias = float((rr.pixel_colour(m_seed) - rr.pixel_colour(ref))[valid].mean())
    print(f"quality: {q}, valid share {valid.mean():.4f}, bias of the reprojected means {bias:+.6f}")
    assert 0.85 < valid.mean() < 0.95
    assert q["ratio_all"] <= 0.725 and q["ratio_valid"] <= 0.677
    assert abs(bias) <= 0.002


def test_render_interactive(rt, gpu_scenes):
    """Three views: shapes, history from the second view on, and two runs with the same seeds are bit-identical."""
    w, h = 48, 36
    base = gpu_scenes["cornell_box"]
    cam = base.camera()
    views = [rt.look_at(cam["pos"], (50.0, 40.0, 0.0)), rt.look_at((60.0, 55.0, 260.0), (50.0, 40.0, 0.0)),
             dict(rt.look_at((45.0, 50.0, 270.0), (50.0, 40.0, 0.0)), view_spp=40)]

    def run():
        return list(rt.render_interactive(base, views, w, h, first=8, max_n=16, abs_tol=0.02, view_spp=24, seed=SEED))

    a, b = run(), run()
    assert len(a) == 3
    for (rgb, frac, samples), (rgb2, frac2, samples2) in zip(a, b):
        assert rgb.shape == (h, w, 3) and rgb.dtype == np.uint8
        assert np.array_equal(rgb, rgb2) and frac == frac2 and samples == samples2
    assert a[0][1] == 0.0 and a[1][1] > 0.5 and a[2][1] > 0.5
    assert a[0][2] >= 2 * 8 * w * h and all(f[2] <= 24 * w * h for f in a[:2]) and a[2][2] <= 40 * w * h
    assert a[0][2] > 2 * 8 * w * h  # the first view has no history: sparse passes ran


def test_interactive_job_keeps_the_history_between_requests(rt, gpu_scenes):
    """server.InteractiveJob (RT_REPROJECT): two requests with two cameras send the two frames render_interactive
    yields for those views; the second starts from the first one's history."""
    from rt_amd import server

    w, h = 60, 45
    base = gpu_scenes["cornell_box"]
    cams = [dict(pos=(50.0, 52.0, 295.6), dir=(0.0, -0.042612, -1.0)), dict(pos=(64.0, 58.0, 255.6), dir=(-0.1, -0.092612, -1.0))]
    sent = []

    async def send(msg):
        sent.append(msg)

    job = server.InteractiveJob(send, max_n=16, first=8)

    async def go():
        for cam in cams:
            assert not job.running()
            assert await job.run(base.view(**cam), w, h, 16, SEED) is False

    asyncio.run(go())
    assert len(sent) == 2 * h and not job.running()
    frames = np.zeros((2, h, w, 3), dtype=np.uint8)
    for i, m in enumerate(sent):
        _, n, x, y = struct.unpack("<BBHH", m[:6])
        frames[i // h, y, x:x + n] = np.frombuffer(m[6:], dtype=np.uint8).reshape(n, 3)
    want = list(rt.render_interactive(base, cams, w, h, first=8, max_n=16, seed=SEED))
    assert want[0][1] == 0.0 and want[1][1] > 0.5
    assert np.array_equal(frames[0], want[0][0]) and np.array_equal(frames[1], want[1][0])


def test_server_round_trip_with_a_camera(rt, gpu_scenes, monkeypatch):
    """One render request with "camera": the frame is rt_amd.render of the view."""
    from rt_amd import server
    from test_ws_server import H, W, _session

    monkeypatch.setenv("RT_SEED", hex(SEED))
    base = gpu_scenes["cornell_box"]
    cam = dict(pos=[64.0, 58.0, 255.6], dir=[-0.1, -0.092612, -1.0], fov=0.6)
    srv = server.Server({"cornell_box": base}, renderer=server.gpu_band_renderer(), width=W, height=H, band_rows=16,
                        log=lambda *_: None)
    got = asyncio.run(_session(srv, [json.dumps({"type": "render", "scene": "cornell_box", "spp": 8, "camera": cam})]))
    assert len(got) == H
    frame = np.zeros((H, W, 3), dtype=np.uint8)
    for m in got:
        _, n, x, y = struct.unpack("<BBHH", m[:6])
        frame[y, x:x + n] = np.frombuffer(m[6:], dtype=np.uint8).reshape(n, 3)
    view = base.view(tuple(cam["pos"]), tuple(cam["dir"]), fov=0.6)
    want, _, _ = rt.render(view, W, H, 8, SEED, megakernel=True)
    assert np.array_equal(frame, want)
    assert not np.array_equal(want, rt.render(base, W, H, 8, SEED, megakernel=True)[0])
