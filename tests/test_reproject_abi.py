"""Accumulator reprojection (rt_accum_reproject) without a GPU: every argument check, and the numpy /
oracle restatement tests/reproject_ref.py against its own properties (the GPU tests compare the device to it)."""
import ctypes

import numpy as np
import pytest

import reproject_ref as rr
from conftest import scene_path

RT_E_INVAL = -1
W, H = 96, 72


def _accum(rt, w=8, h=6, device=0):
    a = ctypes.c_void_p()
    assert rt.lib.rt_accum_create(device, w, h, ctypes.byref(a)) == 0
    return a


def test_invalid_arguments_come_back_without_a_device(rt):
    """Each check in the header's order; rt_last_error names the one that fired. (A src with K >= 2 needs a device, so
    the K < 2 check is the last one reachable here: every other check sits in front of it.)"""
    L = rt.lib
    base = rt.Scene.from_toml(scene_path("cornell_box"))
    other = rt.Scene.from_toml(scene_path("cornell_box"))
    v = base.view((40.0, 50.0, 250.0), (0.0, 0.0, -1.0))
    vv = v.view((41.0, 50.0, 250.0), (0.0, 0.0, -1.0))
    dst, src, small, dev1 = _accum(rt), _accum(rt), _accum(rt, 8, 5), _accum(rt, 8, 6, device=1)
    n = ctypes.c_int64(-7)

    def call(d, s, dv, sv, flags=0, max_n=4):
        rc = L.rt_accum_reproject(d, s, dv.handle if dv else None, sv.handle if sv else None, flags, max_n,
                                  ctypes.byref(n))
        return rc, L.rt_last_error().decode()

    try:
        for args in ((None, src, v, base), (dst, None, v, base), (dst, src, None, base), (dst, src, v, None)):
            rc, msg = call(*args)
            assert rc == RT_E_INVAL and "null" in msg
        rc, msg = call(dst, dst, v, base)
        assert rc == RT_E_INVAL and "two accumulators" in msg
        for s in (small, dev1):
            rc, msg = call(dst, s, v, base)
            assert rc == RT_E_INVAL and "size or device" in msg
        rc, msg = call(dst, src, v, other)
        assert rc == RT_E_INVAL and "share a base" in msg
        for bad in (0, -3):
            rc, msg = call(dst, src, v, base, max_n=bad)
            assert rc == RT_E_INVAL and "max_n" in msg
        for flags in (rt.FLAG_MIS, rt.FLAG_FP32, rt.FLAG_MEGAKERNEL, 1 << 9, rt.FLAG_MESH_NEAREST | rt.FLAG_MIS):
            rc, msg = call(dst, src, v, base, flags=flags)
            assert rc == RT_E_INVAL and "unknown flag" in msg
        # views of one base in any combination pass the base check and reach the src K < 2 check
        for dv, sv in ((v, base), (base, v), (vv, v), (vv, base), (base, base)):
            for flags in (0, rt.FLAG_MESH_NEAREST):
                rc, msg = call(dst, src, dv, sv, flags=flags)
                assert rc == RT_E_INVAL and "two full-frame passes" in msg
        assert n.value == -7  # never written on failure
        info = np.zeros(4, dtype=np.int64)
        assert L.rt_accum_info(dst, info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == 0
        assert info.tolist() == [0, 0, 8, 6]
    finally:
        for a in (dst, src, small, dev1):
            L.rt_accum_destroy(a)


# The restatement against its own properties ----------------------------------------------------------------

@pytest.fixture(scope="module")
def classified(oracle, oracle_scenes):
    """classify() of the issue's moves at 96 x 72, computed once."""
    out = {}
    for name, moves in (("cornell_box", ("A", "B")), ("cubes", ("A",)), ("flying_unicorn", ("A", "B"))):
        path = scene_path(name)
        kinds = rr.brdf_kinds(path)
        v0 = rr.scene_view(path)
        for mv in moves:
            v1 = rr.scene_view(path, rr.MOVE_A if mv == "A" else rr.MOVE_B)
            out[name, mv] = rr.classify(oracle_scenes[name], kinds, v1, v0, W, H)
    return out


@pytest.mark.parametrize("name", ("cornell_box", "cubes", "flying_unicorn"))
def test_identical_views_map_every_subpixel_onto_itself(oracle_scenes, name):
    """With dst = src the geometric steps send each of the 27,648 subpixels to itself, facing and visible from the
    camera (every object taken as diffuse); with the scene's BRDFs only the non-diffuse hits drop out."""
    path = scene_path(name)
    v0 = rr.scene_view(path)
    kinds = rr.brdf_kinds(path)
    c = rr.classify(oracle_scenes[name], np.zeros_like(kinds), v0, v0, W, H)
    assert c["ok"].all() and c["ok"].size == 27648
    assert np.array_equal(c["q"], np.broadcast_to(np.arange(W * H).reshape(H, W, 1), (H, W, 4)))
    assert np.array_equal(c["jp"], np.broadcast_to(np.arange(4), (H, W, 4)))
    c2 = rr.classify(oracle_scenes[name], kinds, v0, v0, W, H)
    counts = rr.class_counts(c2)
    assert sum(counts.values()) == counts["non_diffuse"] == int((~c2["ok"]).sum())
    assert np.array_equal(c2["q"][c2["ok"]], c["q"][c2["ok"]]) and np.array_equal(c2["jp"][c2["ok"]], c["jp"][c2["ok"]])


# valid share and rejected subpixels per class. The issue's table counts as "occluded" every subpixel that is not
# mutually visible with the old camera; by the order of the definition's steps a few of those (3 / 0 / 8 in move A)
# already fail the same-side test of step 5, so occluded + back_side is the issue's figure.
TABLE = {
    ("cornell_box", "A"): (0.907, dict(non_diffuse=1898, hidden=494, out_of_frame=0)),
    ("cubes", "A"): (0.976, dict(non_diffuse=0, hidden=436, out_of_frame=0)),
    ("flying_unicorn", "A"): (0.864, dict(non_diffuse=1898, hidden=1358, out_of_frame=0)),
    ("cornell_box", "B"): (0.622, dict(out_of_frame=9018)),
    ("flying_unicorn", "B"): (0.602, dict(out_of_frame=9018)),
}


@pytest.mark.parametrize("case", sorted(TABLE))
def test_class_counts_of_the_moves(classified, case):
    c = classified[case]
    share, want = TABLE[case]
    counts = rr.class_counts(c)
    counts["hidden"] = counts["occluded"] + counts["back_side"]
    print(case, counts, c["ok"].all(-1).mean())
    assert round(float(c["ok"].all(-1).mean()), 3) == share
    for k, v in want.items():
        assert counts[k] == v, (k, counts)
    assert counts["miss"] == 0 and counts["behind"] == 0  # the shipped scenes are closed rooms in front of the camera
    assert sum(rr.class_counts(c).values()) == int((~c["ok"]).sum())
    # what the gather reads stays inside the frame
    assert c["q"].min() >= 0 and c["q"].max() < W * H and c["jp"].min() >= 0 and c["jp"].max() <= 3


def test_counts_and_sums_follow_the_definition(classified):
    """A src with per-pixel counts: N_p = min(max_n, min_j N_qj), K_p = max(2, min_j ceil(K_qj N_p / N_qj)), the
    subpixel mean S / N and Q / N survive the rescale, an invalid pixel is all zeros."""
    c = classified["cornell_box", "A"]
    rng = np.random.default_rng(5)
    N = rng.integers(2, 40, size=(H, W))
    K = np.minimum(N, rng.integers(2, 9, size=(H, W)))
    S = rng.uniform(-1.0, 50.0, size=(H, W, 4, 3))
    Q = rng.uniform(0.0, 90.0, size=(H, W, 4, 3))
    max_n = 12
    Sd, Qd, Kd, Nd, n_valid = rr.reproject(S, Q, K, N, c, max_n)
    valid = c["ok"].all(-1)
    assert n_valid == int(valid.sum()) and 0 < n_valid < W * H
    assert not Sd[~valid].any() and not Qd[~valid].any() and not Kd[~valid].any() and not Nd[~valid].any()
    Kf, Nf = K.reshape(-1), N.reshape(-1)
    checked = 0
    for r, col in zip(*np.nonzero(valid)):
        if (r * W + col) % 97:
            continue  # a sample of the pixels, one by one in plain Python integers
        qs = [int(x) for x in c["q"][r, col]]
        n_p = min(max_n, min(int(Nf[q]) for q in qs))
        k_p = max(2, min(-(-int(Kf[q]) * n_p // int(Nf[q])) for q in qs))
        assert (int(Nd[r, col]), int(Kd[r, col])) == (n_p, k_p)
        for j, q in enumerate(qs):
            jp = int(c["jp"][r, col, j])
            for ch in range(3):
                want = float(n_p) * (S.reshape(-1, 4, 3)[q, jp, ch] / float(Nf[q]))
                assert Sd[r, col, j, ch] == want
        checked += 1
    assert checked > 30
    assert (Nd[valid] <= max_n).all() and (Nd[valid] >= 2).all() and (Kd[valid] >= 2).all()
    assert (Kd[valid] <= np.maximum(2, Nd[valid])).all()  # K_q <= N_q in src, so no more passes than samples
    # the mean and the second moment per sample are the source's, to rounding
    m_src = (S / N[..., None, None]).reshape(-1, 4, 3)[c["q"], c["jp"]]
    m_dst = Sd[valid] / Nd[valid][:, None, None]
    assert np.allclose(m_dst, m_src[valid], rtol=4e-16, atol=0)
    # a huge max_n with uniform counts keeps (K, N)
    Su, Qu, Ku, Nu, _ = rr.reproject(S, Q, np.full((H, W), 4), np.full((H, W), 8), c, 1 << 30)
    assert (Ku[valid] == 4).all() and (Nu[valid] == 8).all()
    assert np.array_equal(Su[valid], (8.0 * (S / 8.0)).reshape(-1, 4, 3)[c["q"], c["jp"]][valid])


def test_seeded_accumulator_merges_instead_of_storing():
    a = rr.Accum(4, 3)
    S = np.arange(4 * 3 * 12, dtype=np.float64).reshape(3, 4, 4, 3)
    K = np.array([[2, 0, 3, 2]] * 3)
    N = np.array([[5, 0, 6, 2]] * 3)
    S[K == 0] = 0.0
    a.seed(S, S * 2.0, K, N)
    m = np.full((3, 4, 4, 3), 0.5)
    a.add_sub(m, 2)
    assert np.array_equal(a.S, S + 1.0) and np.array_equal(a.Q, S * 2.0 + 0.5)
    assert np.array_equal(a.K, K + 1) and np.array_equal(a.N, N + 2)
    a.add_sub(m, 2)
    assert (a.K >= 2).all() and np.isfinite(a.var()).all()
    assert np.array_equal(a.sub()[K == 0], m[K == 0])  # a pixel without history holds the new passes only
    b = rr.Accum(4, 3)
    b.add_sub(-m, 1)
    assert np.array_equal(b.S, -m)  # the first pass of a fresh accumulator stores


def test_moved_toml_keeps_everything_but_the_camera(tmp_path, oracle):
    v = rr.scene_view(scene_path("cubes"), rr.MOVE_A)
    path, assets = rr.moved_toml(scene_path("cubes"), v, tmp_path)
    import tomli

    with open(path, "rb") as f:
        moved = tomli.load(f)
    with open(scene_path("cubes"), "rb") as f:
        orig = tomli.load(f)
    assert moved["objects"] == orig["objects"]
    assert moved["camera"] == dict(pos=v["pos"].tolist(), dir=v["dir"].tolist())
    assert oracle.OracleScene(path, assets_dir=assets).light == oracle.OracleScene(scene_path("cubes")).light
