"""The query batteries (tests/query_rays.py) against the CPU oracle alone: the conditions that keep the GPU
tests of tests/test_gpu_queries.py from being vacuous. A family that fails one of them is a bug of its generator."""
import numpy as np
import pytest

import query_rays as qr
from conftest import scene_path

CASES = (("cornell_box", False), ("cubes", False), ("flying_unicorn", False), ("cubes", True), ("flying_unicorn", True))
RAY_FAMILIES = {"room", "secondary", "ties", "axis", "sphere_edges"}
MESH_RAY_FAMILIES = {"mesh_features", "root_ties"}
SEG_FAMILIES = {"nee", "ladder", "ladder_planes", "plane_contact"}


@pytest.fixture(scope="module")
def nearest_scenes(oracle):
    return {n: oracle.OracleScene(scene_path(n), mesh_nearest=True) for n in ("cubes", "flying_unicorn")}


@pytest.fixture(params=CASES, ids=lambda c: c[0] + ("-nearest" if c[1] else ""))
def battery(request, oracle_scenes, nearest_scenes):
    name, nearest = request.param
    return qr.reference(name, (nearest_scenes if nearest else oracle_scenes)[name], nearest)


def test_families_present_finite_and_sized(battery):
    b = battery
    has_mesh = bool(b.scene.meshes)
    assert set(b.rays) == RAY_FAMILIES | (MESH_RAY_FAMILIES if has_mesh else set())
    assert set(b.segs) - {"ladder_unstable"} == SEG_FAMILIES | ({"mesh_box"} if has_mesh else set())
    total = 0
    for f, (o, d) in b.rays.items():
        assert len(o) > 0 and o.shape == d.shape, f
        assert np.isfinite(o).all() and np.isfinite(d).all(), f
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 4e-16, f  # unit to rounding
        total += len(o)
    for f, (x, y) in b.segs.items():
        assert len(x) > 0 and x.shape == y.shape, f
        assert np.isfinite(x).all() and np.isfinite(y).all(), f
        assert np.any(x != y, axis=1).all(), f
        total += len(x)
    brute = b.scene.name == "flying_unicorn" and b.nearest  # the brute-force oracle: a tenth of the battery
    assert total <= (6000 if brute else 52000), total
    if has_mesh and len(b.scene.meshes[0][2]) > 64:
        assert len(b.rays["mesh_features"][0]) >= 200 * 3  # every sampled triangle: vertex, edge midpoint, centroid


def test_full_unicorn_battery_covers_2000_triangles(oracle_scenes):
    b = qr.reference("flying_unicorn", oracle_scenes["flying_unicorn"])
    kind = b.meta["mesh_features"]["kind"]
    assert min(np.count_nonzero(kind == k) for k in (0, 1, 2)) >= 2000
    assert sum(len(v[0]) for v in b.rays.values()) + sum(len(v[0]) for v in b.segs.values()) <= 52000


def test_tie_families(battery):
    """The constructed quotients (wall - o_k) / d_k are bit-equal on the tied axes, every edge and corner of the room
    is covered, and the oracle returns the tie's t and the lowest object index of the tie."""
    b = battery
    o, d, fam, names, t, ids, pos, nrm = b.ref_rays
    m = fam == names.index("ties")
    meta = b.meta["ties"]
    assert set(meta["keys"]) == set(meta["all_keys"]) and len(meta["all_keys"]) == 8 + 4
    for (axes, walls), oo, dd, tq in zip(meta["keys"], o[m], d[m], meta["t"]):
        q = [(p - oo[k]) / dd[k] for k, p in zip(axes, walls)]
        assert len({np.float64(x).tobytes() for x in q}) == 1 and q[0] == tq and tq > 0
        assert all(dd[k] == 0.0 for k in range(3) if k not in axes)
    assert (t[m] == meta["t"]).all()
    assert (ids[m] == meta["want"]).all()
    # the duplicate right wall never wins: object 1 stands before object 5 at x = 99
    assert set(ids[m].tolist()) == {0, 1, 2}  # x = 1, x = 99 and z = 0 walls win their ties (y walls: 3, 4)


def test_axis_family_straddles_the_thresholds(battery):
    o, d = battery.rays["axis"]
    a = np.abs(d)
    for v in (9e-5, 1e-4, 1.1e-4, 1e-300):
        assert (a == v).any(axis=0).all(), v  # on every axis
    exact = (a == 1.0).any(axis=1) & ((d == 0.0).sum(axis=1) == 2)  # +-e_k
    assert exact.sum() >= 24 and len({r.tobytes() for r in d[exact]}) == 24  # 6 directions x 4 signs of the zeros
    assert (np.signbit(d[exact]) & (d[exact] == 0.0)).any()  # -0 components


def test_mesh_feature_rays_hit_their_mesh(battery, oracle_scenes):
    b = battery
    if not b.scene.meshes:
        return  # cornell_box: the family does not exist (test_families_present_finite_and_sized)
    o, d, fam, names, t, ids, pos, nrm = b.ref_rays
    m = fam == names.index("mesh_features")
    obj, kind = b.meta["mesh_features"]["obj"], b.meta["mesh_features"]["kind"]
    for i in np.unique(obj):
        frac = (ids[m][obj == i] == i).mean()
        assert frac >= 0.8, (i, frac)
    assert ((kind == 0) & (ids[m] == obj)).any()  # a ray aimed at a vertex, and it hits
    if b.scene.name == "cubes":
        # octree and nearest-triangle results both present and identical in t on some ray: the mesh was hit
        other = qr.reference("cubes", oracle_scenes["cubes"])
        t2, id2 = other.ref_rays[4][m], other.ref_rays[5][m]
        assert np.array_equal(other.ref_rays[0], o)
        assert ((ids[m] == obj) & (id2 == obj) & (t[m] == t2)).any()


def test_nee_visible_fraction(battery):
    x, y, fam, names, vis = battery.ref_segs
    frac = vis[fam == names.index("nee")].mean()
    assert 0.2 <= frac <= 0.8, frac


def test_margin_ladder(battery):
    """Sphere and mesh hits: every rung up to 0.0009 past the hit is visible, every rung from 0.0011 is occluded, and
    the rung at exactly 0.001 goes both ways, each at least 10 %: there the outcome hangs on the last bits of t,
    |y - x| and the direction."""
    b = battery
    x, y, fam, names, vis = b.ref_segs
    v = vis[fam == names.index("ladder")].reshape(-1, len(qr.LADDER))
    assert len(v) >= 50
    dl = np.array(qr.LADDER)
    assert v[:, dl <= 0.0009].all()
    assert not v[:, dl >= 0.0011].any()
    at = v[:, dl == 0.001].mean()
    assert 0.1 <= at <= 0.9, at
    # every ray family with hits on spheres or meshes has rungs
    have = set(np.unique(b.meta["ladder"]["fam"]))
    assert have >= {k for k, f in enumerate(b.ref_rays[3]) if f != "ties"}, have
