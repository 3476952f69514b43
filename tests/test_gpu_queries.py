"""The query code of every kernel family against the CPU oracle, ray by ray and segment by segment, on the
batteries of tests/query_rays.py (whose own conditions tests/test_query_rays.py checks on the CPU): DESIGN.md §2
claims the device traces the reference's rays bit for bit, so there is no allowance here: object, t, position and
normal of every ray, and the visibility of every segment, equal the oracle's in every form (rt_diag.h RT_DIAG_*).
Each battery is submitted twice, in family order (whole waves of one kind) and under a fixed permutation (waves
that mix tangent, axis-parallel, tie and ordinary rays, so the wave votes of the exact-arithmetic shortcuts, of
flat_query and of the root order pass in some waves and fail in others); a lane's result must not depend on its
wave-mates. Nothing renders."""
import numpy as np
import pytest

import query_rays as qr
from conftest import scene_path

pytestmark = pytest.mark.gpu

# (scene, form, nearest-triangle mode): every form the scene admits
CASES = [("cornell_box", "DIAG_FUSED", False), ("cornell_box", "DIAG_FUSED_G0", False),
         ("cubes", "DIAG_FUSED", False), ("cubes", "DIAG_SPLIT_SLOTS", False), ("cubes", "DIAG_SPLIT_KIDS", False),
         ("cubes", "DIAG_SPLIT_FLAT", False),
         ("flying_unicorn", "DIAG_FUSED", False), ("flying_unicorn", "DIAG_SPLIT_SLOTS", False),
         ("flying_unicorn", "DIAG_SPLIT_KIDS", False),
         ("cubes", "DIAG_FUSED", True), ("flying_unicorn", "DIAG_FUSED", True),
         ("cubes", "DIAG_FUSED_G1", False), ("flying_unicorn", "DIAG_FUSED_G1", False),
         ("cubes", "DIAG_FUSED_G1", True), ("flying_unicorn", "DIAG_FUSED_G1", True)]
IDS = [f"{n}-{f[5:].lower()}{'-nearest' if nr else ''}" for n, f, nr in CASES]

_NEAREST = {}
_TRACE = {}  # case -> the device's first-pass results, shared by the tests (read only)


def _battery(case, oracle, oracle_scenes):
    name, _, nearest = case
    if not nearest:
        return qr.reference(name, oracle_scenes[name])
    if name not in _NEAREST:
        _NEAREST[name] = oracle.OracleScene(scene_path(name), mesh_nearest=True)
    return qr.reference(name, _NEAREST[name], True)


def _pad(a, b):
    """A batch whose size is no multiple of the wave size (64): one copy of the first query is appended if need be."""
    k = 1 if len(a) % 64 == 0 else 0
    return np.vstack([a, a[:k]]), np.vstack([b, b[:k]])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _report(what, bad, fam, names, extra):
    idx = np.flatnonzero(bad)
    per = {names[k]: int(np.count_nonzero(fam[idx] == k)) for k in np.unique(fam[idx])}
    first = "; ".join(f"#{i} [{names[fam[i]]}] {extra(i)}" for i in idx[:6])
    return f"{what}: {len(idx)} of {len(bad)} differ {per}: {first}"


def _device_trace(case, rt, gpu_scenes, b):
    if case not in _TRACE:
        name, form, nearest = case
        o, d = _pad(b.ref_rays[0], b.ref_rays[1])
        assert len(o) % 64 != 0
        n = len(b.ref_rays[0])
        res = gpu_scenes[name].diag_trace(o, d, form=getattr(rt, form), mesh_nearest=nearest)
        perm = np.random.default_rng(qr.SEED).permutation(len(o))
        res_p = gpu_scenes[name].diag_trace(o[perm], d[perm], form=getattr(rt, form), mesh_nearest=nearest)
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        _TRACE[case] = (tuple(a[:n] for a in res), tuple(a[inv][:n] for a in res_p))
    return _TRACE[case]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_trace_every_ray_bit_exact(case, rt, gpu_scenes, oracle, oracle_scenes):
    """obj, t, pos and n of every ray of every family are the oracle's, bit for bit (uint64 views)."""
    b = _battery(case, oracle, oracle_scenes)
    o, d, fam, names, t_o, id_o, p_o, n_o = b.ref_rays
    (t, ids, prim, pos, nrm), _ = _device_trace(case, rt, gpu_scenes, b)
    hit = id_o >= 0
    bad = (ids != id_o) | (_bits(t) != _bits(t_o))
    bad |= hit & (np.any(_bits(pos) != _bits(p_o), axis=1) | np.any(_bits(nrm) != _bits(n_o), axis=1))
    print(f"{case}: {len(bad)} rays, {np.count_nonzero(bad)} differ")
    assert not bad.any(), _report(f"trace {case}", bad, fam, names, lambda i: (
        f"o={o[i].tolist()} d={d[i].tolist()} device obj {ids[i]} t {t[i]!r} oracle obj {id_o[i]} t {t_o[i]!r}"))
    on_mesh = np.isin(id_o, [m[0] for m in b.scene.meshes])
    assert (prim[on_mesh] >= 0).all() and (prim[~on_mesh] == -1).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_trace_lane_independent(case, rt, gpu_scenes, oracle, oracle_scenes):
    """The same rays under a fixed permutation (mixed waves), un-permuted: bit-identical to the family-order pass."""
    b = _battery(case, oracle, oracle_scenes)
    fam, names = b.ref_rays[2], b.ref_rays[3]
    first, second = _device_trace(case, rt, gpu_scenes, b)
    bad = np.zeros(len(fam), dtype=bool)
    for a, c in zip(first, second):
        a2, c2 = (_bits(a), _bits(c)) if a.dtype == np.float64 else (a, c)
        bad |= (a2 != c2).reshape(len(fam), -1).any(axis=1)
    assert not bad.any(), _report(f"trace order {case}", bad, fam, names, lambda i: (
        f"obj {first[1][i]} / {second[1][i]} t {first[0][i]!r} / {second[0][i]!r}"))


@pytest.mark.parametrize("name", ["cornell_box", "cubes", "flying_unicorn"])
def test_hit_triangle_agrees_between_forms(name, rt, gpu_scenes, oracle, oracle_scenes):
    """The oracle reports no triangle; the forms of one scene (octree mode) name the same one on every ray."""
    cases = [c for c in CASES if c[0] == name and not c[2]]
    b = _battery(cases[0], oracle, oracle_scenes)
    fam, names = b.ref_rays[2], b.ref_rays[3]
    prims = [_device_trace(c, rt, gpu_scenes, b)[0][2] for c in cases]
    for c, p in zip(cases[1:], prims[1:]):
        bad = p != prims[0]
        assert not bad.any(), _report(f"prim {c} vs {cases[0]}", bad, fam, names, lambda i: f"{p[i]} / {prims[0][i]}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_visible_every_segment(case, rt, gpu_scenes, oracle, oracle_scenes):
    """Every segment of every family: the oracle's mutually_visible; the permuted pass gives the same answers and
    masks; and the split forms' cull is sound on its own: when the oracle's segment is occluded and its nearest hit
    is on a mesh, that mesh is in the near mask. (rt_diag_trace has no mask output: there a mesh culled wrongly
    shows as a different hit object in test_trace_every_ray_bit_exact.)"""
    name, form, nearest = case
    b = _battery(case, oracle, oracle_scenes)
    x, y, fam, names, vis_o = b.ref_segs
    xs, ys = _pad(x, y)
    assert len(xs) % 64 != 0
    n = len(x)
    sc = gpu_scenes[name]
    vis, near = sc.diag_visible(xs, ys, form=getattr(rt, form), mesh_nearest=nearest)
    perm = np.random.default_rng(qr.SEED + 1).permutation(len(xs))
    vis_p, near_p = sc.diag_visible(xs[perm], ys[perm], form=getattr(rt, form), mesh_nearest=nearest)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    bad = vis[:n] != vis_o
    print(f"{case}: {n} segments, {np.count_nonzero(bad)} differ")
    assert not bad.any(), _report(f"visible {case}", bad, fam, names, lambda i: (
        f"x={x[i].tolist()} y={y[i].tolist()} device {vis[i]} oracle {vis_o[i]}"))
    bad = (vis_p[inv][:n] != vis[:n]) | (near_p[inv][:n] != near[:n])
    assert not bad.any(), _report(f"visible order {case}", bad, fam, names, lambda i: (
        f"{vis[i]} / {vis_p[inv][i]} mask {near[i]} / {near_p[inv][i]}"))
    if not form.startswith("DIAG_SPLIT"):
        assert not near.any()
        return
    if not hasattr(b, "seg_hits"):  # the oracle's nearest hit along every segment, once per battery
        dd = y - x
        b.seg_hits = b.scene.orc.trace(x, dd / np.linalg.norm(dd, axis=1, keepdims=True))[1]
    mesh_objs = [m[0] for m in b.scene.meshes]
    checked = 0
    for k, obj in enumerate(mesh_objs):
        need = ~vis_o & (b.seg_hits == obj)
        checked += np.count_nonzero(need)
        bad = need & ((near[:n] >> k) & 1 == 0)
        assert not bad.any(), _report(f"cull {case} mesh {k}", bad, fam, names, lambda i: (
            f"x={x[i].tolist()} y={y[i].tolist()} mask {near[i]}"))
    assert checked > 500
