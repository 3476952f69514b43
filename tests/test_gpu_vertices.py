"""The f64 integrator's vertex, shade_vertex<C, Cold> (csrc/device/integrator_f64.h) with brdf_sample, brdf_eval,
light_sample, sincos_2pi, Rng::below53 and kP53Survive, against the CPU oracle vertex by vertex, through every
instantiation the render kernels run (rt_diag.h rt_diag_vertex: the fused forms RT_DIAG_FUSED / _G0 / _G1 / _LDS and
the deferred-shadow forms RT_DIAG_SPLIT_SLOTS / _ROLES / _KIDS / _FLAT, which resolve a pending shadow query as their kernel
family does and add ShadowDefer::c iff no mesh occludes), on the batteries of tests/vertex_states.py (whose own
conditions tests/test_vertex_states.py checks on the CPU). No statistical allowance: every vertex of every family is
compared.

The reference is the oracle's variant 1 (oracle.cpp vertex_step): the device's algebraic forms (shade_vertex's NEE term
through one reciprocal and its continuation weight as k / p, the host-evaluated DevObject::lef and brdf_eval's
DevObject::kpi, the cancelled MIS weights) written in plain IEEE C++ with glibc's libm. Both sides are built
without floating-point contraction (-ffp-contract=off in raytracer-server_amd/Makefile's COMMON flags for every f64
kernel file, and in oracle/Makefile), so with equal libm results the device must produce variant 1's bits.

Exact, every vertex: the hit object, the continue flag, kind, depth, the RNG state after (it moves iff Russian
roulette passed, so survival is compared everywhere), pdf_prev == 0 against > 0, the next ray's origin, and the bits
of bemit and o (copies); a NaN equals a NaN. The Phong lobe and the NEE visibility are not device outputs (a render
lane carries neither on), so they are compared through what they decide: absorption exactly (the stream moved, the
next direction is the zero vector, the path ends <=> the oracle's lobe is absorption); the diffuse against the
specular lobe in the next direction, beta and pdf_prev; the visibility in L, whose NEE term is all or nothing.

Numeric (L, beta, the next direction, pdf_prev), per vertex and per output:
    |device - ref1| <= 2 * max over nudges |ref1(nudge) - ref1(0)| + 2 ulp(max-norm of ref1)
where a nudge moves glibc's sin and cos (and, in scenes with a Phong object, the specular lobe's two pow results) by
-1 / 0 / +1 ulp: the factor 2 because the device's trig is claimed within 1 ulp of glibc, itself up to an ulp from the
true value; the 2 ulp term for norm() of a nudged vector. Where no libm call feeds an output (mirror and camera
vertices, beta as shade_vertex's k / p, the whole of a mesh light's NEE) the envelope is zero and the comparison is bit for
bit up to the 2 ulp term. Nothing in the bound is measured on the device.

Each battery is submitted twice, in family order and under a fixed permutation, both padded to a size that is no
multiple of 64, so the wave votes of sqrt_rn, div_sqrt and rcp_any pass in some waves and fail in others; a lane's
result must not depend on its wave-mates."""
import numpy as np
import pytest

import vertex_states as vs

pytestmark = pytest.mark.gpu

# (scene, form, mis, nearest-triangle mode): every fused form the scene admits
CASES = []
for _name, _forms in (("cornell_box", ("DIAG_FUSED", "DIAG_FUSED_G0", "DIAG_FUSED_LDS")),
                      ("cubes", ("DIAG_FUSED", "DIAG_FUSED_G1", "DIAG_FUSED_LDS")),
                      ("phong_room", ("DIAG_FUSED", "DIAG_FUSED_G0", "DIAG_FUSED_LDS")),
                      ("quirks", ("DIAG_FUSED", "DIAG_FUSED_G1", "DIAG_FUSED_LDS"))):
    CASES += [(_name, f, m, False) for f in _forms for m in (False, True)]
CASES += [("cubes", "DIAG_FUSED", False, True), ("cubes", "DIAG_FUSED_G1", True, True),
          ("cubes", "DIAG_FUSED_LDS", True, True), ("quirks", "DIAG_FUSED_LDS", False, True)]
# the deferred-shadow forms: the cubes admit all three (flat octrees with slot tables; no mirror: the query pool's
# nospec instances); the quirk scene's Phong and mirror objects take the wavefront's F = 11 / 15 instances
DEFERRED = [("cubes", f, m, False) for f in ("DIAG_SPLIT_SLOTS", "DIAG_SPLIT_ROLES", "DIAG_SPLIT_KIDS", "DIAG_SPLIT_FLAT")
            for m in (False, True)]
CASES += DEFERRED + [("quirks", "DIAG_SPLIT_KIDS", False, False), ("quirks", "DIAG_SPLIT_KIDS", True, False)]
IDS = [f"{n}-{f[5:].lower()}-{'mis' if m else 'nee'}{'-nearest' if nr else ''}" for n, f, m, nr in CASES]

_SCENES = {}
_RUNS = {}  # case -> (family-order pass, permuted pass un-permuted), shared by the tests (read only)


def _scene(rt, name):
    if rt.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need an MI355X")
    if name not in _SCENES:
        _SCENES[name] = rt.Scene.from_toml(vs.scene_file(name))
    return _SCENES[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _pad(*arrays):
    """A batch whose size is no multiple of the wave size (64): a copy of the first rows is appended if need be."""
    k = 1 if len(arrays[0]) % 64 == 0 else 0
    return tuple(np.concatenate([a, a[:k]]) for a in arrays)


def _run(case, rt):
    if case not in _RUNS:
        name, form, mis, nearest = case
        b = vs.reference(name, mis, nearest)
        sc = _scene(rt, name)
        n = len(b.st)
        st, rg, dk = _pad(b.st, b.rng, b.dk)
        assert len(st) % 64 != 0
        kw = dict(form=getattr(rt, form), mis=mis, mesh_nearest=nearest)
        first = sc.diag_vertex(st, rg, dk, **kw)
        perm = np.random.default_rng(vs.SEED + 1).permutation(len(st))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        second = sc.diag_vertex(st[perm], rg[perm], dk[perm], **kw)
        _RUNS[case] = ({k: v[:n] for k, v in first.items()}, {k: v[inv][:n] for k, v in second.items()})
    return _RUNS[case]


def _report(what, bad, b, extra):
    idx = np.flatnonzero(bad)
    per = {b.names[k]: int(np.count_nonzero(b.fam[idx] == k)) for k in np.unique(b.fam[idx])}
    first = "; ".join(
        f"#{i} [{b.names[b.fam[i]]}] depth {b.dk[i, 0]} kind {b.dk[i, 1]} rng {[hex(int(x)) for x in b.rng[i]]} "
        f"ray {b.st[i, :6].tolist()} beta {b.st[i, 6:9].tolist()} pdf_prev {b.st[i, 18]!r}: {extra(i)}"
        for i in idx[:4])
    return f"{what}: {len(idx)} of {len(bad)} vertices differ {per}: {first}"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_vertex_exact_outputs(case, rt):
    b = vs.reference(case[0], case[2], case[3])
    dev, _ = _run(case, rt)
    ref = b.ref
    checks = {
        "hit object": dev["info"][:, 0] != ref["info"][:, vs.HIT],
        "continue flag": dev["info"][:, 1] != ref["info"][:, vs.CONT],
        "depth": dev["dk"][:, 0] != ref["dk"][:, 0],
        "kind": dev["dk"][:, 1] != ref["dk"][:, 1],
        "RNG state after (survival)": (dev["rng"] != ref["rng"]).any(axis=1),
        "pdf_prev == 0 / > 0": (dev["st"][:, vs.PDF_PREV] > 0) != (ref["st"][:, vs.PDF_PREV] > 0),
        "next ray origin": (_bits(dev["st"][:, vs.RAY_O]) != _bits(ref["st"][:, vs.RAY_O])).any(axis=1),
        "bemit": (_bits(dev["st"][:, vs.BEMIT]) != _bits(ref["st"][:, vs.BEMIT])).any(axis=1),
        "o": (_bits(dev["st"][:, vs.OUT]) != _bits(ref["st"][:, vs.OUT])).any(axis=1),
    }
    if not case[1].startswith("DIAG_SPLIT"):
        checks["deferral (none in a fused form)"] = (dev["info"][:, 2:] != 0).any(axis=1)
    # The Phong lobe, as far as the device shows it. Absorption (oracle lobe 4) <=> the stream moved (roulette passed),
    # the next direction is the zero vector bit for bit and the path ends. The diffuse and specular lobes draw the
    # same number of values and both continue: which of them was taken shows only in the direction, beta and
    # pdf_prev (test_vertex_numeric_outputs).
    moved = (dev["rng"] != b.rng).any(axis=1)
    zero_dir = (_bits(dev["st"][:, vs.RAY_D]) == 0).all(axis=1)
    checks["Phong absorption"] = (ref["info"][:, vs.LOBE] == 4) != (moved & zero_dir & (dev["info"][:, 1] == 0))
    total = sum(int(v.sum()) for v in checks.values())
    print(f"{case}: {len(b.st)} vertices, {total} exact mismatches")
    for what, bad in checks.items():
        assert not bad.any(), _report(f"{what} {case}", bad, b, lambda i: (
            f"device info {dev['info'][i].tolist()} dk {dev['dk'][i].tolist()} oracle info {ref['info'][i].tolist()} "
            f"dk {ref['dk'][i].tolist()}"))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_vertex_numeric_outputs(case, rt):
    b = vs.reference(case[0], case[2], case[3])
    dev, _ = _run(case, rt)
    d, r, env = dev["st"], b.ref["st"], b.env
    for label, cols in (("L", vs.RAD), ("beta", vs.BETA), ("next direction", vs.RAY_D),
                        ("pdf_prev", slice(18, 19))):
        dv, rv, ev = d[:, cols], r[:, cols], env[:, cols]
        with np.errstate(invalid="ignore", over="ignore"):
            finite = np.isfinite(rv)
            norm = np.where(finite, np.abs(rv), 0.0).max(axis=1, keepdims=True)
            bound = 2.0 * ev + 2.0 * np.spacing(norm)
            err = np.abs(dv - rv)
            ok = np.where(finite, err <= bound, _bits(dv) == _bits(rv))  # inf: the same inf
            ok |= np.isnan(rv) & np.isnan(dv)                            # a NaN equals a NaN
        bad = ~ok.all(axis=1)
        exact = int((ev == 0).all(axis=1).sum())
        worst = float(np.nanmax(np.where(finite & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)))
        print(f"{case} {label}: {len(bad)} vertices ({exact} with a zero envelope), {int(bad.sum())} outside the bound, "
              f"largest error {worst:.3f} of the bound")
        assert not bad.any(), _report(f"{label} {case}", bad, b, lambda i: (
            f"device {dv[i].tolist()} oracle {rv[i].tolist()} bound {bound[i].tolist()}"))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_vertex_lane_independent(case, rt):
    """The same vertices under a fixed permutation (mixed waves), un-permuted: bit-identical to the family-order pass."""
    b = vs.reference(case[0], case[2], case[3])
    first, second = _run(case, rt)
    bad = np.zeros(len(b.st), dtype=bool)
    for k in first:
        a, c = first[k], second[k]
        a, c = (_bits(a), _bits(c)) if a.dtype == np.float64 else (a, c)
        bad |= (a != c).reshape(len(bad), -1).any(axis=1)
    assert not bad.any(), _report(f"order {case}", bad, b, lambda i: (
        f"L {first['st'][i, vs.RAD].tolist()} / {second['st'][i, vs.RAD].tolist()}"))


@pytest.mark.parametrize("case", DEFERRED, ids=[IDS[CASES.index(c)] for c in DEFERRED])
def test_deferred_shadow_is_pending_iff_a_mesh_could_block(case, rt):
    """ShadowDefer::pending is set iff the oracle's segment passes the analytic objects (the scene without its meshes)
    and the form's near mask (rt_diag_visible, whose soundness tests/test_gpu_queries.py checks) is non-empty, and
    ShadowDefer::meshes is that mask. The battery holds at least 300 shadow segments each that a mesh blocks, that
    pass a near mesh, and that have an empty near mask (the L of all of them is compared in
    test_vertex_numeric_outputs: the deferred term is added iff no mesh occludes).
    Assumption: the expected values are taken on the oracle's segment (x, y). x is the device's bit for bit, but y is
    the light sample, whose sin and cos may be an ulp apart between glibc and the device, so a segment within an ulp
    of a decision (the f32 cull's padded box, whose pad is 2^-16 of the scene's extent, or an analytic occluder's
    0.001 margin) could be expected one way and shaded the other without anything being wrong. No battery segment is
    that close (0 differ); a mismatch here is to be checked against that before it is called a fault."""
    name, form, mis, _ = case
    b = vs.reference(name, mis)
    dev, _ = _run(case, rt)
    rows, x, y, visible, clear = vs.nee_segments(b)
    # (the roles pool shares the slot form's query code: rt_diag_visible has no form of its own for it)
    qform = rt.DIAG_SPLIT_SLOTS if form == "DIAG_SPLIT_ROLES" else getattr(rt, form)
    _, near = _scene(rt, name).diag_visible(x, y, form=qform)
    want = np.zeros(len(b.st), dtype=bool)
    want[rows] = clear & (near != 0)
    mask = np.zeros(len(b.st), dtype=np.int64)
    mask[rows] = np.where(want[rows], near, 0)
    bad = ((dev["info"][:, 2] != 0) != want) | (dev["info"][:, 3] != mask)
    counts = (int((clear & ~visible).sum()), int((clear & visible & (near != 0)).sum()), int((clear & (near == 0)).sum()))
    print(f"{case}: {len(rows)} shadow segments: a mesh blocks {counts[0]}, pass a near mesh {counts[1]}, "
          f"empty near mask {counts[2]}; {int(bad.sum())} differ")
    assert not bad.any(), _report(f"pending {case}", bad, b, lambda i: (
        f"device pending {dev['info'][i, 2]} meshes {dev['info'][i, 3]} expected {int(want[i])} / {mask[i]}"))
    assert min(counts) >= 300, counts
    assert not ((near == 0) & clear & ~visible).any()  # (a blocked segment's mesh is in the mask)


def _ordered(x):
    """Doubles as integers in their numeric order (neighbouring doubles differ by 1; -0 and +0 coincide)."""
    i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    return np.where(i < 0, np.int64(-(2 ** 63)) - i, i)


def test_sincos_2pi_within_one_ulp_of_glibc(rt, oracle):
    """path_f64.h / DESIGN.md §2: sincos_2pi is within 1 ulp of glibc's sin and cos. On 2 pi u for 2^20 random 53-bit
    u, for every k / 8 with 0 .. 4 ulps (2^-53) either side, and for u = 0, 2^-53, 1 - 2^-53."""
    if rt.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need an MI355X")
    rng = np.random.default_rng(vs.SEED + 2)
    v = [rng.integers(0, vs.P53, size=1 << 20, dtype=np.int64)]
    v.append(np.array(sorted({(k << 50) + d for k in range(9) for d in range(-4, 5) if 0 <= (k << 50) + d < vs.P53}
                             | {0, 1, vs.P53 - 1}), dtype=np.int64))
    u = np.concatenate(v).astype(np.float64) * 2.0 ** -53  # exact
    x = 2.0 * np.pi * u  # the path's own product, 2.0 * PI * uniform()
    s_d, c_d = rt.diag_sincos(x)
    s_o, c_o = oracle.sincos(x)
    ds, dc = np.abs(_ordered(s_d) - _ordered(s_o)), np.abs(_ordered(c_d) - _ordered(c_o))
    print(f"sincos_2pi: {len(x)} arguments; sin differs from glibc by 1 ulp on {int((ds == 1).sum())}, cos on "
          f"{int((dc == 1).sum())}; more than 1 ulp: sin {int((ds > 1).sum())}, cos {int((dc > 1).sum())}")
    bad = (ds > 1) | (dc > 1)
    assert not bad.any(), "; ".join(
        f"x={x[i]!r} (u={u[i]!r}) sin {s_d[i]!r} / {s_o[i]!r} cos {c_d[i]!r} / {c_o[i]!r}" for i in np.flatnonzero(bad)[:6])
