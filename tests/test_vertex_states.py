"""The vertex batteries of tests/vertex_states.py, checked with the CPU oracle alone (no GPU): every family reaches
the branch it is aimed at, in the stated number; `state_for` inverts the stream; the forward step of the oracle
(orc_vertex) adds up to the recursion's frames; and the device's algebraic forms (variant 1) agree with the
reference's expressions (variant 0) to the measured bound, itself at most 1e-12."""
import numpy as np
import pytest

import vertex_states as vs

CASES = [(n, m) for n in vs.SCENES for m in (False, True)]
IDS = [f"{n}-{'mis' if m else 'nee'}" for n, m in CASES]


def _b(case):
    return vs.reference(*case)


def test_state_for_inverts_the_stream(oracle):
    rng = np.random.default_rng(vs.SEED)
    for k in range(8):
        for v in (0, 1, vs.M_SURVIVE, vs.P53 - 1, int(rng.integers(0, vs.P53))):
            s0, s1 = vs.state_for(k, v, rng)
            draws, after = oracle.stream(s0, s1, k + 1)
            assert draws[k] == v * 2.0 ** -53, (k, v)
            s = (s0, s1)
            for _ in range(k + 1):
                r, s = vs.step(*s)
            assert (r >> 11) == v and s == after
    # unstep is step's inverse
    s = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
    assert vs.unstep(*vs.step(*s)[1]) == s


def test_threshold_is_the_devices():
    """kP53Survive: 0.9 * 2^53 is an integer, and uniform() < 0.9 is exactly draw < M."""
    assert float(vs.M_SURVIVE) == 0.9 * 2.0 ** 53
    assert (vs.M_SURVIVE - 1) * 2.0 ** -53 < 0.9 and not (vs.M_SURVIVE * 2.0 ** -53 < 0.9)


@pytest.mark.parametrize("name", ["cornell_box", "cubes"])
@pytest.mark.parametrize("mis", [False, True])
def test_forward_walk_adds_up_to_the_recursion(name, mis):
    """Stepping orc_vertex from the camera states and summing each path's final L in sample order gives
    orc_render's subpixel means to 1e-13 relative (the sums associate differently), in both variants."""
    orc = vs.oracle_scene(name)
    w, h, spp = 12, 9, 16
    ns = spp // 4
    _, sub, _ = orc.render(w, h, spp, vs.SEED, mis=mis)
    row, col, s, m = (a.ravel() for a in np.meshgrid(np.arange(h), np.arange(w), np.arange(4), np.arange(ns),
                                                      indexing="ij"))
    for variant in (0, 1):
        st, rg, dk = orc.camera_states(w, h, vs.SEED, col, row, s, m)
        L = np.zeros((len(st), 3))
        act = np.arange(len(st))
        while len(act):
            o = orc.vertex(st, rg, dk, mis=mis, variant=variant)
            L[act] = o["st"][:, vs.RAD]
            c = o["info"][:, vs.CONT] == 1
            act, st, rg, dk = act[c], o["st"][c], o["rng"][c], o["dk"][c]
        Lr = L.reshape(h, w, 4, ns, 3)
        acc = np.zeros((h, w, 4, 3))
        for k in range(ns):
            acc = acc + Lr[:, :, :, k] * (1.0 / ns)
        assert np.all(np.abs(acc - sub) <= 1e-13 * np.abs(sub)), variant


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_walk_and_steered_families(case):
    b = _b(case)
    sc, info = b.scene, b.ref["info"]
    hit, kind, depth = info[:, vs.HIT], b.dk[:, 1], b.dk[:, 0]
    brdf = np.where(hit >= 0, sc.brdf[np.maximum(hit, 0)], -1)
    w = b.rows("walk")
    assert len(b.st) <= 22000 and len(w) >= 1500
    assert set(np.unique(kind[w])) == ({0, 1, 2} if (sc.brdf == vs.SPECULAR).any() else {0, 2})
    assert depth[w].max() >= 8 and all((depth[w] == d).any() for d in range(9))
    on_light = int((hit == sc.light).sum())
    assert on_light >= 200
    if (sc.brdf == vs.SPECULAR).any():
        assert int(((kind == vs.K_SPEC) & (brdf == vs.SPECULAR)).sum()) >= 200  # mirror then mirror
        assert int(((kind == vs.K_SPEC) & (hit == sc.light)).sum()) >= 200      # mirror then light
        assert int(((kind != vs.K_SPEC) & (brdf == vs.SPECULAR)).sum()) >= 200  # onto a mirror: bemit / o handed over
    mis_hit = (kind == vs.K_DIFF) & (hit == sc.light) & (b.st[:, vs.PDF_PREV] > 0)
    assert int(mis_hit.sum()) >= (200 if b.mis else 0)
    if not b.mis:
        assert not (b.st[:, vs.PDF_PREV] != 0).any()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_roulette_family(case):
    """The forced draw decides survival exactly as uniform() < p: always at depth <= 5 after the increment, draw < M
    from 6 on; on every BRDF the scene has."""
    b = _b(case)
    r = b.rows("roulette")
    meta = b.meta["roulette"]
    assert len(r) == len(meta) >= 240
    info = b.ref["info"][r]
    brdf_hit = np.where(info[:, vs.HIT] >= 0, b.scene.brdf[np.maximum(info[:, vs.HIT], 0)], -1)
    assert (brdf_hit == meta[:, 0]).all()  # the base vertices hit what they were chosen for
    after = meta[:, 1] + 1
    want = np.where(after <= 5, 1, (meta[:, 2] < vs.M_SURVIVE).astype(int))
    assert (info[:, vs.SURVIVED] == want).all()
    assert set(np.unique(meta[:, 0])) == set(np.unique(b.scene.brdf))
    for d in (5, 6, 7):
        for v in vs.RR_VALUES:
            assert ((after == d) & (meta[:, 2] == v)).sum() >= 16
    assert (b.dk[r, 0] == meta[:, 1]).all() and (b.ref["dk"][r, 0] == after).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lobe_and_light_draw_families(case):
    b = _b(case)
    sc = b.scene
    out, info, aux = b.ref["st"], b.ref["info"], b.ref["aux"]
    for label, idx in (("lobe_u1", sc.n_light + 1), ("lobe_u2", sc.n_light + 2)) + \
            ((("light_xi1", 0), ("light_xi2", 1)) if not sc.mesh_light else ()):
        r = b.rows(label)
        vals = b.meta[label]
        assert len(r) == len(vals) >= 36
        for i, v in zip(r, vals):
            assert oracle_draw(b, i, idx) == v * 2.0 ** -53
    r = b.rows("lobe_u1")
    zero = r[b.meta["lobe_u1"] == 0]
    zero = zero[info[zero, vs.SURVIVED] == 1]  # (a base vertex past depth 5 may lose its roulette)
    # u1 = 0: z = 0, the sampled direction lies in the surface, cos = 0 to rounding, and the reference's 0 / 0
    cw = np.einsum("ij,ij->i", aux[zero, 7:10], out[zero][:, vs.RAY_D])
    assert len(zero) >= 8 and (np.abs(cw) < 1e-15).all()
    assert (cw == 0.0).sum() >= 1  # the device's cw != 0 escape is taken
    assert np.isnan(b.ref0["st"][zero[cw == 0.0]][:, vs.BETA]).all()
    assert set(np.unique(b.meta["lobe_u2"])) == set(vs.U2_VALUES) and len(vs.U2_VALUES) == 40
    if "frame_switch" in b.names:
        nx = np.abs(aux[b.rows("frame_switch"), 7])
        assert (nx > 0.1).sum() >= 20 and (nx <= 0.1).sum() >= 20 and (np.abs(nx - 0.1) < 1e-15).sum() >= 8
    else:
        assert sc.name != "cornell_box"  # the only scene with a diffuse sphere that reflects
    if not sc.mesh_light:
        # cosl <= 0 and dot(n, i) <= 0 under NEE and MIS, a tiny cosl, the light's near field
        nee = np.flatnonzero(info[:, vs.NEE_VIS] >= 0)
        d = aux[nee, 4:7] - aux[nee, 1:4]
        i = d / np.linalg.norm(d, axis=1, keepdims=True)
        cosl = -np.einsum("ij,ij->i", aux[nee, 10:13], i)
        cosn = np.einsum("ij,ij->i", aux[nee, 7:10], i)
        assert (cosl <= 0).sum() >= 1000 and (cosn <= 0).sum() >= 150 and (np.abs(cosl) < 1e-3).sum() >= 3
        near = b.rows("near_light")
        g = sc.objects[sc.light]["geometry"]
        dist = np.linalg.norm(aux[near, 1:4] - np.array(g["pos"]), axis=1) - g["r"]
        assert len(near) == 64 and (info[near, vs.NEE_VIS] >= 0).all() and (dist < 3 * g["r"]).all()


def oracle_draw(b, i, idx):
    return vs.oracle_bind.stream(int(b.rng[i, 0]), int(b.rng[i, 1]), idx + 1)[0][idx]


def test_mesh_light_pick_family():
    """Around every chosen cumulative-area boundary the pick changes triangle within the five draws, and the largest
    draw picks the last triangle."""
    for mis in (False, True):
        b = _b(("quirks", mis))
        r = b.rows("light_pick")
        m = b.meta["light_pick"]
        tri = b.ref["info"][r, vs.LIGHT_TRI]
        n_tri = len(m["cum"])
        assert n_tri == 12 and (tri >= 0).all()
        for j in (0, n_tri // 2, n_tri - 2):
            got = set(np.unique(tri[m["boundary"] == j]))
            assert got == {j, j + 1}, (j, got)
        assert (tri[m["value"] == vs.P53 - 1] == n_tri - 1).all() and (tri[m["value"] == 0] == 0).all()
        assert (np.bincount(b.ref["info"][:, vs.LIGHT_TRI][b.ref["info"][:, vs.LIGHT_TRI] >= 0], minlength=12) > 0).all()


@pytest.mark.parametrize("name", ["phong_room", "quirks"])
def test_phong_family(name):
    """Both thresholds of the lobe choice have draws on either side: all three branches on every Phong object, odd
    and even powers, and sampled directions below the surface."""
    for mis in (False, True):
        b = _b((name, mis))
        r = b.rows("phong_lobe")
        meta, info = b.meta["phong_lobe"], b.ref["info"][r]
        powers = set()
        for i in np.unique(meta[:, 0]):
            o = b.scene.objects[i]["brdf"]
            powers.add(int(o["power"]) % 2)
            kd, ks = float(o["kd"]), float(o["ks"])
            assert kd + ks < 1.0
            sel = (meta[:, 0] == i) & (info[:, vs.SURVIVED] == 1)
            u = meta[sel, 1] * 2.0 ** -53
            want = np.where(u < kd, 2, np.where(u < kd + ks, 3, 4))
            assert (info[sel, vs.LOBE] == want).all() and set(np.unique(want)) == {2, 3, 4}
            for t in (kd, kd + ks):  # the draws straddle the threshold within two ulps
                near = u[np.abs(u - t) <= 3 * 2.0 ** -53]
                assert (near < t).any() and (near >= t).any()
        assert powers == ({0, 1} if name == "phong_room" else {0})
        lobe = b.ref["info"][:, vs.LOBE]
        cw = np.einsum("ij,ij->i", b.ref["aux"][:, 7:10], b.ref["st"][:, vs.RAY_D])
        assert ((lobe == 4) & (b.ref["info"][:, vs.CONT] == 0)).sum() >= 100  # absorption: in = 0 ends the path
        assert (((lobe == 2) | (lobe == 3)) & (cw < 0)).sum() >= 100      # below the surface


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zero_term_families(case):
    b = _b(case)
    info = b.ref["info"]
    r = b.rows("kd_zero")
    on_kd0 = np.isin(info[r, vs.HIT], b.scene.kd0)
    assert on_kd0.sum() >= 48
    k = r[on_kd0]
    # Le f == 0: variant 1 skips the shadow ray, variant 0 traces it; the draws are the same
    assert (info[k, vs.NEE_VIS] == -2).all() and (b.ref0["info"][k, vs.NEE_VIS] >= 0).all()
    assert (b.ref["rng"][k] == b.ref0["rng"][k]).all() and (info[k, vs.SURVIVED] == b.ref0["info"][k, vs.SURVIVED]).all()
    z = b.rows("beta_zero")
    alive = z[info[z, vs.SURVIVED] == 1]
    spec = b.scene.brdf[np.maximum(info[alive, vs.HIT], 0)] == vs.SPECULAR
    assert len(alive) >= 30 and (info[alive, vs.CONT] == spec).all()
    m = b.rows("miss")
    assert len(m) == 96 and (info[m, vs.HIT] == -1).all() and (info[m, vs.CONT] == 0).all()
    assert (b.ref["st"][m].view(np.uint64) == b.st[m].view(np.uint64)).all()


@pytest.mark.parametrize("mis", [False, True])
def test_deferred_shadow_segments_on_the_cubes(mis):
    """The cubes' shadow segments that pass the analytic objects (the scene without its meshes): at least 300 that
    a mesh blocks, 300 that pass a near mesh and 300 with an empty near mask. The near mask itself is the device's
    f32 cull's answer (tests/test_gpu_vertices.py counts on it); here the two classes are counted by what any sound
    cull must answer: a visible segment that crosses a mesh's cull box (f64 slab test) has that mesh in its mask, and
    one whose bounding box stays a unit clear of every cull box (the cull's pad is 2^-16 of the scene's extent) has
    none."""
    import query_rays as qr

    b = _b(("cubes", mis))
    rows, x, y, visible, clear = vs.nee_segments(b)
    assert not (visible & ~clear).any()  # the meshes only ever take visibility away
    assert (clear & ~visible).sum() >= 300 and (~clear).sum() >= 300
    crosses = np.zeros(len(x), dtype=bool)
    far = np.ones(len(x), dtype=bool)
    d = y - x
    for m in qr.Scene("cubes", b.scene.orc).meshes:
        lo, hi = m[5], m[6]
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (lo - x) / d, (hi - x) / d
        t0 = np.nanmax(np.minimum(ta, tb), axis=1).clip(min=0.0)
        t1 = np.nanmin(np.maximum(ta, tb), axis=1).clip(max=1.0)
        crosses |= t0 <= t1
        far &= ((np.maximum(x, y) < lo - 1.0) | (np.minimum(x, y) > hi + 1.0)).any(axis=1)
    assert not (crosses & far).any()
    assert (clear & visible & crosses).sum() >= 300 and (clear & far).sum() >= 300


def test_device_forms_agree_with_the_references_expressions():
    """Variant 1 against variant 0 over every battery: no worse than the recorded measurement (vertex_states
    FORMS_REL), which is at most 1e-12 (the forms agree to ~1e-15; the frame tests allow 1e-9)."""
    got = vs.measure_forms()
    print("variant 1 vs variant 0, largest relative difference:", got)
    for k, v in got.items():
        assert v <= vs.FORMS_REL[k], (k, v, vs.FORMS_REL[k])
        assert vs.FORMS_REL[k] <= 1e-12
