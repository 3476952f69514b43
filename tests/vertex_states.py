"""Batteries of path vertices for the vertex-by-vertex integrator tests (tests/test_vertex_states.py on the CPU,
tests/test_gpu_vertices.py on the device): named families of the state a render lane holds on arrival at a vertex
(ray, beta, L, bemit, o, pdf_prev, RNG state, depth, kind), aimed at the integrator's rare branches.

A state is a row of three arrays, the layout of OracleScene.vertex and Scene.diag_vertex: st (19 doubles), rng (the
xoroshiro128++ state, 2 uint64), dk (depth, kind). Every family starts from vertices of real paths (the `walk`
family, recorded by stepping the oracle) and replaces what it aims at: the ray (steered at an object), the depth, or
the RNG state, chosen with `state_for` so that one draw of the vertex has a wanted 53-bit value. The seed is fixed.

Draw order of a vertex from its arrival state (oracle.cpp vertex_step, integrator_f64.h shade_vertex): a mirror
draws Russian roulette only; every other vertex draws the light sample (sphere light: xi1, xi2; mesh light: the
triangle pick, then two for the point), Russian roulette, then the BSDF sample (diffuse: u1, u2; Phong: the lobe
choice, xi1, xi2)."""
import atexit
import os
import shutil
import tempfile

import numpy as np

import extra_scenes
import oracle_bind

SEED = 20241020
MASK = (1 << 64) - 1
P53 = 1 << 53
M_SURVIVE = int(0.9 * 9007199254740992.0)  # path_f64.h kP53Survive: 0.9 * 2^53 is an integer
K_CAMERA, K_SPEC, K_DIFF = 0, 1, 2
DIFFUSE, SPECULAR, PHONG = 0, 1, 2
SCENES = ("cornell_box", "cubes", "phong_room", "quirks")
# the oracle's info columns
HIT, CONT, SURVIVED, LOBE, NEE_VIS, LIGHT_TRI = range(6)
# st columns
RAY_O, RAY_D, BETA, RAD, BEMIT, OUT, PDF_PREV = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), slice(12, 15), \
    slice(15, 18), 18

# Largest relative difference between the oracle's variant 1 (the device's algebraic forms) and variant 0 (the
# reference's expressions) over all batteries, per numeric output, measured with
#   python -c "import sys; sys.path.insert(0, 'tests'); import vertex_states as vs; print(vs.measure_forms())"
# (tests/test_vertex_states.py re-measures and asserts it is not exceeded, and that it is at most 1e-12)
# measured: L 1.7317001930477973e-15, beta 5.997451018729811e-16, dir 0.0, pdf_prev 0.0 (dir and pdf_prev come out
# of brdf_sample, which both variants share)
FORMS_REL = dict(L=1.7317001930477973e-15, beta=5.997451018729811e-16, dir=0.0, pdf_prev=0.0)

_DIR = None


def _scratch_dir():
    """A directory of this process for the scene files written here, removed when the process ends."""
    global _DIR
    if _DIR is None:
        _DIR = tempfile.mkdtemp(prefix="vertex_scenes_")
        atexit.register(shutil.rmtree, _DIR, ignore_errors=True)
    return _DIR


def scene_file(name):
    """The TOML of a battery scene: a reference scene, or one of extra_scenes written to a directory of this process."""
    if name in extra_scenes.TEXTS:
        p = os.path.join(_scratch_dir(), f"{name}.toml")
        return p if os.path.exists(p) else extra_scenes.write(_scratch_dir(), name)
    return os.path.join(oracle_bind.REPO, "scenes", f"{name}.toml")


# ------------------------------------------------------------------------------------- xoroshiro128++, inverted

def _rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & MASK


def _rotr(x, k):
    return ((x >> k) | (x << (64 - k))) & MASK


def step(s0, s1):
    """One xoroshiro128++ step: (output, next state)."""
    r = (_rotl((s0 + s1) & MASK, 17) + s0) & MASK
    b = s1 ^ s0
    return r, (_rotl(s0, 49) ^ b ^ ((b << 21) & MASK), _rotl(b, 28))


def unstep(n0, n1):
    """The state whose step leads to (n0, n1): b' = rotr(n1, 28), a = rotr(n0 ^ b' ^ (b' << 21), 49), b = b' ^ a."""
    b = _rotr(n1, 28)
    a = _rotr(n0 ^ b ^ ((b << 21) & MASK), 49)
    return a, b ^ a


def state_for(draw_index, value53, rng):
    """A stream state whose draw number `draw_index` (0 = the next one) is value53 * 2^-53 exactly: at that draw the
    state is (a, b) with a and the output's low 11 bits random and b = rotr(r - a, 17) - a; earlier states by unstep."""
    assert 0 <= value53 < P53
    a = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
    r = (value53 << 11) | int(rng.integers(0, 1 << 11))
    b = (_rotr((r - a) & MASK, 17) - a) & MASK
    s = (a, b)
    for _ in range(draw_index):
        s = unstep(*s)
    return s


def ladder53(k8):
    """The 53-bit draws at k8 / 8 and one and two ulps (2^-53) either side, inside [0, 2^53)."""
    c = k8 << 50
    return sorted({v for v in (c - 2, c - 1, c, c + 1, c + 2) if 0 <= v < P53})


U2_VALUES = sorted({v for k in range(9) for v in ladder53(k)} | {0, P53 - 1})
U1_VALUES = (0, 1, P53 - 1)
RR_VALUES = (0, M_SURVIVE - 1, M_SURVIVE, M_SURVIVE + 1, P53 - 1)


# --------------------------------------------------------------------------------------------------- the scene

class Scene:
    """What the generators need of a battery scene: every object's BRDF and shape, the light, the draw layout."""

    def __init__(self, name, orc):
        import tomli

        self.name, self.orc = name, orc
        with open(scene_file(name), "rb") as f:
            spec = tomli.load(f)
        self.brdf = np.array([{"diffuse": DIFFUSE, "specular": SPECULAR, "phong": PHONG}[o["brdf"]["type"]]
                              for o in spec["objects"]])
        self.objects = spec["objects"]
        self.light = orc.light
        self.mesh_light = spec["objects"][self.light]["geometry"]["type"] != "sphere"
        self.n_light = 3 if self.mesh_light else 2  # draws of the light sample
        self.kd0 = [i for i, o in enumerate(spec["objects"])
                    if o["brdf"]["type"] == "diffuse" and not any(o["brdf"]["kd"])]

    def spheres(self, brdf=None):
        return [(i, np.array(o["geometry"]["pos"], dtype=np.float64), float(o["geometry"]["r"]))
                for i, o in enumerate(self.objects)
                if o["geometry"]["type"] == "sphere" and (brdf is None or self.brdf[i] == brdf)]

    def rr_index(self, brdf):
        """Which draw of a vertex on an object of this BRDF is the Russian-roulette one."""
        return 0 if brdf == SPECULAR else self.n_light

    def light_point(self, rng, n):
        """Points to aim at on the light: on a sphere light's surface, inside a mesh light's box."""
        g = self.objects[self.light]["geometry"]
        if not self.mesh_light:
            d = rng.normal(size=(n, 3))
            return np.array(g["pos"]) + 0.7 * float(g["r"]) * d / np.linalg.norm(d, axis=1, keepdims=True)
        bb = self.orc.mesh_stats(self.light)["bbox"]
        return rng.uniform(bb[:3] * 0.75 + bb[3:] * 0.25, bb[:3] * 0.25 + bb[3:] * 0.75, size=(n, 3))


class Rows:
    """Vertex states as the three arrays, with the family of every row."""

    def __init__(self):
        self.st, self.rng, self.dk, self.fam, self.names = [], [], [], [], []

    def add(self, name, st, rng, dk):
        st = np.asarray(st, dtype=np.float64).reshape(-1, 19)
        if not len(st):
            return
        if name not in self.names:
            self.names.append(name)
        self.st.append(st)
        self.rng.append(np.asarray(rng, dtype=np.uint64).reshape(-1, 2))
        self.dk.append(np.asarray(dk, dtype=np.int32).reshape(-1, 2))
        self.fam.append(np.full(len(st), self.names.index(name)))

    def done(self):
        self.st, self.rng, self.dk = np.vstack(self.st), np.vstack(self.rng), np.vstack(self.dk)
        self.fam = np.concatenate(self.fam)
        return self

    def rows(self, name):
        return np.flatnonzero(self.fam == self.names.index(name))


def _aim(st, target):
    """The rows' rays turned towards the target points (unit directions, origins kept)."""
    st = st.copy()
    d = target - st[:, RAY_O]
    st[:, RAY_D] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return st


def _states(rng, draw_index, values, reps):
    """reps states per value: (len(values) * reps, 2) uint64, value-major."""
    return np.array([state_for(draw_index, v, rng) for v in values for _ in range(reps)], dtype=np.uint64)


def _tile(a, n):
    """Rows of `a` repeated cyclically to n rows."""
    return a[np.arange(n) % len(a)]


# ------------------------------------------------------------------------------------------------ the families

def walk(sc, mis, rng, width=48, height=36, n_cam=900):
    """Every vertex of the paths of n_cam camera samples, recorded by stepping the oracle (variant 1) until each path
    ends: the arrival states, and the oracle's info of each vertex."""
    pix = rng.choice(width * height * 4, size=n_cam, replace=False)
    col, row, sub = (pix // 4) % width, (pix // 4) // width, pix % 4
    st, rg, dk = sc.orc.camera_states(width, height, SEED, col, row, sub, np.zeros(n_cam, dtype=np.int32))
    out_st, out_rng, out_dk, out_info = [], [], [], []
    while len(st):
        o = sc.orc.vertex(st, rg, dk, mis=mis, variant=1)
        out_st.append(st); out_rng.append(rg); out_dk.append(dk); out_info.append(o["info"])
        c = o["info"][:, CONT] == 1
        st, rg, dk = o["st"][c], o["rng"][c], o["dk"][c]
    return np.vstack(out_st), np.vstack(out_rng), np.vstack(out_dk), np.vstack(out_info)


def build(name, orc, mis):
    """The battery of scene `name` under the MIS flag `mis`: Rows, with b.scene and b.meta for the CPU test."""
    rng = np.random.default_rng([SEED, sum(name.encode()), int(mis)])
    sc = Scene(name, orc)
    b = Rows()
    b.scene, b.mis, b.meta = sc, bool(mis), {}
    w_st, w_rng, w_dk, w_info = walk(sc, mis, rng)
    b.add("walk", w_st, w_rng, w_dk)
    hit = w_info[:, HIT]
    on = lambda brdf: np.flatnonzero((hit >= 0) & (sc.brdf[np.maximum(hit, 0)] == brdf) & (hit != sc.light))
    kind = w_dk[:, 1]

    def pick(idx, n):
        return idx[rng.permutation(len(idx))[:n]] if len(idx) else idx

    # steered: paths arriving after a camera start, a mirror bounce and a diffuse bounce, turned towards the light
    # (a vertex on the light itself, mirror then light, the MIS BSDF hit with pdf_prev > 0) and towards the mirrors
    # (mirror then mirror)
    pool = {k: (w_st[kind == k], w_rng[kind == k], w_dk[kind == k]) for k in (K_CAMERA, K_SPEC, K_DIFF)}
    mirrors = sc.spheres(SPECULAR)

    def mirror_points(n):
        return np.array([mirrors[j % len(mirrors)][1] + 0.6 * mirrors[j % len(mirrors)][2] * rng.uniform(-1, 1, 3)
                         for j in range(n)])

    def steered(src, targets, wanted, n_hit, n_miss):
        """The rows of src = (st, rng, dk), tiled to len(targets), aimed at the targets: n_hit of those whose ray's
        first hit is one of the objects `wanted` and n_miss that something else stops."""
        j = np.arange(len(targets)) % len(src[0])
        st = _aim(src[0][j], targets)
        reach = np.isin(orc.trace(st[:, RAY_O], st[:, RAY_D])[1], wanted)
        keep = np.concatenate([np.flatnonzero(reach)[:n_hit], np.flatnonzero(~reach)[:n_miss]])
        return st[keep], src[1][j[keep]], src[2][j[keep]]

    if mirrors:
        # paths turned towards the mirrors after a camera start and a diffuse bounce; the states they leave the
        # mirror with (stepped with the oracle) join the walk's few after-a-mirror states as sources below
        extra = []
        for k, label in ((K_CAMERA, "camera"), (K_DIFF, "diffuse")):
            rows = steered(pool[k], mirror_points(1200), [m[0] for m in mirrors], 300, 40)
            b.add(f"to_mirror_after_{label}", *rows)
            o = orc.vertex(*rows, mis=mis, variant=1)
            go = (o["info"][:, CONT] == 1) & (o["dk"][:, 1] == K_SPEC)
            extra.append((o["st"][go], o["rng"][go], o["dk"][go]))
        pool[K_SPEC] = tuple(np.concatenate([pool[K_SPEC][c]] + [e[c] for e in extra]) for c in range(3))
    for k, label in ((K_CAMERA, "camera"), (K_SPEC, "mirror"), (K_DIFF, "diffuse")):
        if len(pool[k][0]):
            # candidates with several targets each; those that reach the light, and a few that something blocks
            b.add(f"to_light_after_{label}", *steered(pool[k], sc.light_point(rng, 3000), [sc.light], 400, 80))
    if mirrors and len(pool[K_SPEC][0]):
        b.add("to_mirror_after_mirror", *steered(pool[K_SPEC], mirror_points(2000), [m[0] for m in mirrors], 400, 40))

    # roulette: the Russian-roulette draw at 0, M - 1, M, M + 1, 2^53 - 1 (M = kP53Survive) at depths 4, 5, 6 on
    # arrival (5, 6, 7 after the increment: p = 1 up to 5, 0.9 from 6), on diffuse, mirror and Phong vertices
    meta = []
    for brdf in (DIFFUSE, SPECULAR, PHONG):
        src = pick(on(brdf), 16)
        if not len(src):
            continue
        for depth in (4, 5, 6):
            rs = _states(rng, sc.rr_index(brdf), RR_VALUES, len(src))
            st = _tile(w_st[src], len(rs))
            dk = _tile(w_dk[src], len(rs)).copy()
            dk[:, 0] = depth
            if depth > 0:
                dk[dk[:, 1] == K_CAMERA, 1] = K_DIFF  # only the first vertex of a path is a camera vertex
            b.add("roulette", st, rs, dk)
            meta += [(brdf, depth, v) for v in RR_VALUES for _ in range(len(src))]
    b.meta["roulette"] = np.array(meta)

    # diffuse lobe: u1 at 0 (cos = 0: the general form and the reference's 0 / 0), 2^-53, 1 - 2^-53; u2 on the
    # octant boundaries k / 8 of the trig reduction, two ulps either side, 0 and 1 - 2^-53
    src = pick(on(DIFFUSE), 12)
    if len(src):
        i_u1 = sc.n_light + 1
        for label, idx, vals in (("lobe_u1", i_u1, U1_VALUES), ("lobe_u2", i_u1 + 1, U2_VALUES)):
            rs = _states(rng, idx, vals, len(src))
            b.add(label, _tile(w_st[src], len(rs)), rs, _tile(w_dk[src], len(rs)))
            b.meta[label] = np.repeat(vals, len(src))
    # frame switch: diffuse spheres hit where the normal's x is 0.1 and within 1e-3 .. 1e-16 of it, either side
    # (local_coord's base vector switches at |n.x| > 0.1)
    balls = [s for s in sc.spheres(DIFFUSE) if s[0] != sc.light and s[0] not in sc.kd0]
    src = pick(np.flatnonzero(kind == K_DIFF), 8)
    if balls and len(src):
        st_l = []
        for _, c, r in balls:
            for e in (0.0, 1e-16, -1e-16, 1e-12, -1e-12, 1e-6, -1e-6, 1e-3, -1e-3):
                for sg in (1.0, -1.0):
                    for phi in rng.uniform(0.2, 1.3, 4):  # upper side (clear of the floor)
                        nx = sg * (0.1 + e)
                        n = np.array([nx, np.sqrt(1 - nx * nx) * np.sin(phi), np.sqrt(1 - nx * nx) * np.cos(phi)])
                        s = w_st[src[len(st_l) % len(src)]].copy()
                        s[RAY_O], s[RAY_D] = c + (r + 6.0) * n, -n
                        st_l.append(s)
        k = len(st_l)
        b.add("frame_switch", np.array(st_l), _tile(w_rng[src], k), _tile(w_dk[src], k))

    # light sample: xi1 at 0, 0.5, 1 - 2^-53 and xi2 on the ladder (sphere light); the triangle pick on every
    # cumulative-area boundary of the first, a middle and the last triangle, two ulps either side, and the largest
    # draw (mesh light)
    src = pick(np.concatenate([on(DIFFUSE), on(PHONG)]), 12)
    if len(src) and not sc.mesh_light:
        for label, idx, vals in (("light_xi1", 0, (0, P53 >> 1, P53 - 1)), ("light_xi2", 1, U2_VALUES)):
            rs = _states(rng, idx, vals, len(src))
            b.add(label, _tile(w_st[src], len(rs)), rs, _tile(w_dk[src], len(rs)))
            b.meta[label] = np.repeat(vals, len(src))
        # near field: vertices on whatever lies straight above the light, a few radii from its surface
        g = sc.objects[sc.light]["geometry"]
        c, r = np.array(g["pos"], dtype=np.float64), float(g["r"])
        k = 64
        near = pick(np.flatnonzero(kind == K_DIFF), 16)
        st = _tile(w_st[near], k).copy()
        st[:, RAY_O] = c + np.column_stack([rng.uniform(-r, r, k), np.full(k, r + 1.0), rng.uniform(-r, r, k)])
        st[:, RAY_D] = [0.0, 1.0, 0.0]
        b.add("near_light", st, _tile(w_rng[near], k), _tile(w_dk[near], k))
    if len(src) and sc.mesh_light:
        areas = orc.light_areas()
        cum = np.cumsum(areas)  # the same sequential sum as the pick's
        total = cum[-1]
        vals, tri = [], []
        for j in (0, len(cum) // 2, len(cum) - 2):
            v0 = int(round(cum[j] / total * P53))
            for v in range(v0 - 2, v0 + 3):
                vals.append(min(max(v, 0), P53 - 1)); tri.append(j)
        for v in (P53 - 1, P53 - 2, 0):
            vals.append(v); tri.append(-1)
        rs = _states(rng, 0, vals, len(src))
        b.add("light_pick", _tile(w_st[src], len(rs)), rs, _tile(w_dk[src], len(rs)))
        b.meta["light_pick"] = dict(value=np.repeat(vals, len(src)), boundary=np.repeat(tri, len(src)), cum=cum)

    # phong: the lobe choice at ph_kd and ph_kd + ph_ks, the 53-bit draws just below, at and above each threshold
    # (diffuse lobe, specular lobe, absorption), on objects with an even and an odd power
    meta = []
    for i in np.flatnonzero(sc.brdf == PHONG):
        src = pick(np.flatnonzero(hit == i), 12)
        if not len(src):
            continue
        kd, ks = float(sc.objects[i]["brdf"]["kd"]), float(sc.objects[i]["brdf"]["ks"])
        vals = sorted({min(max(int(np.floor(t * P53)) + d, 0), P53 - 1) for t in (kd, kd + ks) for d in (-1, 0, 1, 2)})
        rs = _states(rng, sc.n_light + 1, vals, len(src))
        b.add("phong_lobe", _tile(w_st[src], len(rs)), rs, _tile(w_dk[src], len(rs)))
        meta += [(i, v) for v in vals for _ in range(len(src))]
    if meta:
        b.meta["phong_lobe"] = np.array(meta)

    # zero terms: vertices on objects with kd = 0 (Le f = 0: the shadow ray is skipped, the draws are not), zero
    # throughput on arrival, rays that leave the scene
    if sc.kd0:
        src = pick(np.flatnonzero(kind != K_CAMERA), 96)
        tg = []
        for j in range(len(src)):
            g = sc.objects[sc.kd0[j % len(sc.kd0)]]["geometry"]
            if g["type"] == "sphere":
                tg.append(np.array(g["pos"]) + 0.5 * float(g["r"]) * rng.uniform(-1, 1, 3))
            elif g["type"] == "plane":  # an axis plane of the room: a point on it inside the room
                p = rng.uniform([5.0, 5.0, 5.0], [95.0, 75.0, 195.0])
                k = int(np.argmax(np.abs(g["n"])))
                p[k] = g["pos"][k]
                tg.append(p)
            else:
                tg.append(sc.light_point(rng, 1)[0])
        b.add("kd_zero", _aim(w_st[src], np.array(tg)), w_rng[src], w_dk[src])
    src = pick(np.flatnonzero(kind != K_CAMERA), 96)
    st = w_st[src].copy()
    st[:, BETA] = 0.0
    b.add("beta_zero", st, w_rng[src], w_dk[src])
    st = w_st[src].copy()
    st[:, RAY_O], st[:, RAY_D] = [500.0, 52.0, 295.6], [1.0, 0.0, 0.0]
    b.add("miss", st, w_rng[src], w_dk[src])
    return b.done()


_CACHE = {}
NUDGES = [(s, c, 0, 0) for s in (-1, 0, 1) for c in (-1, 0, 1) if (s, c) != (0, 0)]
POW_NUDGES = [(s, c, a, p) for s in (-1, 0, 1) for c in (-1, 0, 1) for a in (-1, 0, 1) for p in (-1, 0, 1)
              if (a, p) != (0, 0)]


def oracle_scene(name, nearest=False):
    key = ("scene", name, bool(nearest))
    if key not in _CACHE:
        _CACHE[key] = oracle_bind.OracleScene(scene_file(name), mesh_nearest=bool(nearest))
    return _CACHE[key]


def analytic_scene(name):
    """The scene without its mesh objects (the light stays: a sphere), as an OracleScene: its mutually_visible is the
    analytic half of the device's deferred shadow test. Sphere-light scenes only."""
    key = ("analytic", name)
    if key not in _CACHE:
        import tomli

        with open(scene_file(name), "rb") as f:
            spec = tomli.load(f)
        keep = [o for o in spec["objects"] if o["geometry"]["type"] in ("sphere", "plane")]
        assert any("emitted" in o for o in keep), "the light must be analytic"

        def val(v):  # the values a scene file holds: numbers, strings, lists and inline tables of them
            if isinstance(v, dict):
                return "{ " + ", ".join(f"{k} = {val(x)}" for k, x in v.items()) + " }"
            if isinstance(v, list):
                return "[" + ", ".join(val(x) for x in v) + "]"
            return f'"{v}"' if isinstance(v, str) else repr(float(v)) if isinstance(v, float) else repr(v)

        text = "[camera]\n" + "".join(f"{k} = {val(v)}\n" for k, v in spec["camera"].items())
        for o in keep:
            text += "[[objects]]\n" + "".join(f"{k} = {val(v)}\n" for k, v in o.items())
        p = os.path.join(_scratch_dir(), f"{name}_analytic.toml")
        with open(p, "w") as f:
            f.write(text)
        _CACHE[key] = oracle_bind.OracleScene(p)
    return _CACHE[key]


def nee_segments(b):
    """The shadow segments of the battery's vertices whose NEE term is evaluated (variant 1: Le f != 0): row
    indices, x, y, the oracle's visibility, and whether the analytic objects alone let the segment through."""
    rows = np.flatnonzero(b.ref["info"][:, NEE_VIS] >= 0)
    x, y = b.ref["aux"][rows, 1:4], b.ref["aux"][rows, 4:7]
    return rows, x, y, b.ref["info"][rows, NEE_VIS] == 1, analytic_scene(b.scene.name).visible(x, y)


def reference(name, mis, nearest=False):
    """The battery of (name, mis) with the oracle's answers, built once per process and shared (read only):
    b.ref = variant 1's output (OracleScene.vertex), b.ref0 = variant 0's, and b.env = per row, per st column, the
    largest |variant 1 with a nudge - variant 1| over the libm nudges (sin and cos by -1 / 0 / +1 ulp; for scenes
    with a Phong object also its two pow calls): how far an ulp of libm moves each output."""
    key = (name, bool(mis), bool(nearest))
    if key not in _CACHE:
        orc = oracle_scene(name, nearest)  # nearest: the nearest-triangle oracle (Mesh::intersect without the octree)
        b = build(name, orc, mis)
        b.ref = orc.vertex(b.st, b.rng, b.dk, mis=mis, variant=1)
        b.ref0 = orc.vertex(b.st, b.rng, b.dk, mis=mis, variant=0)
        env = np.zeros_like(b.st)
        has_phong = (b.scene.brdf == PHONG).any()
        with np.errstate(invalid="ignore"):
            for ng in NUDGES + (POW_NUDGES if has_phong else []):
                d = np.abs(orc.vertex(b.st, b.rng, b.dk, mis=mis, variant=1, nudge=ng)["st"] - b.ref["st"])
                env = np.fmax(env, d)  # (a NaN difference, inf - inf, counts as none: NaN rows compare by bits)
        b.env = env
        for a in (b.st, b.rng, b.dk, b.fam, b.env, *b.ref.values(), *b.ref0.values()):
            a.setflags(write=False)
        _CACHE[key] = b
    return _CACHE[key]


def forms_rel(b):
    """Largest relative difference of variant 1 from variant 0 per numeric output over the battery's vertices whose
    values are finite in both (norm-wise for the vectors: |v1 - v0|_max / |v0|_max)."""
    out = {}
    s1, s0 = b.ref["st"], b.ref0["st"]
    alive = b.ref["info"][:, SURVIVED] == 1
    for label, cols, rows in (("L", RAD, b.ref["info"][:, HIT] >= 0), ("beta", BETA, alive), ("dir", RAY_D, alive),
                              ("pdf_prev", slice(18, 19), alive)):
        a, r = s1[rows][:, cols], s0[rows][:, cols]
        ok = np.isfinite(a).all(axis=1) & np.isfinite(r).all(axis=1)
        den = np.abs(r[ok]).max(axis=1)
        num = np.abs(a[ok] - r[ok]).max(axis=1)
        rel = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
        out[label] = float(rel.max()) if len(rel) else 0.0
    return out


def measure_forms():
    worst = dict(L=0.0, beta=0.0, dir=0.0, pdf_prev=0.0)
    for name in SCENES:
        for mis in (False, True):
            for k, v in forms_rel(reference(name, mis)).items():
                worst[k] = max(worst[k], v)
    return worst
