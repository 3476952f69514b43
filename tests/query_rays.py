"""Batteries of rays (o, d) and segments (x, y) for the ray-by-ray query tests (tests/test_query_rays.py on the
CPU, tests/test_gpu_queries.py on the device): named families aimed at the places where a query's result hangs on
one comparison or one rounding (mesh vertices and edges, bit-equal t on two or three walls, axis-parallel
directions, tangent rays, surface origins, segments ending within the 0.001 margin of an occluder).

Pure numpy. A battery is built from a reference scene's TOML and its OracleScene (hit points, mesh vertices and
boxes come from the oracle); every input is finite, directions are unit to rounding, x != y, the seed is fixed.
`scale` shrinks the random counts (the brute-force nearest-triangle oracle of the unicorn gets scale = 0.1)."""
import itertools
import os

import numpy as np

import oracle_bind

SEED = 20240607
ROOM_LO, ROOM_HI = np.array([2.0, 1.0, 1.0]), np.array([98.0, 80.0, 200.0])
REL = (1e-15, 1e-12, 1e-9)
LADDER = (-1.0, -0.002, -0.0011, -0.001, -0.0009, 0.0, 0.0009, 0.001, 0.0011, 0.002, 1.0)
BOX_STEPS = (1e-9, 1e-7, 1e-5, 1e-3)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere_dirs(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _frame(n):
    """Two unit vectors perpendicular to each row of n (and to each other)."""
    a = np.where(np.abs(n[:, :1]) > 0.5, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    u = _unit(np.cross(a, n))
    return u, np.cross(n, u)


def room_rays(n, rng):
    """tests/test_gpu_parity.py's mix: camera-like rays, random rays inside the room, rays aimed at the mesh region."""
    o = np.empty((n, 3))
    d = rng.normal(size=(n, 3))
    k = n // 3
    o[:k] = [50.0, 52.0, 295.6]
    d[:k] = np.column_stack([rng.uniform(-0.35, 0.35, k), rng.uniform(-0.3, 0.25, k), -np.ones(k)])
    o[k:2 * k] = rng.uniform([2, 1, 1], [98, 80, 200], size=(k, 3))
    tgt = rng.uniform([12, 0, 25], [92, 60, 92], size=(n - 2 * k, 3))
    o[2 * k:] = rng.uniform([2, 1, 1], [98, 80, 250], size=(n - 2 * k, 3))
    d[2 * k:] = tgt - o[2 * k:]
    return o, _unit(d)


class Scene:
    """What the generators need of a reference scene: its axis planes, spheres, light and meshes."""

    def __init__(self, name, orc):
        import tomli

        self.name, self.orc = name, orc
        with open(os.path.join(oracle_bind.REPO, "scenes", f"{name}.toml"), "rb") as f:
            spec = tomli.load(f)
        self.planes = []   # (object, axis, coordinate)
        self.spheres = []  # (object, centre, r)
        self.meshes = []   # (object, vertices, triangles, root box min, root box max, cull box min, cull box max)
        self.light = None
        for i, o in enumerate(spec["objects"]):
            g = o["geometry"]
            if g["type"] == "plane":
                n = np.array(g["n"], dtype=np.float64)
                k = int(np.argmax(np.abs(n)))
                assert abs(n[k]) == 1.0 and np.count_nonzero(n) == 1, "axis planes only"
                self.planes.append((i, k, float(g["pos"][k])))
            elif g["type"] == "sphere":
                self.spheres.append((i, np.array(g["pos"], dtype=np.float64), float(g["r"])))
                if "emitted" in o and self.light is None:
                    self.light = self.spheres[-1]
            else:
                v, idx = orc.mesh_vertices(i)
                bb = orc.mesh_stats(i)["bbox"]
                self.meshes.append((i, v, idx, bb[:3].copy(), bb[3:].copy(), np.minimum(bb[:3], v.min(0)),
                                    np.maximum(bb[3:], v.max(0))))
        assert self.light is not None and orc.light == self.light[0]

    def walls(self, axis):
        """The distinct wall coordinates of an axis with the lowest object index at each."""
        out = {}
        for i, k, p in self.planes:
            if k == axis:
                out.setdefault(p, i)
        return sorted(out.items())


# ------------------------------------------------------------------------------------------------ ray families

def secondary_rays(sc, room, rng):
    """From the oracle's hit points of the room rays (surface point + 1e-5 n), cosine-distributed about the normal."""
    t, ids, pos, nrm = sc.orc.trace(*room)
    hit = ids >= 0
    pos, nrm = pos[hit], nrm[hit]
    u, v = _frame(nrm)
    r1, r2 = rng.uniform(size=len(pos)), rng.uniform(size=len(pos))
    z = np.sqrt(r1)
    r = np.sqrt(1.0 - r1)
    phi = 2.0 * np.pi * r2
    d = u * (r * np.cos(phi))[:, None] + v * (r * np.sin(phi))[:, None] + nrm * z[:, None]
    return pos, _unit(d)


def tie_rays(sc):
    """Rays to every edge (two walls) and corner (three walls) of the room with bit-equal t on the walls: the
    origin lies m from each wall, the direction has +-s on those axes (s = 1 / sqrt(2), 1 / sqrt(3)) and 0 on the
    third. Only origins whose numerators wall - o_k come out equal in magnitude (hence bit-equal quotients) are
    kept; `want` is the lowest object index among the tied walls, `axes` the tied axes, `t` the shared quotient."""
    os_, ds, want, key = [], [], [], []
    free = {0: (30.0, 50.0, 70.0), 1: (30.0, 45.0, 70.0), 2: (120.0, 150.0, 180.0)}  # clear of the objects
    for axes in list(itertools.combinations(range(3), 2)) + [(0, 1, 2)]:
        s = 1.0 / np.sqrt(float(len(axes)))
        for walls in itertools.product(*[sc.walls(k) for k in axes]):
            for m in (0.5, 3.0, 7.0, 11.0):
                rest = [k for k in range(3) if k not in axes]
                for f in (free[rest[0]] if rest else (0.0,)):
                    o, d = np.zeros(3), np.zeros(3)
                    for k, (p, _) in zip(axes, walls):
                        inward = 1.0 if p < ROOM_LO[k] else -1.0  # towards the room's inside
                        o[k] = p + inward * m
                        d[k] = -inward * s
                    if rest:
                        o[rest[0]] = f
                    os_.append(o)
                    ds.append(d)
                    want.append(min(i for _, i in walls))
                    key.append((axes, tuple(p for p, _ in walls)))
    o, d = np.array(os_), np.array(ds)
    want = np.array(want, dtype=np.int32)
    q = np.full((len(o), 3), np.nan)
    for j, (axes, ps) in enumerate(key):
        for k, p in zip(axes, ps):
            q[j, k] = (p - o[j, k]) / d[j, k]
    tied = np.array([len({x.tobytes() for x in row[~np.isnan(row)]}) == 1 for row in q])
    keys = [key[j] for j in np.flatnonzero(tied)]
    return o[tied], d[tied], want[tied], np.nanmax(q[tied], axis=1), keys, sorted(set(key))


def _targets(sc):
    """Points through and beside each sphere and each mesh's bounding box."""
    pts = []
    for _, c, r in sc.spheres:
        pts += [c] + [c + r * f * e for e in np.vstack([np.eye(3), -np.eye(3)]) for f in (0.999, 1.001)]
    for m in sc.meshes:
        c, h = (m[3] + m[4]) / 2, (m[4] - m[3]) / 2
        pts += [c] + [c + h * f * e for e in np.vstack([np.eye(3), -np.eye(3)]) for f in (0.999, 1.001)]
    return np.array(pts)


def axis_rays(sc, rng, scale):
    """Directions +-e_k with +0 and -0 elsewhere, and directions with one component of magnitude 9e-5, 1e-4, 1.1e-4
    (the plane test's |d_n| < 1e-4) or 1e-300 (outside the exact reciprocal's range), the others on the unit
    circle scaled to keep |d| = 1; through and beside each sphere and mesh box, from 60 before the target."""
    tg = _targets(sc)
    dirs = []
    for k in range(3):
        for sg in (1.0, -1.0):
            for z1, z2 in itertools.product((0.0, -0.0), repeat=2):
                d = np.array([z1, z2, 0.0])
                d = np.insert(d[:2], k, sg)
                dirs.append(d)
    nphi = 3 if scale >= 1.0 else 2
    for k in range(3):
        for eps in (9e-5, 1e-4, 1.1e-4, 1e-300):
            for sg in (1.0, -1.0):
                for phi in rng.uniform(0, 2 * np.pi, nphi):
                    c = np.sqrt(1.0 - eps * eps)
                    d = np.insert(np.array([c * np.cos(phi), c * np.sin(phi)]), k, sg * eps)
                    dirs.append(d)
    dirs = np.array(dirs)
    if scale < 1.0:
        tg = tg[rng.permutation(len(tg))[: max(6, int(len(tg) * scale * 2))]]
    o = (tg[:, None, :] - 60.0 * dirs[None, :, :]).reshape(-1, 3)
    d = np.broadcast_to(dirs[None], (len(tg),) + dirs.shape).reshape(-1, 3)
    # Slab entries: a ray that runs along axis j beside a box (a mesh's cull box, a sphere's bounds), outside its
    # slab of axis k, and drifts into that slab with the small component: it crosses the box's face k at the
    # face's centre after 150, or only past the box's far end. With 1e-300 it runs in the face's plane. These are
    # the culls' nearly-parallel cases (near_box's slab branch, the f32 cull's, the walks' subtree bounds).
    boxes = [(m[5], m[6]) for m in sc.meshes] + [(c - r, c + r) for _, c, r in sc.spheres]
    eo, ed = [], []
    for lo, hi in boxes:
        ctr, ext = (lo + hi) / 2, hi - lo
        for k in range(3):
            for j in [a for a in range(3) if a != k][: 2 if scale >= 1.0 else 1]:
                for eps in (9e-5, 1e-4, 1.1e-4, 1e-300):
                    for sg in (1.0, -1.0):
                        dd = np.zeros(3)
                        dd[k] = -sg * eps
                        dd[j] = np.sqrt(1.0 - eps * eps)
                        for beyond in (0.0, 0.6):
                            e = ctr.copy()
                            e[k] = hi[k] if sg > 0 else lo[k]
                            e[j] += beyond * ext[j]
                            eo.append(e - 150.0 * dd)
                            ed.append(dd)
    return np.vstack([o, np.array(eo)]), np.vstack([d, np.array(ed)])


def sphere_edge_rays(sc, rng, scale):
    """Tangent rays: aimed at centre + r (1 +- e) u for unit u perpendicular to the view direction; and origins on
    each sphere's surface moved k * 1e-4 along the normal (the eps test of t) and inside the sphere."""
    os_, ds = [], []
    nview = max(2, int(8 * scale))
    for _, c, r in sc.spheres:
        for o in rng.uniform(ROOM_LO, ROOM_HI, size=(nview, 3)):
            if np.linalg.norm(o - c) < 1.5 * r:
                o = c + np.array([0.0, 0.0, 3.0 * r])
            w = _unit(c - o)[None]
            u, v = _frame(w)
            for phi in rng.uniform(0, 2 * np.pi, 3):
                p = np.cos(phi) * u[0] + np.sin(phi) * v[0]
                for e in (0.0, 1e-15, 1e-12, 1e-9, 1e-6):
                    for sg in ((1.0,) if e == 0.0 else (1.0, -1.0)):
                        os_.append(o)
                        ds.append(_unit(c + r * (1.0 + sg * e) * p - o))
        nsurf = max(3, int(12 * scale))
        for n in _sphere_dirs(rng, nsurf):
            for k in (0.0, 0.5, 0.99, 1.0, 1.01, 2.0, -1.0, -1000.0):
                o = c + (r + k * 1e-4) * n
                for d in (n, -n, _sphere_dirs(rng, 1)[0], _unit(np.cross(n, [0.3, 0.5, 0.8]))):
                    os_.append(o)
                    ds.append(d)
        for o in c + 0.9 * r * rng.uniform(-0.5, 0.5, size=(nsurf, 3)):
            os_.append(o)
            ds.append(_sphere_dirs(rng, 1)[0])
    if not os_:
        return np.zeros((0, 3)), np.zeros((0, 3))
    return np.array(os_), np.array(ds)


def mesh_feature_rays(sc, rng, scale):
    """From random room origins aimed exactly at mesh vertices, edge midpoints (the cubes' face diagonals are
    triangle edges) and centroids, and at those targets moved by +-{1e-15, 1e-12, 1e-9} relative. Small meshes: every
    vertex, edge and triangle; large ones: `ntri` random triangles. Returns o, d, the mesh object aimed at and the
    target kind (0 vertex, 1 edge midpoint, 2 centroid; +4: a moved target)."""
    os_, ds, obj, kind = [], [], [], []
    for i, v, idx, mn, mx, _, _ in sc.meshes:
        if len(idx) <= 64:
            tri = idx
            edges = sorted({tuple(sorted((int(t[a]), int(t[b])))) for t in tri for a, b in ((0, 1), (1, 2), (0, 2))})
            tg = [(v[j], 0) for j in range(len(v))] + [((v[a] + v[b]) / 2, 1) for a, b in edges] + \
                 [(v[t].mean(0), 2) for t in tri]
            norig = max(1, int(round(4 * scale)))
        else:
            tri = idx[rng.choice(len(idx), size=max(200, int(2200 * scale)), replace=False)]
            tg = []
            for t in tri:
                tg += [(v[t[0]], 0), ((v[t[0]] + v[t[1]]) / 2, 1), (v[t].mean(0), 2)]
            norig = 1
        for p, kd in tg:
            for _ in range(norig):
                o = rng.uniform([2, 1, 1], [98, 80, 250])
                while np.all((o > mn - 1.0) & (o < mx + 1.0)):  # not from inside the mesh's box
                    o = rng.uniform([2, 1, 1], [98, 80, 250])
                os_.append(o); ds.append(_unit(p - o)); obj.append(i); kind.append(kd)
                if len(idx) > 64 and kd != int(rng.integers(3)):
                    continue  # large meshes: one moved target per triangle on average
                for e in (REL if len(idx) <= 64 else REL[int(rng.integers(3)):][:1]):
                    for sg in (1.0, -1.0):
                        os_.append(o); ds.append(_unit(p * (1.0 + sg * e) - o)); obj.append(i); kind.append(kd + 4)
    if not os_:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, np.int32)
    return np.array(os_), np.array(ds), np.array(obj, dtype=np.int32), np.array(kind, dtype=np.int32)


def root_tie_rays(sc, rng, scale):
    """Origins on one, two and all three of the planes through the centre of each mesh's root box (the octants'
    common corner, oracle.octants of the bbox), where pairs, quadruples and all eight of the octant-centre distances
    tie, and within {1e-15, 1e-12} relative of those planes; directions into the mesh."""
    os_, ds = [], []
    per = max(2, int(round(24 * scale)))
    for _, v, idx, mn, mx, _, _ in sc.meshes:
        c = oracle_bind.octants(mn, mx)[0][1]
        for ks in [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]:
            for e in (0.0, 1e-15, -1e-15, 1e-12, -1e-12):
                for _ in range(per if e == 0.0 else max(1, per // 3)):
                    o = rng.uniform([2, 1, 1], [98, 80, 200])
                    for k in ks:
                        o[k] = c[k] * (1.0 + e)
                    p = rng.uniform(mn, mx)
                    if np.linalg.norm(p - o) < 1e-3:
                        p = mx
                    os_.append(o)
                    ds.append(_unit(p - o))
    if not os_:
        return np.zeros((0, 3)), np.zeros((0, 3))
    return np.array(os_), np.array(ds)


# -------------------------------------------------------------------------------------------- segment families

def nee_segments(sc, origins, rng):
    """From the secondary family's origins to points uniform on the light sphere's surface."""
    _, c, r = sc.light
    return origins, c + r * _sphere_dirs(rng, len(origins))


def ladder_segments(o, d, t):
    """x = o, y = o + (t + delta) d for every delta of LADDER: shape (rays, deltas, 3) each."""
    dl = np.array(LADDER)
    y = o[:, None, :] + (t[:, None] + dl[None, :])[:, :, None] * d[:, None, :]
    return np.broadcast_to(o[:, None, :], y.shape).copy(), y


def plane_contact_segments(sc, rng, scale):
    """Endpoints exactly on a wall's coordinate (planes_clear's equality cases), on opposite sides of one wall, y
    outside the room, and segments 1e9 - 1, 1e9 + 1 and 2e9 long along a room diagonal (the dist < 1e9 guard)."""
    n = max(4, int(round(40 * scale)))
    xs, ys = [], []
    for k in range(3):
        for p, _ in sc.walls(k):
            a, b = rng.uniform(ROOM_LO, ROOM_HI, size=(n, 3)), rng.uniform(ROOM_LO, ROOM_HI, size=(n, 3))
            b1 = b.copy(); b1[:, k] = p
            xs.append(a); ys.append(b1)                      # y on the wall
            a1 = a.copy(); a1[:, k] = p
            xs.append(a1); ys.append(b)                      # x on the wall
            a2 = b.copy(); a2[:, k] = p                      # both on the wall
            a2[:, (k + 1) % 3] = a[:, (k + 1) % 3]
            xs.append(a1); ys.append(a2)
            out = 1.0 if p > 1.0 else -1.0                   # the side away from the room
            b2 = b.copy(); b2[:, k] = p + out * rng.uniform(1e-9, 30.0, n)
            xs.append(a); ys.append(b2)                      # opposite sides
            xs.append(b2); ys.append(a)
    a = rng.uniform(ROOM_LO, ROOM_HI, size=(n, 3))
    xs.append(a); ys.append(a + _sphere_dirs(rng, n) * rng.uniform(150, 600, (n, 1)))  # y outside the room
    for sg in itertools.product((1.0, -1.0), repeat=3):
        dg = _unit(np.array([98.0, 81.6, 200.0]) * np.array(sg))
        for L in (1e9 - 1.0, 1e9 + 1.0, 2e9):
            a = rng.uniform(ROOM_LO, ROOM_HI, size=(2, 3))
            xs.append(a); ys.append(a + L * dg)
    return np.vstack(xs), np.vstack(ys)


def box_segments(sc, rng, scale):
    """Segments that start outside a mesh's cull box (the root box united with the vertex bounds) and end
    BOX_STEPS before and after the point where their line enters it: the walks' root cull and the f32 cull at
    tmax = |y - x|."""
    n = max(6, int(round(120 * scale)))
    xs, ys = [], []
    for _, v, idx, mn, mx, lo, hi in sc.meshes:
        x = rng.uniform([2, 1, 1], [98, 80, 250], size=(4 * n, 3))
        x = x[np.any((x < lo - 1.0) | (x > hi + 1.0), axis=1)][:n]
        d = _unit(rng.uniform(lo, hi, size=(len(x), 3)) - x)
        with np.errstate(divide="ignore"):
            ta, tb = (lo - x) / d, (hi - x) / d
        t_in = np.minimum(ta, tb).max(axis=1)
        for st in BOX_STEPS:
            for sg in (-1.0, 1.0):
                xs.append(x)
                ys.append(x + (t_in + sg * st)[:, None] * d)
    if not xs:
        return np.zeros((0, 3)), np.zeros((0, 3))
    return np.vstack(xs), np.vstack(ys)


# ---------------------------------------------------------------------------------------------------- battery

class Battery:
    """rays[family] = (o, d); segs[family] = (x, y); meta: what the CPU test needs to check a family."""

    def __init__(self):
        self.rays, self.segs, self.meta = {}, {}, {}

    def all_rays(self):
        names = list(self.rays)
        o = np.vstack([self.rays[f][0] for f in names])
        d = np.vstack([self.rays[f][1] for f in names])
        fam = np.concatenate([np.full(len(self.rays[f][0]), k) for k, f in enumerate(names)])
        return o, d, fam, names

    def all_segs(self):
        names = list(self.segs)
        x = np.vstack([self.segs[f][0] for f in names])
        y = np.vstack([self.segs[f][1] for f in names])
        fam = np.concatenate([np.full(len(self.segs[f][0]), k) for k, f in enumerate(names)])
        return x, y, fam, names


def build(name, orc, scale=1.0):
    """The battery of scene `name` (a reference scene), hits taken from its OracleScene `orc`."""
    rng = np.random.default_rng([SEED, sum(name.encode())])
    sc = Scene(name, orc)
    b = Battery()
    b.scene = sc
    room = room_rays(int(5000 * scale), rng)
    b.rays["room"] = room
    b.rays["secondary"] = secondary_rays(sc, room, rng)
    o, d, want, tq, keys, all_keys = tie_rays(sc)
    b.rays["ties"] = (o, d)
    b.meta["ties"] = dict(want=want, t=tq, keys=keys, all_keys=all_keys)
    b.rays["axis"] = axis_rays(sc, rng, scale)
    if sc.spheres:
        b.rays["sphere_edges"] = sphere_edge_rays(sc, rng, scale)
    if sc.meshes:
        o, d, obj, kind = mesh_feature_rays(sc, rng, scale)
        b.rays["mesh_features"] = (o, d)
        b.meta["mesh_features"] = dict(obj=obj, kind=kind)
        b.rays["root_ties"] = root_tie_rays(sc, rng, scale)

    b.segs["nee"] = nee_segments(sc, b.rays["secondary"][0], rng)
    # the margin ladder: an equal share of every ray family's hits on spheres and meshes, and on planes
    o, d, fam, names = b.all_rays()
    t, ids, _, _ = orc.trace(o, d)
    curved = {i for i, _, _ in sc.spheres} | {m[0] for m in sc.meshes}
    plane = {i for i, _, _ in sc.planes}
    for label, objs, total in (("ladder", curved, int(700 * scale)), ("ladder_planes", plane, int(250 * scale))):
        pick = []
        for k in range(len(names)):
            c = np.flatnonzero((fam == k) & np.isin(ids, list(objs)) & (t > 1.5))  # (delta = -1 keeps x != y)
            share = max(4, total // len(names))
            pick.append(c[np.linspace(0, len(c) - 1, min(share, len(c))).astype(int)] if len(c) else c)
        pick = np.concatenate(pick)
        x, y = ladder_segments(o[pick], d[pick], t[pick])
        if label == "ladder":
            # The rungs' ray is (x, norm(y - x)), whose direction may differ from d in its last bits. A ray whose hit
            # does not survive that (it grazes a vertex or an edge, or another object comes first) proves nothing
            # about the margin: only rays whose every rung still has the ladder's own hit as its nearest (same
            # object, t within 1e-7: a thousandth of the 1e-4 between the rungs around the margin) stay in `ladder`;
            # the others are kept, for the comparison with the oracle, as `ladder_unstable`.
            t2, id2, _, _ = orc.trace(x.reshape(-1, 3), _unit(y - x).reshape(-1, 3))
            own = ((id2.reshape(x.shape[:2]) == ids[pick][:, None]) &
                   (np.abs(t2.reshape(x.shape[:2]) - t[pick][:, None]) <= 1e-7)).all(axis=1)
            if (~own).any():
                b.segs["ladder_unstable"] = (x[~own].reshape(-1, 3), y[~own].reshape(-1, 3))
            x, y, pick = x[own], y[own], pick[own]
        b.segs[label] = (x.reshape(-1, 3), y.reshape(-1, 3))
        b.meta[label] = dict(o=o[pick], d=d[pick], t=t[pick], obj=ids[pick], fam=fam[pick])
    b.segs["plane_contact"] = plane_contact_segments(sc, rng, scale)
    if sc.meshes:
        b.segs["mesh_box"] = box_segments(sc, rng, scale)
    return b


_CACHE = {}


def reference(name, orc, nearest=False):
    """The battery of `name` with the oracle's answers, built once per process and shared by the tests (read only):
    b.ref_rays = (o, d, family index, family names, t, obj, pos, nrm), b.ref_segs = (x, y, family index, family
    names, visible). nearest: `orc` is the scene's nearest-triangle oracle (mesh_nearest=True), brute force, so the
    unicorn's battery is a tenth of the size."""
    key = (name, bool(nearest))
    if key not in _CACHE:
        b = build(name, orc, 0.1 if nearest and name == "flying_unicorn" else 1.0)
        b.nearest = bool(nearest)
        o, d, fam, names = b.all_rays()
        b.ref_rays = (o, d, fam, names) + tuple(orc.trace(o, d))
        x, y, sfam, snames = b.all_segs()
        b.ref_segs = (x, y, sfam, snames, orc.visible(x, y))
        for a in b.ref_rays + b.ref_segs:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = b
    return _CACHE[key]
