"""Scenes of many spheres, past the kernels' small-scene tables, as TOML text: the same file loads into rt_amd.Scene
and into the oracle (oracle_bind.OracleScene). Fixed seeds; every number is written with repr(), so both loaders read
the same doubles. Used by tests/test_object_bvh.py."""
import math
import os
import random

_DIFFUSE = 'brdf = {{ type = "diffuse", kd = [{}, {}, {}] }}'
_MIRROR = 'brdf = { type = "specular", ks = [0.95, 0.95, 0.95] }'
_PHONG = 'brdf = { type = "phong", kd = 0.4, ks = 0.4, power = 9, color_d = [0.8, 0.5, 0.3], color_s = [1.0, 1.0, 1.0] }'


def _f(x):
    return repr(float(x))


def _v(v):
    return "[" + ", ".join(_f(x) for x in v) + "]"


def _obj(brdf, geom, emitted=None):
    e = f"emitted = {_v(emitted)}\n" if emitted is not None else ""
    return f"[[objects]]\n{e}{brdf}\ngeometry = {geom}\n"


def sphere(pos, r, brdf=None, emitted=None):
    return _obj(brdf or _DIFFUSE.format(0.7, 0.7, 0.7), f'{{ type = "sphere", pos = {_v(pos)}, r = {_f(r)} }}', emitted)


def plane(pos, n, kd=(0.6, 0.6, 0.6)):
    return _obj(_DIFFUSE.format(*kd), f'{{ type = "plane", pos = {_v(pos)}, n = {_v(n)} }}')


def cube(pos, size, rotate_y=None):
    t = f"transforms = [ {{ rotate_y = {_f(rotate_y)} }} ]\n" if rotate_y is not None else ""
    return _obj(_DIFFUSE.format(0.8, 0.8, 0.8), f'{{ type = "cube", pos = {_v(pos)}, size = {_f(size)} }}') + t


def light(pos, r, power=30.0):
    return sphere(pos, r, _DIFFUSE.format(0.0, 0.0, 0.0), (power, power, power))


def camera(pos, direction):
    return f"[camera]\npos = {_v(pos)}\ndir = {_v(direction)}\n"


def _brdf(rng, i):
    if i % 7 == 3:
        return _MIRROR
    if i % 11 == 5:
        return _PHONG
    return _DIFFUSE.format(*(round(0.25 + 0.6 * rng.random(), 3) for _ in range(3)))


def grid_spheres(n, rng, centre, pitch=4.0):
    """n spheres on a jittered 3-D grid (about cubic, filled layer by layer) around `centre`; radii 0.4 to 0.65 of
    the pitch, so neighbours overlap. Returns [(pos, r)]."""
    side = max(1, math.ceil(n ** (1.0 / 3.0)))
    out = []
    for i in range(n):
        ix, iy, iz = i % side, (i // side) % side, i // (side * side)
        p = [centre[0] + (ix - (side - 1) / 2) * pitch + (rng.random() - 0.5) * pitch * 0.5,
             centre[1] + iy * pitch + (rng.random() - 0.5) * pitch * 0.5,
             centre[2] - iz * pitch + (rng.random() - 0.5) * pitch * 0.5]
        out.append((p, pitch * (0.4 + 0.25 * rng.random())))
    return out


def field(n, seed=1234):
    """A floor, a back wall, a sphere light and n grid spheres seen from outside the grid (a deeper, regular tree)."""
    rng = random.Random(seed)
    side = max(1, math.ceil(n ** (1.0 / 3.0)))
    ext = side * 4.0
    t = camera((0.0, ext * 0.6, ext * 1.6 + 12.0), (0.0, -0.2, -1.0))
    t += plane((0.0, -2.0, 0.0), (0.0, 1.0, 0.0))
    t += plane((0.0, 0.0, -ext - 10.0), (0.0, 0.0, 1.0), (0.5, 0.5, 0.7))
    t += light((0.0, ext + 14.0, ext * 0.5), 0.2 * ext + 2.0)
    for i, (p, r) in enumerate(grid_spheres(n, rng, (0.0, 1.0, 0.0))):
        t += sphere(p, r, _brdf(rng, i))
    return t


def crowd(inside=True, seed=77):
    """About 300 spheres over a floor and a back wall: a jittered grid with overlapping neighbours, two exact
    duplicates, concentric spheres, one sphere that encloses the `inside` camera and a block of the grid (with a second
    emitter in it, so its inside is lit), r = 1e-3 spheres far away, mirror and Phong spheres among the diffuse ones,
    and the light sphere in the middle of the object list. inside=False: the same objects seen from outside."""
    rng = random.Random(seed)
    t = camera((0.0, 8.0, 26.0), (0.0, -0.1, -1.0)) if inside else camera((3.0, 14.0, 64.0), (0.0, -0.12, -1.0))
    t += plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    t += plane((0.0, 0.0, -34.0), (0.0, 0.0, 1.0), (0.5, 0.5, 0.7))
    g = grid_spheres(275, rng, (0.0, 2.0, 8.0))
    for i, (p, r) in enumerate(g[:140]):
        t += sphere(p, r, _brdf(rng, i))
    t += light((0.0, 44.0, 10.0), 6.0)  # the light: the first emitter, in the middle of the list
    for i, (p, r) in enumerate(g[140:]):
        t += sphere(p, r, _brdf(rng, 140 + i))
    t += sphere(g[10][0], g[10][1], _DIFFUSE.format(0.2, 0.9, 0.2))  # exact duplicates of earlier spheres
    t += sphere(g[157][0], g[157][1], _MIRROR)
    for r in (3.0, 2.0, 1.0, 2.0):  # concentric (and one more duplicate)
        t += sphere((-18.0, 6.0, 20.0), r, _DIFFUSE.format(0.9, 0.4, 0.4))
    t += sphere((0.0, 8.0, 16.0), 17.0, _DIFFUSE.format(0.7, 0.7, 0.6))  # encloses the inside camera and a block
    t += sphere((4.0, 19.0, 18.0), 3.5, _DIFFUSE.format(0.0, 0.0, 0.0), (120.0, 120.0, 120.0))  # lights that inside
    for k in range(6):  # specks far from the origin
        a = 0.9 * k
        t += sphere((420.0 * math.cos(a), 35.0 + 11.0 * k, -380.0 * math.sin(a) - 200.0), 1e-3)
    return t


def edge(kind):
    """The smallest trees. "s5": five spheres and nothing else (two leaves); "s1p17": one sphere and 17 planes (the
    root is a leaf, a long rest list); "s4p13": four spheres and 13 planes."""
    t = camera((0.0, 4.0, 30.0), (0.0, -0.05, -1.0))
    if kind == "s5":
        t += light((0.0, 16.0, 4.0), 4.0)
        for k, x in enumerate((-9.0, -3.0, 3.5, 9.0)):
            t += sphere((x, 2.0 + k, -2.0 * k), 3.0 + 0.25 * k, _MIRROR if k == 2 else None)
        return t
    ns, npl = (1, 17) if kind == "s1p17" else (4, 13)
    room = [((0.0, -3.0, 0.0), (0.0, 1.0, 0.0)), ((0.0, 30.0, 0.0), (0.0, -1.0, 0.0)), ((-20.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
            ((20.0, 0.0, 0.0), (-1.0, 0.0, 0.0)), ((0.0, 0.0, -25.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, 40.0), (0.0, 0.0, -1.0))]
    for k in range(npl):
        if k < 3:
            p, n = room[k]
        elif k - 3 < npl - 6:  # slanted planes that cut the room's corners, between the room's own planes
            a = 0.55 * (k - 3) + 0.2
            n = (math.cos(a) * 0.8, -0.6 if k % 2 else 0.6, math.sin(a) * 0.8)
            p = tuple(-40.0 * c for c in n)
        else:
            p, n = room[3 + (k - 3 - (npl - 6))]
        t += plane(p, n, (0.4 + 0.03 * k, 0.7 - 0.02 * k, 0.5))
        if k == 1:
            t += light((0.0, 22.0, 0.0), 3.0)
    for k in range(ns - 1):
        t += sphere((-8.0 + 8.0 * k, 1.0 + k, -4.0 + 2.0 * k), 3.5, _MIRROR if k == 1 else None)
    return t


def mixed(seed=5):
    """A cube mesh, 20 spheres and three planes: not compact, with a mesh on the rest list."""
    rng = random.Random(seed)
    t = camera((0.0, 8.0, 34.0), (0.0, -0.15, -1.0))
    t += plane((0.0, -2.0, 0.0), (0.0, 1.0, 0.0))
    g = grid_spheres(19, rng, (0.0, 0.5, 2.0), 4.5)
    for i, (p, r) in enumerate(g[:8]):
        t += sphere(p, r, _brdf(rng, i))
    t += cube((9.0, 2.0, 8.0), 6.0, 0.4)
    t += light((-4.0, 26.0, 6.0), 4.0)
    t += plane((0.0, 0.0, -22.0), (0.0, 0.0, 1.0), (0.5, 0.5, 0.7))
    for i, (p, r) in enumerate(g[8:]):
        t += sphere(p, r, _brdf(rng, 8 + i))
    t += plane((-24.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.7, 0.4, 0.4))
    return t


SCENES = {"crowd": lambda: crowd(True), "crowd_out": lambda: crowd(False), "s5": lambda: edge("s5"),
          "s1p17": lambda: edge("s1p17"), "s4p13": lambda: edge("s4p13"), "mixed": mixed}


def write(directory, name):
    """Writes scene `name` (a key of SCENES, or "field<N>") into `directory` and returns the file's path."""
    text = field(int(name[5:])) if name.startswith("field") else SCENES[name]()
    p = os.path.join(str(directory), f"{name}.toml")
    with open(p, "w") as f:
        f.write(text)
    return p
