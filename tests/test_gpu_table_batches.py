"""The compact tables read in batches (path_f64.h: AxisBatch, spheres_batched, closest_batched, shadow_batched)
against the CPU oracle on three scenes made for the batches' slots, none of which the reference scenes reach:

  full    4 axis planes on every axis and 4 spheres (one the light): 16 objects, every slot of every batch live, the
          object order scattered so that a slot's index is not its position;
  sparse  no plane on x, one on y, two on z and one sphere (the light): the n == 0 and n == 1 guards over batches
          whose other slots are the packer's zeros (a zero position or a zero sphere row used as an operand would
          put a wall through the origin or a point sphere there, and show as a hit the oracle does not have);
  twins   two planes at y = 81.6 with object indices 0 and 5 and different colours: the packer keeps one slot, whose
          index (now a lane of the batch) must be the lower one.

For each scene rt_diag_trace and rt_diag_visible run in the fused mesh-free form of the headline kernel
(RT_DIAG_FUSED_G0: k_megakernel_f64<8, 4>'s Cfg) on tests/query_rays.py's generators (room rays, rays from the
points they hit, axis-parallel and nearly axis-parallel rays, NEE segments to the light, segments touching the
planes), at most 4096 of each: t, object, position and normal bit-identical to the oracle, visibility equal. A scene
that did not pack as compact would have empty tables and miss every ray, so these tests also hold that the three
scenes are compact (tools/pack_dump.cpp prints `compact 1` for each). One 48x32 render at 16 spp per scene through
the megakernel holds tests/test_gpu_parity.py's tolerance (1e-9 on the subpixel means, RGB8 equal)."""
import os

import numpy as np
import pytest

import query_rays as qr

pytestmark = pytest.mark.gpu

SEED = 0x5EED
MAX_QUERIES = 4096


def _plane(axis, p, kd):
    pos, n = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    pos[axis] = p
    n[axis] = 1.0 if p < 50.0 else -1.0
    return (f'[[objects]]\nbrdf = {{ type = "diffuse", kd = {kd} }}\n'
            f'geometry = {{ type = "plane", pos = {pos}, n = {n} }}\n')


def _sphere(c, r, brdf):
    return f'[[objects]]\nbrdf = {brdf}\ngeometry = {{ type = "sphere", pos = {c}, r = {r} }}\n'


def _light(c, r):
    return ('[[objects]]\nemitted = [40.0, 40.0, 40.0]\nbrdf = { type = "diffuse", kd = [0.0, 0.0, 0.0] }\n'
            f'geometry = {{ type = "sphere", pos = {c}, r = {r} }}\n')


_DIFF = '{ type = "diffuse", kd = [0.8, 0.7, 0.3] }'
_DIFF2 = '{ type = "diffuse", kd = [0.3, 0.8, 0.6] }'
_MIRROR = '{ type = "specular", ks = [0.95, 0.95, 0.95] }'
_RED, _BLUE, _GREY, _GREEN = [0.75, 0.25, 0.25], [0.25, 0.25, 0.75], [0.75, 0.75, 0.75], [0.25, 0.75, 0.25]

# Planes at x = 1, 12, 88, 99, y = 0, 10, 70, 81.6, z = 0, 20, 180, 200: a middle cell with the camera, the light
# and most ray origins, inside a shell of cells whose rays end on the outer planes, so every plane is the nearest
# hit of some rays; the other spheres straddle planes of the middle cell. The objects come in no order of axis,
# position or kind.
FULL = ("[camera]\npos = [50.0, 44.0, 170.0]\ndir = [0.05, -0.1, -1.0]\n" +
        _plane(2, 200.0, _GREY) + _plane(0, 99.0, _BLUE) + _plane(1, 70.0, _GREY) +
        _sphere([88.0, 40.0, 95.0], 9.0, _MIRROR) + _plane(0, 1.0, _RED) + _plane(1, 0.0, _GREY) +
        _plane(2, 20.0, _GREEN) + _light([50.0, 52.0, 100.0], 4.0) + _plane(0, 88.0, _BLUE) +
        _plane(1, 81.6, _GREY) + _sphere([40.0, 10.0, 80.0], 8.0, _DIFF) + _plane(2, 0.0, _GREY) +
        _plane(0, 12.0, _RED) + _plane(1, 10.0, _GREEN) + _sphere([55.0, 38.0, 180.0], 7.0, _DIFF2) +
        _plane(2, 180.0, _GREY))

SPARSE = ("[camera]\npos = [50.0, 30.0, 190.0]\ndir = [0.0, -0.15, -1.0]\n" +
          _plane(2, 0.0, _GREY) + _plane(1, 0.0, _RED) + _light([50.0, 40.0, 100.0], 6.0) + _plane(2, 200.0, _BLUE))

TWINS = ("[camera]\npos = [50.0, 52.0, 195.0]\ndir = [0.0, -0.042612, -1.0]\n" +
         _plane(1, 81.6, _GREEN) + _plane(0, 1.0, _RED) + _plane(0, 99.0, _BLUE) + _plane(2, 0.0, _GREY) +
         _plane(1, 0.0, _GREY) + _plane(1, 81.6, _RED) + _sphere([27.0, 16.5, 47.0], 16.5, _DIFF) +
         _sphere([73.0, 16.5, 78.0], 16.5, _MIRROR) + _light([50.0, 70.0, 100.0], 4.0))

TEXTS = {"full": FULL, "sparse": SPARSE, "twins": TWINS}
NAMES = list(TEXTS)


class _Layout(qr.Scene):
    """What query_rays' generators read of a scene (its planes, spheres and light), from one of TEXTS."""

    def __init__(self, name, orc):
        import tomli

        self.name, self.orc = name, orc
        self.planes, self.spheres, self.meshes, self.light = [], [], [], None
        for i, o in enumerate(tomli.loads(TEXTS[name])["objects"]):
            g = o["geometry"]
            if g["type"] == "plane":
                k = int(np.argmax(np.abs(g["n"])))
                self.planes.append((i, k, float(g["pos"][k])))
            else:
                self.spheres.append((i, np.array(g["pos"], dtype=np.float64), float(g["r"])))
                if "emitted" in o:
                    self.light = self.spheres[-1]
        assert orc.light == self.light[0]


class _Ref:
    pass


_REF = {}


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("table_batches")
    for name, text in TEXTS.items():
        (d / f"{name}.toml").write_text(text)
    return str(d)


def _reference(name, oracle, scene_dir):
    """The scene's batteries with the oracle's answers and its render, made once and shared (read only)."""
    if name not in _REF:
        r = _Ref()
        r.path = os.path.join(scene_dir, f"{name}.toml")
        r.orc = oracle.OracleScene(r.path)
        sc = _Layout(name, r.orc)
        rng = np.random.default_rng([qr.SEED, sum(name.encode())])
        room = qr.room_rays(1200, rng)
        second = qr.secondary_rays(sc, room, rng)   # from the points the room rays hit: on planes and spheres
        axis = qr.axis_rays(sc, rng, 0.1)
        fams = [room, second, axis]
        r.names = ["room", "secondary", "axis"]
        r.o = np.vstack([f[0] for f in fams])[:MAX_QUERIES]
        r.d = np.vstack([f[1] for f in fams])[:MAX_QUERIES]
        r.fam = np.concatenate([np.full(len(f[0]), k) for k, f in enumerate(fams)])[:MAX_QUERIES]
        r.hits = r.orc.trace(r.o, r.d)
        nee = qr.nee_segments(sc, second[0], rng)
        contact = qr.plane_contact_segments(sc, rng, 0.1)
        r.snames = ["nee", "plane_contact"]
        r.x = np.vstack([nee[0], contact[0]])[:MAX_QUERIES]
        r.y = np.vstack([nee[1], contact[1]])[:MAX_QUERIES]
        r.sfam = np.concatenate([np.full(len(nee[0]), 0), np.full(len(contact[0]), 1)])[:MAX_QUERIES]
        r.vis = r.orc.visible(r.x, r.y)
        r.render = r.orc.render(48, 32, 16, SEED)
        _REF[name] = r
    return _REF[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _per_family(bad, fam, names):
    return {names[k]: int(np.count_nonzero(bad & (fam == k))) for k in range(len(names))}


@pytest.mark.parametrize("name", NAMES)
def test_trace_every_ray_bit_exact(name, rt, oracle, scene_dir):
    r = _reference(name, oracle, scene_dir)
    t_o, id_o, p_o, n_o = r.hits
    assert 1000 < len(r.o) <= MAX_QUERIES
    t, ids, prim, pos, nrm = rt.Scene.from_toml(r.path).diag_trace(r.o, r.d, form=rt.DIAG_FUSED_G0)
    hit = id_o >= 0
    bad = (ids != id_o) | (_bits(t) != _bits(t_o))
    bad |= hit & (np.any(_bits(pos) != _bits(p_o), axis=1) | np.any(_bits(nrm) != _bits(n_o), axis=1))
    print(f"{name}: {len(bad)} rays, {np.count_nonzero(hit)} hit, {np.count_nonzero(bad)} differ")
    i = np.flatnonzero(bad)[:4]
    assert not bad.any(), (f"{name}: {_per_family(bad, r.fam, r.names)} rays differ; first: o {r.o[i].tolist()} "
                           f"d {r.d[i].tolist()} device {ids[i].tolist()} {t[i].tolist()} oracle {id_o[i].tolist()} "
                           f"{t_o[i].tolist()}")
    # what the scene is for: every object is some ray's nearest hit (every slot's position and index were used)
    assert set(np.unique(id_o[hit])) == _objects_that_can_be_hit(name)


def _objects_that_can_be_hit(name):
    import tomli

    n = len(tomli.loads(TEXTS[name])["objects"])
    return set(range(n)) - ({5} if name == "twins" else set())  # the higher twin never wins a tie


@pytest.mark.parametrize("name", NAMES)
def test_visible_every_segment(name, rt, oracle, scene_dir):
    r = _reference(name, oracle, scene_dir)
    assert 500 < len(r.x) <= MAX_QUERIES
    vis, near = rt.Scene.from_toml(r.path).diag_visible(r.x, r.y, form=rt.DIAG_FUSED_G0)
    bad = vis != r.vis
    print(f"{name}: {len(bad)} segments, {np.count_nonzero(r.vis)} visible, {np.count_nonzero(bad)} differ")
    i = np.flatnonzero(bad)[:4]
    assert not bad.any(), (f"{name}: {_per_family(bad, r.sfam, r.snames)} segments differ; first: x {r.x[i].tolist()} "
                           f"y {r.y[i].tolist()} device {vis[i].tolist()} oracle {r.vis[i].tolist()}")
    assert not near.any()
    # both answers occur, so neither an always-clear nor an always-blocked query passes
    assert 0.05 < np.mean(r.vis) < 0.95


@pytest.mark.parametrize("name", NAMES)
def test_render_parity(name, rt, oracle, scene_dir):
    """tests/test_gpu_parity.py's _assert_parity on a 48x32 frame at 16 spp through the megakernel."""
    r = _reference(name, oracle, scene_dir)
    rgb_o, sub_o, st_o = r.render
    rgb_g, sub_g, st = rt.render(rt.Scene.from_toml(r.path), 48, 32, 16, SEED, megakernel=True, want_sub=True)
    assert st["samples"] == 48 * 32 * 4 * 4
    assert 0.9 * st_o["vertices"] <= st["vertices"] <= st_o["vertices"]
    rel = np.abs(sub_g - sub_o) / np.maximum(np.abs(sub_o), 1e-300)
    frac_sub = np.all((rel <= 1e-9) | (np.abs(sub_g - sub_o) <= 1e-15), axis=-1).mean()
    diff = np.abs(rgb_g.astype(int) - rgb_o.astype(int))
    same_px = np.all(diff == 0, axis=-1).mean()
    print(f"{name}: subpixels within 1e-9 {frac_sub:.5f}, RGB8-identical pixels {same_px:.5f}, "
          f"lit pixels {np.mean(rgb_o.max(axis=-1) > 0):.3f}")
    assert frac_sub >= 0.999, f"{name}: only {frac_sub:.5f} of subpixels within 1e-9"
    assert same_px >= 0.999, f"{name}: only {same_px:.5f} of pixels RGB8-identical"
    assert (~np.all(diff <= 1, axis=-1)).mean() <= 0.001
    assert np.mean(rgb_o.max(axis=-1) > 0) > 0.5  # a lit frame: the comparison is of paths, not of black
