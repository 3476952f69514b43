"""Pixel lists of mesh scenes through the pool kernels, the part that needs no GPU: the new entry points
and constants are exported, declared for Rust and mirrored in rt_amd; rt_render_pixels_path names the pool family each
shipped scene has; and rt_render_pixels_with rejects a family the scene lacks, an unknown family and every bad argument
rt_render_pixels rejects, before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, scene_path

NAMES = ("rt_render_pixels_path", "rt_render_pixels_with", "rt_render_pixels_with_device")
CONSTS = {"RT_LIST_AUTO": 0, "RT_LIST_FUSED": 1, "RT_LIST_FPOOL": 2, "RT_LIST_ROLES": 3}
INVAL, NODEVICE = -1, -6
U32 = ctypes.POINTER(ctypes.c_uint32)
U8 = ctypes.POINTER(ctypes.c_uint8)
D = ctypes.POINTER(ctypes.c_double)
W, H = 8, 6


@pytest.fixture(scope="module")
def scenes(rt):
    return {n: rt.Scene.from_toml(scene_path(n)) for n in ("cornell_box", "cubes", "flying_unicorn")}


def _is_inval(rt, rc, word=None):
    assert rc == INVAL, rc
    msg = rt.lib.rt_last_error()
    assert len(msg) > 0
    if word is not None:
        assert word in msg, msg


def _path(rt, scene, p, n):
    out = (ctypes.c_int32 * 2)(-7, -7)
    rc = rt.lib.rt_render_pixels_path(scene.handle if scene is not None else None,
                                      ctypes.byref(p) if p is not None else None, n, out)
    return rc, (out[0], out[1])


def test_exported_declared_and_mirrored(rt):
    header = open(os.path.join(REPO, "include", "rt_ffi.h")).read()
    rust = open(os.path.join(REPO, "ffi", "raytracer_ffi.rs")).read()
    diag = open(os.path.join(REPO, "include", "rt_diag.h")).read()
    for n in NAMES:
        assert hasattr(rt.lib, n), f"missing export {n}"
        assert re.search(rf"^int {n}\(", header, re.M), f"{n} not declared in rt_ffi.h"
        assert not re.search(rf"\b{n}\b", diag)
        assert re.search(rf"pub fn {n}\s*\(", rust), f"{n} not declared in raytracer_ffi.rs"
        assert n in rt._EXPORTS
        assert getattr(rt.lib, n).argtypes is not None
    for name, v in CONSTS.items():
        assert re.search(rf"^#define {name}\s+{v}\b", header, re.M), name
        assert re.search(rf"pub const {name}: i32 = {v};", rust), name
        assert getattr(rt, name[3:]) == v
    assert rt.lib.rt_abi_version() == 3
    assert callable(rt.render_pixels_path)
    assert rt.render_pixels.__defaults__[-1] == rt.LIST_AUTO  # render_pixels(..., path=LIST_AUTO)


@pytest.mark.parametrize("mis", (False, True))
@pytest.mark.parametrize("scene,pool", (("cornell_box", "LIST_FUSED"), ("cubes", "LIST_FPOOL"),
                                        ("flying_unicorn", "LIST_ROLES")))
def test_pool_family_of_the_shipped_scenes(rt, scenes, scene, pool, mis):
    """path_out[1] is the scene's pool whatever the list length; path_out[0] is it for the whole frame (whatever the
    threshold below which the automatic choice keeps the fused kernel), and either it or the fused kernel below."""
    want = getattr(rt, pool)
    for w, h in ((W, H), (1920, 1080)):
        for n in (1, 2, 17, w * h // 2, w * h):
            fam, has = rt.render_pixels_path(scenes[scene], w, h, 8, n, mis=mis)
            assert has == want, (scene, n)
            assert fam in (want, rt.LIST_FUSED)
        assert rt.render_pixels_path(scenes[scene], w, h, 8, w * h, mis=mis) == (want, want)
        # the choice is monotone in the list length: the pool from some length on
        fams = [rt.render_pixels_path(scenes[scene], w, h, 8, n, mis=mis)[0] for n in range(1, w * h + 1, max(1, w * h // 97))]
        first = fams.index(want)
        assert all(f == want for f in fams[first:])


def test_path_rejects_what_render_pixels_rejects(rt, scenes):
    good = rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL, 0, 1)
    for name, sc in scenes.items():
        for flag in (rt.FLAG_FP32, rt.FLAG_MESH_NEAREST):
            rc, out = _path(rt, sc, rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL | flag), 3)
            _is_inval(rt, rc, b"not supported")
            assert out == (-7, -7)
    sc = scenes["cubes"]
    _is_inval(rt, _path(rt, None, good, 3)[0])
    _is_inval(rt, _path(rt, sc, None, 3)[0])
    _is_inval(rt, rt.lib.rt_render_pixels_path(sc.handle, ctypes.byref(good), 3, None))
    for n in (-1, W * H + 1, 1 << 40):
        _is_inval(rt, _path(rt, sc, good, n)[0], b"n_pixels")
    for p in (rt.make_params(W, H, 8, 1, (0, 0, W, H - 1), rt.FLAG_MEGAKERNEL),
              rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL, row_step=2)):
        _is_inval(rt, _path(rt, sc, p, 3)[0])
    assert _path(rt, sc, good, 0)[0] == 0  # an empty list has a family too


def _cube_mesh(rt):
    """The first cube of the cubes scene, as rt_scene_create takes a mesh."""
    m = rt.Scene.from_toml(scene_path("cubes")).mesh(6)
    return dict(vertices=m["vertices"], indices=m["indices"], bbox_min=m["bbox"][:3], bbox_max=m["bbox"][3:],
                surface_area=m["surface_area"])


def test_a_phong_mesh_scene_has_no_pool(rt):
    """The same flat octree with and without a Phong object in the scene: the query pool's list instances cover the
    diffuse / mirror scenes only."""
    floor = dict(geom_kind=1, pos=[0.0, 0.0, 0.0], n=[0.0, 1.0, 0.0], brdf_kind=0, k=[0.7, 0.7, 0.7])
    phong = dict(geom_kind=1, pos=[0.0, 0.0, 0.0], n=[0.0, 0.0, -1.0], brdf_kind=2, phong_kd=0.6, phong_ks=0.3,
                 phong_power=10, color_d=[0.5, 0.25, 1.0], color_s=[1.0, 1.0, 0.5])
    wall = dict(phong, brdf_kind=0, k=[0.5, 0.5, 0.5])
    cube = dict(geom_kind=2, mesh=0, brdf_kind=0, k=[0.9, 0.9, 0.9])
    light = dict(geom_kind=0, pos=[50.0, 70.0, 100.0], r=4.0, brdf_kind=0, k=[0.0, 0.0, 0.0], emitted=[50.0, 50.0, 50.0])
    cam = ([50.0, 52.0, 295.6], [0.0, -0.042612, -1.0])
    plain = rt.Scene.from_desc(*cam, [floor, wall, cube, light], [_cube_mesh(rt)])
    shiny = rt.Scene.from_desc(*cam, [floor, phong, cube, light], [_cube_mesh(rt)])
    for mis in (False, True):
        assert rt.render_pixels_path(plain, W, H, 8, W * H, mis=mis) == (rt.LIST_FPOOL, rt.LIST_FPOOL)
        assert rt.render_pixels_path(shiny, W, H, 8, W * H, mis=mis) == (rt.LIST_FUSED, rt.LIST_FUSED)
    p = rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL, 0, 1)
    px = np.array([0, 5], dtype=np.uint32)
    for fam in (rt.LIST_FPOOL, rt.LIST_ROLES):
        _is_inval(rt, rt.lib.rt_render_pixels_with(shiny.handle, ctypes.byref(p), px.ctypes.data_as(U32), 2, fam, None,
                                                   None, None, None), b"kernel family")


def test_render_pixels_with_bad_arguments_are_inval(rt, scenes):
    """A family the scene lacks, a path outside 0 .. 3 and everything rt_render_pixels rejects: RT_E_INVAL before any
    device call (so also without a GPU); the device form checks everything but the list."""
    L = rt.lib
    good = rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL, 0, 1)
    px = np.array([0, 5, 47], dtype=np.uint32)
    sub = np.zeros((3, 4, 3))
    rgb = np.zeros((3, 3), dtype=np.uint8)

    def host(scene, p, ids, path):
        return L.rt_render_pixels_with(scene.handle if scene is not None else None,
                                       ctypes.byref(p) if p is not None else None,
                                       ids.ctypes.data_as(U32) if ids is not None else None,
                                       0 if ids is None else ids.size, path, rgb.ctypes.data_as(U8), sub.ctypes.data_as(D),
                                       None, None)

    def dev(scene, p, n, path, ptr=ctypes.c_void_p(16)):
        return L.rt_render_pixels_with_device(scene.handle if scene is not None else None,
                                              ctypes.byref(p) if p is not None else None, ptr, n, path, None,
                                              ctypes.c_void_p(16), None, None)

    lacks = (("flying_unicorn", rt.LIST_FPOOL), ("cubes", rt.LIST_ROLES), ("cornell_box", rt.LIST_FPOOL),
             ("cornell_box", rt.LIST_ROLES))
    for name, fam in lacks:
        _is_inval(rt, host(scenes[name], good, px, fam), b"kernel family")
        _is_inval(rt, dev(scenes[name], good, 3, fam), b"kernel family")
    for name, sc in scenes.items():
        for path in (-1, 4, 17, 1 << 30):
            _is_inval(rt, host(sc, good, px, path), b"kernel family")
            _is_inval(rt, dev(sc, good, 3, path), b"kernel family")
    # rt_render_pixels' own rules, with a family the scene has
    for name, fam in (("cubes", rt.LIST_FPOOL), ("flying_unicorn", rt.LIST_ROLES), ("cubes", rt.LIST_FUSED),
                      ("cornell_box", rt.LIST_AUTO)):
        sc = scenes[name]
        _is_inval(rt, host(None, good, px, fam))
        _is_inval(rt, host(sc, None, px, fam))
        _is_inval(rt, dev(None, good, 3, fam))
        _is_inval(rt, dev(sc, None, 3, fam))
        _is_inval(rt, dev(sc, good, 3, fam, ptr=None), b"null pixel list")
        _is_inval(rt, L.rt_render_pixels_with(sc.handle, ctypes.byref(good), None, 3, fam, None, None, None, None),
                  b"null pixel list")
        bad = [rt.make_params(W, H, 8, 1, (0, 0, W, H - 1), rt.FLAG_MEGAKERNEL),
               rt.make_params(W, H, 8, 1, (1, 0, W - 1, H), rt.FLAG_MEGAKERNEL),
               rt.make_params(2 * W, 2 * H, 8, 1, (0, 0, W, H), rt.FLAG_MEGAKERNEL),
               rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL, row_step=2),
               rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL, row_step=-1),
               rt.make_params(0, H, 8, 1, None, rt.FLAG_MEGAKERNEL),
               rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL | rt.FLAG_FP32),
               rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL | rt.FLAG_MESH_NEAREST)]
        for p in bad:
            _is_inval(rt, host(sc, p, px, fam))
            _is_inval(rt, dev(sc, p, 3, fam))
        for n in (-1, W * H + 1, 1 << 40):
            _is_inval(rt, dev(sc, good, n, fam), b"n_pixels")
        for ids, word in (((5, 3, 47), b"ascending"), ((3, 3), b"ascending"), ((0, W * H), b"outside"),
                          ((0xFFFFFFFF,), b"outside")):
            _is_inval(rt, host(sc, good, np.array(ids, dtype=np.uint32), fam), word)
        # an empty list is RT_OK without a launch; the outputs stay untouched
        sub[:] = 7.0
        assert host(sc, good, np.zeros(0, dtype=np.uint32), fam) == 0 and dev(sc, good, 0, fam) == 0
        assert np.all(sub == 7.0) and np.all(rgb == 0)


def test_valid_arguments_without_a_gpu_are_nodevice(rt, scenes):
    """Valid arguments on a host without a GPU: RT_E_NODEVICE (-6), like the rest of the ABI. (With a device the calls
    run; tests/test_gpu_render_pixels_pool.py checks what they compute.)"""
    if rt.device_count() > 0:
        rgb, sub, st = rt.render_pixels(scenes["cubes"], W, H, [], 8, want_sub=True, path=rt.LIST_FPOOL)
        assert rgb.shape == (0, 3) and sub.shape == (0, 4, 3) and st["samples"] == 0
        return
    good = rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL, 0, 1)
    px = np.array([0, 5, 47], dtype=np.uint32)
    sub = np.zeros((3, 4, 3))
    for name, fam in (("cubes", rt.LIST_FPOOL), ("flying_unicorn", rt.LIST_ROLES), ("cubes", rt.LIST_FUSED),
                      ("cubes", rt.LIST_AUTO), ("cornell_box", rt.LIST_FUSED)):
        h = scenes[name].handle
        rc = rt.lib.rt_render_pixels_with(h, ctypes.byref(good), px.ctypes.data_as(U32), 3, fam, None,
                                          sub.ctypes.data_as(D), None, None)
        assert rc == NODEVICE and b"no HIP device" in rt.lib.rt_last_error()
        rc = rt.lib.rt_render_pixels_with_device(h, ctypes.byref(good), ctypes.c_void_p(16), 3, fam, None,
                                                 ctypes.c_void_p(16), None, None)
        assert rc == NODEVICE
