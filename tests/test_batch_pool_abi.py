"""Batched error-target passes of mesh scenes through the pool kernels, the part that needs no GPU: the
two new entry points are exported, declared for Rust and mirrored in rt_amd; rt_render_pixel_passes_with rejects an
unknown family, a family the scene lacks and every bad argument rt_render_pixel_passes rejects, before any device call;
and the code objects hold the passes instances of both pool kernels with the argument layout their bodies read in
place."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, scene_path
from test_kernarg_layout import _kernels

NAMES = ("rt_render_pixel_passes_with", "rt_render_pixel_passes_with_device")
PASSES_KERNELS = ("k_megakernel_fpool_passes_f64", "k_megakernel_roles_passes_f64", "k_render_passes_f64")
INVAL, NODEVICE = -1, -6
U8 = ctypes.POINTER(ctypes.c_uint8)
U32 = ctypes.POINTER(ctypes.c_uint32)
U64 = ctypes.POINTER(ctypes.c_uint64)
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


class Calls:
    """The two _with forms on a three-entry list of six units, every argument replaceable."""

    def __init__(self, rt):
        self.L = rt.lib
        self.good = rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL, 0, 1)
        self.px = np.array([0, 5, 47], dtype=np.uint32)
        self.ct = np.array([1, 3, 2], dtype=np.uint8)
        self.sd = np.arange(1, 17, dtype=np.uint64)
        self.sub = np.full((6, 4, 3), 7.0)
        self.rgb = np.zeros((6, 3), dtype=np.uint8)

    def host(self, scene, path, p="good", ids="px", counts="ct", seeds="sd", n_seeds=3, n=None):
        p = self.good if isinstance(p, str) else p
        ids = self.px if isinstance(ids, str) else ids
        counts = self.ct if isinstance(counts, str) else counts
        seeds = self.sd if isinstance(seeds, str) else seeds
        return self.L.rt_render_pixel_passes_with(
            scene.handle if scene is not None else None, ctypes.byref(p) if p is not None else None,
            ids.ctypes.data_as(U32) if ids is not None else None,
            counts.ctypes.data_as(U8) if counts is not None else None,
            (0 if ids is None else ids.size) if n is None else n,
            seeds.ctypes.data_as(U64) if seeds is not None else None, n_seeds, path,
            self.rgb.ctypes.data_as(U8), self.sub.ctypes.data_as(D), None, None)

    def dev(self, scene, path, p="good", n=3, units=6, ptr=ctypes.c_void_p(16), cptr=ctypes.c_void_p(32), seeds="sd",
            n_seeds=3):
        p = self.good if isinstance(p, str) else p
        seeds = self.sd if isinstance(seeds, str) else seeds
        return self.L.rt_render_pixel_passes_with_device(
            scene.handle if scene is not None else None, ctypes.byref(p) if p is not None else None, ptr, cptr, n, units,
            seeds.ctypes.data_as(U64) if seeds is not None else None, n_seeds, path, None, ctypes.c_void_p(64), None,
            None)


def test_exported_declared_and_mirrored(rt):
    header = open(os.path.join(REPO, "include", "rt_ffi.h")).read()
    rust = open(os.path.join(REPO, "ffi", "raytracer_ffi.rs")).read()
    diag = open(os.path.join(REPO, "include", "rt_diag.h")).read()
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for n in NAMES:
        assert hasattr(rt.lib, n), f"missing export {n}"
        assert re.search(rf"^int {n}\(", header, re.M), f"{n} not declared in rt_ffi.h"
        assert not re.search(rf"\b{n}\b", diag)
        assert re.search(rf"pub fn {n}\s*\(", rust), f"{n} not declared in raytracer_ffi.rs"
        assert n in rt._EXPORTS
        assert getattr(rt.lib, n).argtypes is not None
        assert n in text, f"{n} not in INTEGRATION.md"
    # the family argument sits behind n_seeds in both forms, in C and in Rust
    for n in NAMES:
        c = re.search(rf"^int {n}\((.*?)\);", header, re.M | re.S).group(1)
        r = re.search(rf"pub fn {n}\s*\((.*?)\)", rust, re.S).group(1)
        assert re.search(r"int32_t n_seeds,\s*int32_t path,", c), n
        assert re.search(r"n_seeds: i32,\s*path: i32,", r), n
    assert rt.lib.rt_abi_version() == 3  # additive
    assert rt.render_pixel_passes.__defaults__[-1] == rt.LIST_AUTO  # render_pixel_passes(..., path=LIST_AUTO)
    # the header no longer says that the pool kernels lack the instance, and names the family rule
    assert "the pool kernels have no such instance" not in header
    assert "rt_render_pixels_path answers for a batched render" in re.sub(r"\s*\n \*\s*", " ", header)


def test_the_batch_stays_opt_in(rt):
    """No default moved: the batch is asked for, for every scene."""
    import inspect

    sig = inspect.signature(rt.render_to_error).parameters
    assert sig["batch"].default == 0 and sig["gain"].default is None
    assert rt.ERROR_TARGET_BATCH_DEFAULTS == dict(batch=8, gain=1.0)


def test_an_unknown_family_is_inval(rt, scenes):
    c = Calls(rt)
    for sc in scenes.values():
        for path in (-1, 4, 17, 1 << 30, -(1 << 31)):
            _is_inval(rt, c.host(sc, path), b"kernel family")
            _is_inval(rt, c.dev(sc, path), b"kernel family")
    assert np.all(c.sub == 7.0) and np.all(c.rgb == 0)


def _cube_mesh(rt):
    m = rt.Scene.from_toml(scene_path("cubes")).mesh(6)
    return dict(vertices=m["vertices"], indices=m["indices"], bbox_min=m["bbox"][:3], bbox_max=m["bbox"][3:],
                surface_area=m["surface_area"])


def _phong_mesh_scene(rt):
    """A flat octree beside a Phong wall (tests/test_list_pool_abi.py's scene): no pool instance for lists or passes."""
    floor = dict(geom_kind=1, pos=[0.0, 0.0, 0.0], n=[0.0, 1.0, 0.0], brdf_kind=0, k=[0.7, 0.7, 0.7])
    phong = dict(geom_kind=1, pos=[0.0, 0.0, 0.0], n=[0.0, 0.0, -1.0], brdf_kind=2, phong_kd=0.6, phong_ks=0.3,
                 phong_power=10, color_d=[0.5, 0.25, 1.0], color_s=[1.0, 1.0, 0.5])
    cube = dict(geom_kind=2, mesh=0, brdf_kind=0, k=[0.9, 0.9, 0.9])
    light = dict(geom_kind=0, pos=[50.0, 70.0, 100.0], r=4.0, brdf_kind=0, k=[0.0, 0.0, 0.0], emitted=[50.0, 50.0, 50.0])
    return rt.Scene.from_desc([50.0, 52.0, 295.6], [0.0, -0.042612, -1.0], [floor, phong, cube, light], [_cube_mesh(rt)])


def test_a_family_the_scene_lacks_is_inval(rt, scenes):
    """RT_LIST_ROLES on the cubes, RT_LIST_FPOOL on the unicorn, either pool on cornell_box and on a Phong mesh scene:
    the rule is the pixel list's (rt_render_pixels_path's path_out[1] is the one pool a scene has)."""
    c = Calls(rt)
    shiny = _phong_mesh_scene(rt)
    assert rt.render_pixels_path(shiny, W, H, 8, 6) == (rt.LIST_FUSED, rt.LIST_FUSED)
    lacks = ((scenes["cubes"], rt.LIST_ROLES), (scenes["flying_unicorn"], rt.LIST_FPOOL),
             (scenes["cornell_box"], rt.LIST_FPOOL), (scenes["cornell_box"], rt.LIST_ROLES),
             (shiny, rt.LIST_FPOOL), (shiny, rt.LIST_ROLES))
    for sc, fam in lacks:
        for p in (c.good, rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL | rt.FLAG_MIS, 0, 1)):
            _is_inval(rt, c.host(sc, fam, p=p), b"kernel family")
            _is_inval(rt, c.dev(sc, fam, p=p), b"kernel family")
    assert np.all(c.sub == 7.0) and np.all(c.rgb == 0)


def test_render_pixel_passes_own_bad_arguments_through_the_with_forms(rt, scenes):
    """tests/test_batch_abi.py's cases of rt_render_pixel_passes, with a family the scene has."""
    c = Calls(rt)
    MK = rt.FLAG_MEGAKERNEL
    for name, fam in (("cubes", rt.LIST_FPOOL), ("flying_unicorn", rt.LIST_ROLES), ("cubes", rt.LIST_FUSED),
                      ("flying_unicorn", rt.LIST_AUTO), ("cornell_box", rt.LIST_FUSED), ("cornell_box", rt.LIST_AUTO)):
        sc = scenes[name]
        for f in (c.host, c.dev):
            _is_inval(rt, f(None, fam), b"null")
            _is_inval(rt, f(sc, fam, p=None), b"null")
            _is_inval(rt, f(sc, fam, seeds=None), b"null seeds")
            for ns in (0, 17, -1):
                _is_inval(rt, f(sc, fam, n_seeds=ns), b"n_seeds")
            for p in (rt.make_params(W, H, 8, 1, (0, 0, W, H - 1), MK), rt.make_params(W, H, 8, 1, (1, 0, W - 1, H), MK),
                      rt.make_params(2 * W, 2 * H, 8, 1, (0, 0, W, H), MK)):
                _is_inval(rt, f(sc, fam, p=p), b"whole frame")
            _is_inval(rt, f(sc, fam, p=rt.make_params(W, H, 8, 1, None, MK, row_step=2)))
            for flag in (rt.FLAG_FP32, rt.FLAG_MESH_NEAREST):
                _is_inval(rt, f(sc, fam, p=rt.make_params(W, H, 8, 1, None, MK | flag)), b"not supported")
        _is_inval(rt, c.host(sc, fam, ids=None, n=3), b"null pixel list")
        _is_inval(rt, c.host(sc, fam, counts=None), b"null count list")
        _is_inval(rt, c.dev(sc, fam, ptr=None), b"null pixel list")
        _is_inval(rt, c.dev(sc, fam, cptr=None), b"null count list")
        for counts in ([0, 1, 1], [1, 4, 1], [1, 1, 255]):
            _is_inval(rt, c.host(sc, fam, counts=np.array(counts, dtype=np.uint8)), b"count")
        _is_inval(rt, c.host(sc, fam, n_seeds=2), b"count")  # a count of 3 with two seeds
        for ids, word in (([5, 3, 47], b"ascending"), ([3, 3, 4], b"ascending"), ([0, 1, 48], b"outside")):
            _is_inval(rt, c.host(sc, fam, ids=np.array(ids, dtype=np.uint32)), word)
        small = rt.make_params(4, 3, 8, 1, None, MK, 0, 1)
        many = np.ones(12, dtype=np.uint8)
        many[3] = 2
        _is_inval(rt, c.host(sc, fam, p=small, ids=np.arange(12, dtype=np.uint32), counts=many, n_seeds=16), b"units")
        for units in (2, 10, 49):  # below n_pixels, above n_pixels * n_seeds, above the frame
            _is_inval(rt, c.dev(sc, fam, units=units, n_seeds=3 if units != 49 else 16, n=3 if units != 49 else 48),
                      b"units")
        # an empty list is RT_OK without a launch
        assert c.host(sc, fam, ids=np.zeros(0, dtype=np.uint32), counts=np.zeros(0, dtype=np.uint8)) == 0
        assert c.dev(sc, fam, n=0, units=0, ptr=None, cptr=None) == 0
    assert np.all(c.sub == 7.0) and np.all(c.rgb == 0)  # never written


def test_valid_arguments_without_a_gpu_are_nodevice(rt, scenes):
    """Valid arguments on a host without a GPU: RT_E_NODEVICE (-6), like the rest of the ABI. (With a device the calls
    run; tests/test_gpu_batch_pool.py checks what they compute.)"""
    if rt.device_count() > 0:
        rgb, sub, st = rt.render_pixel_passes(scenes["cubes"], W, H, [], [], 8, [1, 2], want_sub=True, path=rt.LIST_FPOOL)
        assert rgb.shape == (0, 3) and sub.shape == (0, 4, 3) and st["samples"] == 0
        return
    c = Calls(rt)
    mis = rt.make_params(W, H, 8, 1, None, rt.FLAG_MEGAKERNEL | rt.FLAG_MIS, 0, 1)
    for name, fam in (("cubes", rt.LIST_FPOOL), ("flying_unicorn", rt.LIST_ROLES), ("cubes", rt.LIST_FUSED),
                      ("flying_unicorn", rt.LIST_FUSED), ("cubes", rt.LIST_AUTO), ("flying_unicorn", rt.LIST_AUTO),
                      ("cornell_box", rt.LIST_FUSED), ("cornell_box", rt.LIST_AUTO)):
        for p in (c.good, mis):
            assert c.host(scenes[name], fam, p=p) == NODEVICE and b"no HIP device" in rt.lib.rt_last_error()
            assert c.dev(scenes[name], fam, p=p) == NODEVICE
    with pytest.raises(rt.RtError) as e:
        rt.render_pixel_passes(scenes["cubes"], W, H, [0, 5], [1, 2], 8, [11, 12], path=rt.LIST_FPOOL)
    assert e.value.code == NODEVICE
    with pytest.raises(rt.RtError) as e:
        rt.render_pixel_passes(scenes["cubes"], W, H, [0, 5], [1, 2], 8, [11, 12], path=rt.LIST_ROLES)
    assert e.value.code == INVAL


def test_passes_kernels_take_the_arguments_their_bodies_read_in_place(tmp_path):
    """The passes instances of the fused body and of both pool bodies are in lib/librtamd.so, and each takes a 248-byte
    DevScene at kernarg offset 0 and a 176-byte RenderArgs at offset 248 (megakernel_common.h karg_scene /
    karg_render_args): units and seeds trail the list instances' arguments."""
    ks = _kernels(tmp_path)
    for stem in PASSES_KERNELS:
        hits = {k: v for k, v in ks.items() if re.search(rf"\d{stem}I", k)}
        assert hits, f"no {stem} instance in the code objects"
        for name, args in hits.items():
            assert "NS_8DevSceneENS_10RenderArgsE" in name, f"{name}: (DevScene, RenderArgs) are not the first two parameters"
            assert args[0] == (0, 248), f"{name}: DevScene at {args[0]}"
            assert args[1] == (248, 176), f"{name}: RenderArgs at {args[1]}"
            # the two trailing explicit arguments are the 8-byte units and seeds pointers
            assert name.endswith("PKjPKm"), name
    # the instance set is the list instances': F = 41, 45 (1024 threads), 9, 13 (256) and the role pool's 9, 13
    def inst(stem):
        return sorted(re.search(rf"{stem}I(.*?)EEv", k).group(1) for k in ks if re.search(rf"\d{stem}I", k))

    assert inst("k_megakernel_fpool_passes_f64") == inst("k_megakernel_fpool_list_f64")
    assert inst("k_megakernel_roles_passes_f64") == inst("k_megakernel_roles_list_f64")
    assert len(inst("k_megakernel_fpool_passes_f64")) == 4 and len(inst("k_megakernel_roles_passes_f64")) == 2
