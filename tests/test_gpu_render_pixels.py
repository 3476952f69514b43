"""The pixel-list render (rt_render_pixels; k_render_list_f64, the fused megakernel's body over a list) against rt_render:
for the same seed, spp and flags, entry e of its outputs is rt_render's sub_out and RGB8 of pixel pixels[e], bit for bit
and byte for byte. That equality is the kernel's specification."""
import ctypes

import numpy as np
import pytest
import torch  # before rt_amd loads, as bench.py: the process's HIP runtime is the one torch brings

import adapt_ref as dref
from conftest import scene_path

pytestmark = pytest.mark.gpu

W, H, SEED = 67, 35, 0xADA97
NPIX = W * H
# (scene, mis): cornell_box is analytic (k_megakernel_f64<8, 4> in rt_render), cubes takes the query-pool kernel in
# rt_render and the fused mesh instance here
CONFIGS = (("cornell_box", False), ("cornell_box", True), ("cubes", False))


def _lists():
    """A single pixel, the frame's first and last pixels, 63 / 64 / 65 / 257 entries (one wave of units is 16 pixels,
    one block 64: below, at and above a block, and several blocks), every pixel."""
    rng = np.random.default_rng(2024)
    out = [np.array([1234]), np.array([0, NPIX - 1])]
    for n in (63, 64, 65, 257):
        out.append(np.sort(rng.choice(NPIX, size=n, replace=False)))
    out.append(np.arange(NPIX))
    return [x.astype(np.uint32) for x in out]


LISTS = _lists()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def frames(rt, gpu_scenes):
    """rt_render's frames, rendered once per (scene, mis, spp) and left unchanged."""
    cache = {}

    def get(scene, mis, spp, w=W, h=H):
        key = (scene, mis, spp, w, h)
        if key not in cache:
            rgb, sub, _ = rt.render(gpu_scenes[scene], w, h, spp, SEED, mis=mis, megakernel=True, want_sub=True)
            cache[key] = (rgb, sub)
        return cache[key]

    return get


@pytest.mark.parametrize("spp", (4, 8, 36))
@pytest.mark.parametrize("scene,mis", CONFIGS)
def test_lists_equal_rt_render(rt, gpu_scenes, frames, scene, mis, spp):
    rgb_f, sub_f = frames(scene, mis, spp)
    assert rgb_f.max() > 50
    for ids in LISTS:
        rgb, sub, st = rt.render_pixels(gpu_scenes[scene], W, H, ids, spp, SEED, mis=mis, want_sub=True)
        assert not st["cancelled"] and st["samples"] == ids.size * 4 * (spp // 4)
        assert np.array_equal(_bits(sub), _bits(dref.gather(sub_f, ids))), (scene, mis, spp, ids.size)
        assert np.array_equal(rgb, dref.gather(rgb_f, ids))


@pytest.mark.parametrize("scene,mis", CONFIGS)
def test_256_spp_on_five_entries(rt, gpu_scenes, frames, scene, mis):
    """64 samples per subpixel: 20 units of one run each."""
    ids = np.array([7, 600, 1234, 1800, NPIX - 1], dtype=np.uint32)
    rgb_f, sub_f = frames(scene, mis, 256)
    rgb, sub, st = rt.render_pixels(gpu_scenes[scene], W, H, ids, 256, SEED, mis=mis, want_sub=True)
    assert st["samples"] == 5 * 256 and st["vertices"] > 0
    assert np.array_equal(_bits(sub), _bits(dref.gather(sub_f, ids))) and np.array_equal(rgb, dref.gather(rgb_f, ids))


def test_flying_unicorn(rt, gpu_scenes, frames):
    """A deep octree: rt_render takes the walk-pool kernel, the list render the fused mesh instance."""
    w, h = 24, 18
    ids = np.sort(np.random.default_rng(7).choice(w * h, size=40, replace=False)).astype(np.uint32)
    rgb_f, sub_f = frames("flying_unicorn", False, 8, w, h)
    rgb, sub, _ = rt.render_pixels(gpu_scenes["flying_unicorn"], w, h, ids, 8, SEED, want_sub=True)
    assert np.array_equal(_bits(sub), _bits(dref.gather(sub_f, ids))) and np.array_equal(rgb, dref.gather(rgb_f, ids))


# The fused list instance is the only list path of Phong scenes and of scenes of more than kMaxCompactObjects (16)
# objects: a 24x18 frame, lists of one pixel, 65 sorted random pixels and every pixel, at spp 8 and 36.
FW, FH = 24, 18


def _fused_lists():
    ids = np.sort(np.random.default_rng(11).choice(FW * FH, size=65, replace=False))
    return [x.astype(np.uint32) for x in (np.array([FW * 7 + 5]), ids, np.arange(FW * FH))]


_LIGHT = dict(geom_kind=0, pos=[50.0, 70.0, 100.0], r=4.0, brdf_kind=0, k=[0.0, 0.0, 0.0], emitted=[50.0, 50.0, 50.0])
_CAM = ([50.0, 52.0, 295.6], [0.0, -0.042612, -1.0])


def _phong_scene(rt):
    """A Phong floor and a Phong sphere before a diffuse wall, under a light: 4 objects (a compact scene)."""
    return rt.Scene.from_desc(*_CAM, [
        dict(geom_kind=1, pos=[0, 0, 0], n=[0, 1, 0], brdf_kind=2, phong_kd=0.5, phong_ks=0.3, phong_power=8,
             color_d=[0.7, 0.6, 0.5], color_s=[1, 1, 1]),
        dict(geom_kind=0, pos=[40, 15, 80], r=15, brdf_kind=2, phong_kd=0.2, phong_ks=0.7, phong_power=24,
             color_d=[0.9, 0.3, 0.3], color_s=[1, 1, 1]),
        dict(geom_kind=1, pos=[0, 0, 0], n=[0, 0, 1], brdf_kind=0, k=[0.75, 0.75, 0.75]), _LIGHT])


def _spheres_scene(rt):
    """A diffuse floor, 17 diffuse spheres and a light: 19 objects, past the compact tables."""
    objs = [dict(geom_kind=1, pos=[0, 0, 0], n=[0, 1, 0], brdf_kind=0, k=[0.75, 0.75, 0.75])]
    for i in range(17):
        objs.append(dict(geom_kind=0, pos=[10.0 + 5.0 * i, 6.0 + 3.0 * (i % 4), 60.0 + 7.0 * (i % 5)], r=4.0 + (i % 3),
                         brdf_kind=0, k=[0.3 + 0.04 * i, 0.6, 0.9 - 0.04 * i]))
    return rt.Scene.from_desc(*_CAM, objs + [_LIGHT])


def _phong_chair(rt, tmp_path):
    """The Phong chair of test_gpu_parity.py's split-tail test: a deep octree over a Phong floor."""
    from test_host_prep import extra_asset_scene

    p = extra_asset_scene(tmp_path, "chair.obj")
    text = open(p).read()
    floor = '{ type = "diffuse", kd = [0.75, 0.75, 0.75] }\ngeometry = { type = "plane", pos = [0.0, 0.0, 0.0]'
    assert floor in text
    text = text.replace(floor, floor.replace('{ type = "diffuse", kd = [0.75, 0.75, 0.75] }',
                                             '{ type = "phong", kd = 0.5, ks = 0.3, power = 8, color_d = [0.7, 0.6, '
                                             '0.5], color_s = [1.0, 1.0, 1.0] }'))
    open(p, "w").write(text)
    return rt.Scene.from_toml(p)


@pytest.mark.parametrize("kind,mis", (("phong", False), ("phong", True), ("spheres", False), ("spheres", True),
                                      ("phong_chair", True)))
def test_fused_only_scenes_equal_rt_render(rt, tmp_path, kind, mis):
    """Cfg F = 10 / 14 (Phong, compact), 0 / 4 (17 spheres: not compact) and 15 (the Phong chair with MIS, whose frame
    runs the role pool): the list's sub and RGB8 against rt_render's, bit for bit and byte for byte."""
    if kind == "phong_chair":
        sc = _phong_chair(rt, tmp_path)
        assert rt.render_pixels_path(sc, FW, FH, 8, FW * FH, mis=True)[1] == rt.LIST_FUSED
    else:
        sc = _phong_scene(rt) if kind == "phong" else _spheres_scene(rt)
    for spp in (8, 36):
        rgb_f, sub_f, _ = rt.render(sc, FW, FH, spp, SEED, mis=mis, megakernel=True, want_sub=True)
        assert rgb_f.max() > 50
        for ids in _fused_lists():
            rgb, sub, st = rt.render_pixels(sc, FW, FH, ids, spp, SEED, mis=mis, want_sub=True)
            assert st["samples"] == ids.size * 4 * (spp // 4)
            assert np.array_equal(_bits(sub), _bits(dref.gather(sub_f, ids))), (kind, mis, spp, ids.size)
            assert np.array_equal(rgb, dref.gather(rgb_f, ids))


def test_outputs_are_optional_and_spp_rounds_down(rt, gpu_scenes, frames):
    ids = LISTS[3]
    rgb_f, sub_f = frames("cornell_box", False, 8)
    sc = gpu_scenes["cornell_box"]
    rgb, sub, st = rt.render_pixels(sc, W, H, ids, 11, SEED, want_sub=False)  # 4 floor(11 / 4) = 8 samples
    assert sub is None and st["samples"] == ids.size * 8 and np.array_equal(rgb, dref.gather(rgb_f, ids))
    rgb, sub, _ = rt.render_pixels(sc, W, H, ids, 8, SEED, want_sub=True, want_rgb=False)
    assert rgb is None and np.array_equal(_bits(sub), _bits(dref.gather(sub_f, ids)))
    rgb, sub, st = rt.render_pixels(sc, W, H, ids, 3, SEED, want_sub=True)  # spp < 4 renders black, as rt_render
    assert st["samples"] == 0 and not rgb.any() and not sub.any()


def test_device_form_equals_host_form(rt, gpu_scenes, frames):
    ids = LISTS[5]
    rgb_f, sub_f = frames("cornell_box", False, 8)
    d_ids = torch.from_numpy(ids.astype(np.int32)).to("cuda")  # the same 32 bits
    d_sub = torch.zeros((ids.size, 4, 3), dtype=torch.float64, device="cuda")
    d_rgb = torch.zeros((ids.size, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = rt.make_params(W, H, 8, SEED, None, rt.FLAG_MEGAKERNEL, 0, 1)
    st = rt.RenderStats()
    rt._check(rt.lib.rt_render_pixels_device(gpu_scenes["cornell_box"].handle, ctypes.byref(p),
                                             ctypes.c_void_p(d_ids.data_ptr()), ids.size,
                                             ctypes.c_void_p(d_rgb.data_ptr()), ctypes.c_void_p(d_sub.data_ptr()), None,
                                             ctypes.byref(st)))
    assert st.samples == ids.size * 8
    assert np.array_equal(_bits(d_sub.cpu().numpy()), _bits(dref.gather(sub_f, ids)))
    assert np.array_equal(d_rgb.cpu().numpy(), dref.gather(rgb_f, ids))


def test_empty_list_leaves_outputs_untouched(rt, gpu_scenes):
    sub = np.full((2, 4, 3), 7.0)
    rgb = np.full((2, 3), 9, dtype=np.uint8)
    p = rt.make_params(W, H, 8, SEED, None, rt.FLAG_MEGAKERNEL, 0, 1)
    ids = np.zeros(1, dtype=np.uint32)
    rc = rt.lib.rt_render_pixels(gpu_scenes["cornell_box"].handle, ctypes.byref(p),
                                 ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 0,
                                 rgb.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                 sub.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None)
    assert rc == 0 and np.all(sub == 7.0) and np.all(rgb == 9)


def test_one_pixel_against_the_oracle(rt, gpu_scenes, oracle_scenes):
    """The oracle's sample_pixel path for one list pixel: subpixel means within 1e-9 (relative; the forward walk sums in
    another association than the recursion), the same RGB8."""
    col, row, spp = 29, 21, 16
    ids = np.array([row * W + col], dtype=np.uint32)
    rgb, sub, _ = rt.render_pixels(gpu_scenes["cornell_box"], W, H, ids, spp, SEED, want_sub=True)
    rgb_o, sub_o, _ = oracle_scenes["cornell_box"].render(W, H, spp, SEED, tile=(col, row, 1, 1), threads=1)
    err = np.abs(sub[0] - sub_o[0, 0])
    print("largest relative difference", float((err / np.maximum(np.abs(sub_o[0, 0]), 1e-300)).max()))
    assert sub_o.max() > 0 and np.all((err <= 1e-9 * np.abs(sub_o[0, 0])) | (err <= 1e-15))
    assert np.array_equal(rgb[0], rgb_o[0, 0])


def test_raised_cancel_word(rt, gpu_scenes):
    rgb, sub, st = rt.render_pixels(gpu_scenes["cornell_box"], W, H, LISTS[6], 64, SEED, want_sub=True,
                                    cancel=ctypes.c_int32(1))
    assert st["cancelled"]
