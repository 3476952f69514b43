"""Pixel lists of mesh scenes through the pool kernels (the list instances of the flat-octree query pool
and of the role-split pool) against rt_render. The specification is §13's: for the same seed, spp and flags, entry e of
the outputs is rt_render's sub_out and RGB8 of pixel pixels[e], bit for bit and byte for byte, whichever kernel family
runs the list."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch  # before rt_amd loads, as bench.py: the process's HIP runtime is the one torch brings

import adapt_ref as dref
from conftest import REPO, scene_path

pytestmark = pytest.mark.gpu

W, H, SEED = 67, 35, 0xADA97
NPIX = W * H
UW, UH = 24, 18  # the unicorn's frame
KERNELS = os.path.join(REPO, "raytracer-server_amd", "csrc", "kernels")


def _define(src, name):
    """The integer a kernel source gives `#define name` (sums and differences of integers and earlier defines; a
    diagnostic-only term counts 0, as in the product build)."""
    text = open(os.path.join(KERNELS, src)).read()
    m = re.findall(rf"^#define {name} (.+?)(?://.*)?$", text, re.M)
    expr = m[-1].strip().strip("()")  # the last one is the product build's (#else branch)
    total, sign = 0, 1
    for tok in re.findall(r"[+-]|\w+", expr):
        if tok in "+-":
            sign = 1 if tok == "+" else -1
        else:
            total += sign * (int(tok) if tok.isdigit() else _define(src, tok))
    return total


# one block's worth of units, in pixels: the 1024-thread query pool of a scene without a mirror (cubes), and the path
# slots of a role-split block
FPOOL_BLOCK = _define("render_flat_f64.hip", "RT_FPOOL_BLOCK")
ROLE_PATHS = _define("render_mesh_f64.hip", "RT_ROLES_PATHS")


def test_block_shapes_read_from_the_code():
    assert FPOOL_BLOCK == 1024 and ROLE_PATHS == 784  # the lists below straddle 256 and 196 entries


def _some(rng, npix, n):
    return np.sort(rng.choice(npix, size=n, replace=False)).astype(np.uint32)


def _cube_lists():
    """One pixel; the first and last pixels; 63 / 64 / 65 / 257 entries; one block's worth of units, one pixel fewer and
    one more; every pixel."""
    rng = np.random.default_rng(2025)
    out = [np.array([1234], dtype=np.uint32), np.array([0, NPIX - 1], dtype=np.uint32)]
    out += [_some(rng, NPIX, n) for n in (63, 64, 65, 257, FPOOL_BLOCK // 4 - 1, FPOOL_BLOCK // 4, FPOOL_BLOCK // 4 + 1)]
    out.append(np.arange(NPIX, dtype=np.uint32))
    return out


def _unicorn_lists():
    rng = np.random.default_rng(7)
    n = UW * UH
    out = [np.array([211], dtype=np.uint32), np.array([0, n - 1], dtype=np.uint32), _some(rng, n, 40)]
    out += [_some(rng, n, k) for k in (ROLE_PATHS // 4 - 1, ROLE_PATHS // 4, ROLE_PATHS // 4 + 1)]
    out.append(np.arange(n, dtype=np.uint32))
    return out


CUBE_LISTS = _cube_lists()
UNICORN_LISTS = _unicorn_lists()
FIVE = np.array([7, 600, 1234, 1800, NPIX - 1], dtype=np.uint32)
UFIVE = np.array([3, 100, 211, 300, UW * UH - 1], dtype=np.uint32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def mirror_cubes(rt, tmp_path_factory):
    """The cubes and one mirror sphere: the query pool's mirror-capable instance (F = 9, 256-thread blocks)."""
    p = tmp_path_factory.mktemp("scenes") / "cubes_mirror.toml"
    p.write_text(open(scene_path("cubes")).read() + '\n[[objects]]\nbrdf = { type = "specular", ks = [0.999, 0.999, 0.999] }\n'
                 'geometry = { type = "sphere", pos = [40.0, 45.0, 60.0], r = 9.0 }\n')
    return rt.Scene.from_toml(str(p))


@pytest.fixture(scope="module")
def frames(rt, gpu_scenes, mirror_cubes):
    """rt_render's frames, rendered once per (scene, mis, spp) and left unchanged."""
    cache = {}
    scenes = dict(gpu_scenes, cubes_mirror=mirror_cubes)

    def get(scene, mis, spp, w=W, h=H):
        key = (scene, mis, spp, w, h)
        if key not in cache:
            rgb, sub, _ = rt.render(scenes[scene], w, h, spp, SEED, mis=mis, megakernel=True, want_sub=True)
            rgb.setflags(write=False)
            sub.setflags(write=False)
            cache[key] = (rgb, sub)
        return cache[key]

    get.scenes = scenes
    return get


def _check_lists(rt, frames, scene, w, h, mis, spp, lists, pool):
    rgb_f, sub_f = frames(scene, mis, spp, w, h)
    assert rgb_f.max() > 50
    sc = frames.scenes[scene]
    assert rt.render_pixels_path(sc, w, h, spp, w * h, mis=mis)[1] == pool
    for ids in lists:
        want_sub, want_rgb = dref.gather(sub_f, ids), dref.gather(rgb_f, ids)
        for fam in (pool, rt.LIST_FUSED):
            rgb, sub, st = rt.render_pixels(sc, w, h, ids, spp, SEED, mis=mis, want_sub=True, path=fam)
            assert not st["cancelled"] and st["samples"] == ids.size * 4 * (spp // 4) and st["vertices"] > 0
            assert np.array_equal(_bits(sub), _bits(want_sub)), (scene, mis, spp, ids.size, fam)
            assert np.array_equal(rgb, want_rgb), (scene, mis, spp, ids.size, fam)


@pytest.mark.parametrize("spp", (4, 8, 36))
@pytest.mark.parametrize("mis", (False, True))
def test_cubes_through_the_query_pool(rt, frames, mis, spp):
    _check_lists(rt, frames, "cubes", W, H, mis, spp, CUBE_LISTS, rt.LIST_FPOOL)


def test_cubes_with_a_mirror_through_the_query_pool(rt, frames):
    sc = frames.scenes["cubes_mirror"]
    _check_lists(rt, frames, "cubes_mirror", W, H, False, 8, (CUBE_LISTS[4], CUBE_LISTS[-1]), rt.LIST_FPOOL)
    # the sphere is in view and mirrors: the frame differs from the plain cubes'
    assert not np.array_equal(frames("cubes_mirror", False, 8)[0], frames("cubes", False, 8)[0])
    with pytest.raises(rt.RtError):
        rt.render_pixels(sc, W, H, CUBE_LISTS[0], 8, SEED, path=rt.LIST_ROLES)


def test_flying_unicorn_through_the_role_pool(rt, frames):
    _check_lists(rt, frames, "flying_unicorn", UW, UH, False, 8, UNICORN_LISTS, rt.LIST_ROLES)


def test_flying_unicorn_with_mis_through_the_role_pool(rt, frames):
    _check_lists(rt, frames, "flying_unicorn", UW, UH, True, 8, (UNICORN_LISTS[2],), rt.LIST_ROLES)


@pytest.mark.parametrize("scene,w,h,ids,pool", (("cubes", W, H, FIVE, "LIST_FPOOL"),
                                                ("flying_unicorn", UW, UH, UFIVE, "LIST_ROLES")))
def test_split_tail_of_a_short_list(rt, frames, scene, w, h, ids, pool):
    """256 spp on five entries: 20 units of 64 samples, fewer than one block's lanes. The pool splits them into chunks
    of 32 samples across lanes (rt_debug_last_split), the fused kernel does not, and both give the frame's bits."""
    sc = frames.scenes[scene]
    rgb_f, sub_f = frames(scene, False, 256, w, h)
    want_sub, want_rgb = dref.gather(sub_f, ids), dref.gather(rgb_f, ids)
    rt.render(sc, w, h, 4, SEED, megakernel=True)  # a frame without a split: no stale plan
    assert rt.debug_last_split()["split"] == 0
    rgb, sub, st = rt.render_pixels(sc, w, h, ids, 256, SEED, want_sub=True, path=getattr(rt, pool))
    plan = rt.debug_last_split()
    print(scene, "split", plan)
    assert plan["split"] > 0 and plan["chunk"] == 32
    assert st["samples"] == 5 * 256 and st["vertices"] > 0
    assert np.array_equal(_bits(sub), _bits(want_sub)) and np.array_equal(rgb, want_rgb)
    rgb, sub, _ = rt.render_pixels(sc, w, h, ids, 256, SEED, want_sub=True, path=rt.LIST_FUSED)
    assert rt.debug_last_split()["split"] == 0
    assert np.array_equal(_bits(sub), _bits(want_sub)) and np.array_equal(rgb, want_rgb)


@pytest.mark.parametrize("scene,w,h", (("cubes", W, H), ("flying_unicorn", UW, UH), ("cubes_mirror", W, H)))
def test_auto_takes_the_family_the_path_call_names(rt, frames, scene, w, h):
    """rt_render_pixels at every pixel: the scene's pool (rt_render_pixels_path), seen in the split it plans at 256 spp,
    and the frame's bits."""
    sc = frames.scenes[scene]
    ids = np.arange(w * h, dtype=np.uint32)
    fam, pool = rt.render_pixels_path(sc, w, h, 256, ids.size)
    assert fam == pool and pool in (rt.LIST_FPOOL, rt.LIST_ROLES)
    rgb_f, sub_f = frames(scene, False, 256, w, h)
    rt.render(sc, w, h, 4, SEED, megakernel=True)
    rgb, sub, _ = rt.render_pixels(sc, w, h, ids, 256, SEED, want_sub=True)
    auto = rt.debug_last_split()
    assert auto["split"] > 0  # a pool kernel ran: k_render_list_f64 plans no split
    rt.render_pixels(sc, w, h, ids, 256, SEED, path=fam)
    assert rt.debug_last_split() == auto
    assert np.array_equal(_bits(sub), _bits(dref.gather(sub_f, ids))) and np.array_equal(rgb, dref.gather(rgb_f, ids))


@pytest.mark.parametrize("scene,w,h,col,row,pool", (("cubes", W, H, 20, 24, "LIST_FPOOL"),
                                                    ("flying_unicorn", UW, UH, 9, 8, "LIST_ROLES")))
def test_one_pixel_against_the_oracle(rt, gpu_scenes, oracle_scenes, scene, w, h, col, row, pool):
    """The oracle's sample_pixel path for one list pixel on a mesh: subpixel means within 1e-9 (relative; the forward walk
    sums in another association than the recursion), the same RGB8."""
    spp = 16
    ids = np.array([row * w + col], dtype=np.uint32)
    rgb, sub, _ = rt.render_pixels(gpu_scenes[scene], w, h, ids, spp, SEED, want_sub=True, path=getattr(rt, pool))
    rgb_o, sub_o, _ = oracle_scenes[scene].render(w, h, spp, SEED, tile=(col, row, 1, 1), threads=1)
    err = np.abs(sub[0] - sub_o[0, 0])
    print("largest relative difference", float((err / np.maximum(np.abs(sub_o[0, 0]), 1e-300)).max()))
    assert sub_o.max() > 0 and np.all((err <= 1e-9 * np.abs(sub_o[0, 0])) | (err <= 1e-15))
    assert np.array_equal(rgb[0], rgb_o[0, 0])


def test_outputs_are_optional_and_spp_rounds_down(rt, gpu_scenes, frames):
    ids = CUBE_LISTS[3]
    rgb_f, sub_f = frames("cubes", False, 8)
    sc = gpu_scenes["cubes"]
    rgb, sub, st = rt.render_pixels(sc, W, H, ids, 11, SEED, want_sub=False, path=rt.LIST_FPOOL)  # 4 floor(11 / 4) = 8
    assert sub is None and st["samples"] == ids.size * 8 and np.array_equal(rgb, dref.gather(rgb_f, ids))
    rgb, sub, _ = rt.render_pixels(sc, W, H, ids, 8, SEED, want_sub=True, want_rgb=False, path=rt.LIST_FPOOL)
    assert rgb is None and np.array_equal(_bits(sub), _bits(dref.gather(sub_f, ids)))
    rgb, sub, st = rt.render_pixels(sc, W, H, ids, 3, SEED, want_sub=True, path=rt.LIST_FPOOL)  # spp < 4 renders black
    assert st["samples"] == 0 and not rgb.any() and not sub.any()
    uids = UNICORN_LISTS[2]
    rgb, sub, st = rt.render_pixels(gpu_scenes["flying_unicorn"], UW, UH, uids, 3, SEED, want_sub=True, path=rt.LIST_ROLES)
    assert st["samples"] == 0 and not rgb.any() and not sub.any()


def test_device_form_equals_host_form(rt, gpu_scenes, frames):
    ids = UNICORN_LISTS[2]
    rgb_f, sub_f = frames("flying_unicorn", False, 8, UW, UH)
    d_ids = torch.from_numpy(ids.astype(np.int32)).to("cuda")  # the same 32 bits
    d_sub = torch.zeros((ids.size, 4, 3), dtype=torch.float64, device="cuda")
    d_rgb = torch.zeros((ids.size, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = rt.make_params(UW, UH, 8, SEED, None, rt.FLAG_MEGAKERNEL, 0, 1)
    st = rt.RenderStats()
    rt._check(rt.lib.rt_render_pixels_with_device(gpu_scenes["flying_unicorn"].handle, ctypes.byref(p),
                                                  ctypes.c_void_p(d_ids.data_ptr()), ids.size, rt.LIST_ROLES,
                                                  ctypes.c_void_p(d_rgb.data_ptr()), ctypes.c_void_p(d_sub.data_ptr()),
                                                  None, ctypes.byref(st)))
    assert st.samples == ids.size * 8 and st.vertices > 0
    assert np.array_equal(_bits(d_sub.cpu().numpy()), _bits(dref.gather(sub_f, ids)))
    assert np.array_equal(d_rgb.cpu().numpy(), dref.gather(rgb_f, ids))


@pytest.mark.parametrize("scene,w,h,pool", (("cubes", W, H, "LIST_FPOOL"), ("flying_unicorn", UW, UH, "LIST_ROLES")))
def test_raised_cancel_word(rt, gpu_scenes, scene, w, h, pool):
    rgb, sub, st = rt.render_pixels(gpu_scenes[scene], w, h, np.arange(w * h, dtype=np.uint32), 64, SEED, want_sub=True,
                                    cancel=ctypes.c_int32(1), path=getattr(rt, pool))
    assert st["cancelled"]


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_add_pixels_is_render_pixels_plus_add_sub_pixels(rt, gpu_scenes):
    """rt_accum_add_pixels goes through the same choice: with every pixel listed the automatic choice is the cubes' query
    pool, whatever the length rule."""
    sc = gpu_scenes["cubes"]
    ids = np.arange(NPIX, dtype=np.uint32)
    assert rt.render_pixels_path(sc, W, H, 256, ids.size) == (rt.LIST_FPOOL, rt.LIST_FPOOL)
    with rt.Accumulator(W, H) as a, rt.Accumulator(W, H) as b:
        for acc in (a, b):
            acc.add(sc, 8, 11)
            acc.add(sc, 8, 12)
        rt.render(sc, W, H, 4, SEED, megakernel=True)
        st = a.add_pixels(sc, ids, 256, 13)
        assert rt.debug_last_split()["split"] > 0  # the pool ran
        assert not st["cancelled"] and st["samples"] == ids.size * 256
        _, sub, _ = rt.render_pixels(sc, W, H, ids, 256, 13, want_sub=True)
        b.add_sub_pixels(ids, sub, 64)
        ka, na = a.counts()
        kb, nb = b.counts()
        assert np.array_equal(ka, kb) and np.array_equal(na, nb) and na.min() == 4 + 64
        ra, rb = a.resolve(want_var=True), b.resolve(want_var=True)
        assert _same(ra[0], rb[0]) and _same(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
