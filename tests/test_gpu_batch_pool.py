"""Batched error-target passes of mesh scenes through the pool kernels (the passes instances of the
flat-octree query pool and of the role-split pool) against rt_render_pixels. The specification is §17's: unit-group
off[e] + i of the outputs is rt_render_pixels' sub_out and RGB8 of pixel pixels[e] for the seed seeds[i] and the same
spp and flags, bit for bit and byte for byte, whichever kernel family runs the units.

Measured on the MI355X (this file, printed by the tests): the largest relative difference of a unit's subpixel means
from the oracle's, cubes 3.2e-16 and flying_unicorn 3.4e-16 (bound 1e-9); the 256-spp lists of five entries split 16
(cubes) and 32 (flying_unicorn) subpixels into chunks of 32 samples."""
import ctypes

import numpy as np
import pytest
import torch  # before rt_amd loads, as bench.py: the process's HIP runtime is the one torch brings

import batch_ref as br
from test_gpu_render_pixels_pool import FPOOL_BLOCK, ROLE_PATHS, mirror_cubes  # noqa: F401  (block shapes from the code)

pytestmark = pytest.mark.gpu

W, H = 67, 35
NPIX = W * H
UW, UH = 24, 18  # the unicorn's frame
SEEDS = [0xB0071 + 1013 * i * i + (i << 41) for i in range(16)]
V = ctypes.c_void_p


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _total(npix, total, cmax, rng):
    """Random ascending pixels with counts cycling 1 .. cmax, trimmed so that they add up to `total` unit-groups."""
    counts = []
    while sum(counts) < total:
        counts.append(min(len(counts) % cmax + 1, total - sum(counts)))
    ids = np.sort(rng.choice(npix, size=len(counts), replace=False))
    return ids, counts, cmax


def _np(lists):
    return [(np.asarray(i, dtype=np.uint32), np.asarray(c, dtype=np.uint8), s) for i, c, s in lists]


def _one16(npix):
    return ([npix // 2 + 3], [16], 16)


def _ends(npix):
    return ([0, npix - 1], [3, 1], 3)


def _once(npix):
    return (np.arange(npix), [1] * npix, 1)


def _cube_lists():
    """(ids, counts, n_seeds) in DESIGN.md §16's order of risk: every pixel once; unit totals around a wave's 64 and
    around one 1024-thread block's 256 unit-groups; then several passes per pixel: first and last, every 4th pixel
    with counts cycling 1 .. 5, one pixel with 16."""
    rng = np.random.default_rng(2026)
    blk = FPOOL_BLOCK // 4
    every4 = np.arange(0, NPIX, 4)
    out = [_once(NPIX)]
    out += [_total(NPIX, t, 3, rng) for t in (63, 64, 65, blk - 1, blk, blk + 1)]
    out += [_ends(NPIX), (every4, [i % 5 + 1 for i in range(every4.size)], 16), _one16(NPIX)]
    return _np(out)


def _mirror_lists():
    rng = np.random.default_rng(9)
    return _np([_once(NPIX)] + [_total(NPIX, t, 3, rng) for t in (63, 64, 65)])


def _unicorn_lists():
    rng = np.random.default_rng(7)
    n = UW * UH
    blk = ROLE_PATHS // 4  # one block's 784 path slots
    ids40 = np.sort(rng.choice(n, size=40, replace=False))
    out = [_once(n)]
    out += [_total(n, t, 3, rng) for t in (blk - 1, blk, blk + 1)]
    out += [_ends(n), (ids40, [i % 3 + 1 for i in range(40)], 3), _one16(n)]
    return _np(out)


CUBE_LISTS = _cube_lists()
MIRROR_LISTS = _mirror_lists()
UNICORN_LISTS = _unicorn_lists()
FIVE = (np.array([7, 600, 1234, 1800, NPIX - 1], dtype=np.uint32), np.array([3, 1, 2, 1, 1], dtype=np.uint8))
UFIVE = (np.array([3, 100, 211, 300, UW * UH - 1], dtype=np.uint32), np.array([3, 1, 2, 1, 1], dtype=np.uint8))


def test_lists_straddle_the_block_shapes():
    assert FPOOL_BLOCK == 1024 and ROLE_PATHS == 784
    assert [int(c.sum()) for _, c, _ in CUBE_LISTS[1:7]] == [63, 64, 65, 255, 256, 257]
    assert [int(c.sum()) for _, c, _ in UNICORN_LISTS[1:4]] == [195, 196, 197]
    assert int(CUBE_LISTS[-1][1][0]) == 16 and int(UNICORN_LISTS[-1][1][0]) == 16


@pytest.fixture(scope="module")
def refs(rt, gpu_scenes, mirror_cubes):  # noqa: F811
    """rt_render_pixels of every pixel for seeds[i], rendered once per (scene, mis, spp, i) and left unchanged."""
    cache = {}
    scenes = dict(gpu_scenes, cubes_mirror=mirror_cubes)

    def get(scene, w, h, mis, spp, i):
        key = (scene, w, h, mis, spp, i)
        if key not in cache:
            rgb, sub, _ = rt.render_pixels(scenes[scene], w, h, np.arange(w * h, dtype=np.uint32), spp, SEEDS[i], mis=mis,
                                           want_sub=True)
            rgb.setflags(write=False)
            sub.setflags(write=False)
            cache[key] = (rgb, sub)
        return cache[key]

    get.scenes = scenes
    return get


def _check_units(rgb, sub, refs, scene, w, h, mis, spp, ids, counts, label):
    off = br.offsets(counts)
    for i in range(int(counts.max())):
        has = counts > i
        r_rgb, r_sub = refs(scene, w, h, mis, spp, i)
        assert np.array_equal(_bits(sub[off[has] + i]), _bits(r_sub[ids[has]])), (label, i)
        assert np.array_equal(rgb[off[has] + i], r_rgb[ids[has]]), (label, i)


def _check_lists(rt, refs, scene, w, h, mis, spp, lists, pool):
    sc = refs.scenes[scene]
    assert rt.render_pixels_path(sc, w, h, spp, w * h, mis=mis)[1] == pool
    assert refs(scene, w, h, mis, spp, 0)[0].max() > 50
    assert not _same(refs(scene, w, h, mis, spp, 0)[1], refs(scene, w, h, mis, spp, 1)[1])
    for ids, counts, n_seeds in lists:
        units = int(counts.astype(np.int64).sum())
        assert units <= w * h and counts.max() <= n_seeds
        for fam in (pool, rt.LIST_FUSED):
            rgb, sub, st = rt.render_pixel_passes(sc, w, h, ids, counts, spp, SEEDS[:n_seeds], mis=mis, want_sub=True,
                                                  path=fam)
            assert not st["cancelled"] and st["samples"] == units * 4 * (spp // 4) and st["vertices"] > 0
            assert sub.shape == (units, 4, 3) and rgb.shape == (units, 3)
            _check_units(rgb, sub, refs, scene, w, h, mis, spp, ids, counts, (scene, mis, spp, ids.size, units, fam))


@pytest.mark.parametrize("spp", (4, 8, 36))
@pytest.mark.parametrize("mis", (False, True))
def test_cubes_through_the_query_pool(rt, refs, mis, spp):
    _check_lists(rt, refs, "cubes", W, H, mis, spp, CUBE_LISTS, rt.LIST_FPOOL)


def test_cubes_with_a_mirror_through_the_query_pool(rt, refs):
    """The mirror-capable instance (F = 9, 256-thread blocks)."""
    _check_lists(rt, refs, "cubes_mirror", W, H, False, 8, MIRROR_LISTS, rt.LIST_FPOOL)
    assert not np.array_equal(refs("cubes_mirror", W, H, False, 8, 0)[0], refs("cubes", W, H, False, 8, 0)[0])
    ids, counts, n_seeds = MIRROR_LISTS[1]
    with pytest.raises(rt.RtError):
        rt.render_pixel_passes(refs.scenes["cubes_mirror"], W, H, ids, counts, 8, SEEDS[:n_seeds], path=rt.LIST_ROLES)


def test_flying_unicorn_through_the_role_pool(rt, refs):
    _check_lists(rt, refs, "flying_unicorn", UW, UH, False, 8, UNICORN_LISTS, rt.LIST_ROLES)


def test_flying_unicorn_with_mis_through_the_role_pool(rt, refs):
    _check_lists(rt, refs, "flying_unicorn", UW, UH, True, 8, (UNICORN_LISTS[5],), rt.LIST_ROLES)


@pytest.mark.parametrize("scene,w,h,five,pool", (("cubes", W, H, FIVE, "LIST_FPOOL"),
                                                 ("flying_unicorn", UW, UH, UFIVE, "LIST_ROLES")))
def test_split_tail_of_a_short_list(rt, refs, scene, w, h, five, pool):
    """256 spp on five entries with counts (3, 1, 2, 1, 1): 32 units of 64 samples, fewer than one block's lanes. The
    pool splits them into chunks of samples across lanes (rt_debug_last_split; a split unit's chunks share its id, so
    its pixel and its seed), the fused kernel does not, and both give rt_render_pixels' bits."""
    sc = refs.scenes[scene]
    ids, counts = five
    rt.render(sc, w, h, 4, 1, megakernel=True)  # a frame without a split: no stale plan
    assert rt.debug_last_split()["split"] == 0
    rgb, sub, st = rt.render_pixel_passes(sc, w, h, ids, counts, 256, SEEDS[:3], want_sub=True, path=getattr(rt, pool))
    plan = rt.debug_last_split()
    print(scene, "split", plan)
    assert plan["split"] > 0
    assert st["samples"] == 8 * 256 and st["vertices"] > 0
    _check_units(rgb, sub, refs, scene, w, h, False, 256, ids, counts, (scene, pool))
    rgb, sub, _ = rt.render_pixel_passes(sc, w, h, ids, counts, 256, SEEDS[:3], want_sub=True, path=rt.LIST_FUSED)
    assert rt.debug_last_split()["split"] == 0
    _check_units(rgb, sub, refs, scene, w, h, False, 256, ids, counts, (scene, "fused"))


@pytest.mark.parametrize("scene,w,h,five", (("cubes", W, H, FIVE), ("flying_unicorn", UW, UH, UFIVE),
                                            ("cubes_mirror", W, H, FIVE)))
def test_auto_takes_the_family_the_path_call_names(rt, refs, scene, w, h, five):
    """rt_render_pixel_passes without a family: the scene's pool (rt_render_pixels_path answers for passes too), seen in
    the split it plans at 256 spp, and rt_render_pixels' bits."""
    sc = refs.scenes[scene]
    ids, counts = five
    fam, pool = rt.render_pixels_path(sc, w, h, 256, int(counts.sum()))
    assert fam == pool and pool in (rt.LIST_FPOOL, rt.LIST_ROLES)
    rt.render(sc, w, h, 4, 1, megakernel=True)
    assert rt.debug_last_split()["split"] == 0
    rgb, sub, _ = rt.render_pixel_passes(sc, w, h, ids, counts, 256, SEEDS[:3], want_sub=True)
    auto = rt.debug_last_split()
    assert auto["split"] > 0  # a pool kernel ran: k_render_passes_f64 plans no split
    r2, s2, _ = rt.render_pixel_passes(sc, w, h, ids, counts, 256, SEEDS[:3], want_sub=True, path=fam)
    assert rt.debug_last_split() == auto
    assert _same(sub, s2) and np.array_equal(rgb, r2)
    _check_units(rgb, sub, refs, scene, w, h, False, 256, ids, counts, (scene, "auto"))


@pytest.mark.parametrize("scene,w,h,col,row,pool", (("cubes", W, H, 20, 24, "LIST_FPOOL"),
                                                    ("flying_unicorn", UW, UH, 9, 8, "LIST_ROLES")))
def test_one_unit_against_the_oracle(rt, gpu_scenes, oracle_scenes, scene, w, h, col, row, pool):
    """The oracle's sample_pixel path for the third pass of one pixel on a mesh, with that pass's seed: subpixel means
    within 1e-9 (relative; the forward walk sums in another association than the recursion), the same RGB8."""
    spp, i = 16, 2
    ids = np.array([row * w + col], dtype=np.uint32)
    rgb, sub, _ = rt.render_pixel_passes(gpu_scenes[scene], w, h, ids, [3], spp, SEEDS[:3], want_sub=True,
                                         path=getattr(rt, pool))
    rgb_o, sub_o, _ = oracle_scenes[scene].render(w, h, spp, SEEDS[i], tile=(col, row, 1, 1), threads=1)
    err = np.abs(sub[i] - sub_o[0, 0])
    print("largest relative difference", float((err / np.maximum(np.abs(sub_o[0, 0]), 1e-300)).max()))
    assert sub_o.max() > 0 and np.all((err <= 1e-9 * np.abs(sub_o[0, 0])) | (err <= 1e-15))
    assert np.array_equal(rgb[i], rgb_o[0, 0])
    assert not _same(sub[0], sub[i])  # another seed, another unit


def test_outputs_are_optional_and_spp_rounds_down(rt, refs):
    ids, counts, n_seeds = CUBE_LISTS[2]
    units = int(counts.sum())
    sc = refs.scenes["cubes"]
    rgb, sub, st = rt.render_pixel_passes(sc, W, H, ids, counts, 11, SEEDS[:n_seeds], want_sub=False, path=rt.LIST_FPOOL)
    assert sub is None and st["samples"] == units * 8  # 4 floor(11 / 4) = 8
    r2, s2, _ = rt.render_pixel_passes(sc, W, H, ids, counts, 8, SEEDS[:n_seeds], want_sub=True, want_rgb=False,
                                       path=rt.LIST_FPOOL)
    assert r2 is None
    _check_units(rgb, s2, refs, "cubes", W, H, False, 8, ids, counts, "optional outputs")
    rgb, sub, st = rt.render_pixel_passes(sc, W, H, ids, counts, 3, SEEDS[:n_seeds], want_sub=True, path=rt.LIST_FPOOL)
    assert st["samples"] == 0 and not rgb.any() and not sub.any()  # spp < 4 renders black
    uids, ucounts, un = UNICORN_LISTS[5]
    rgb, sub, st = rt.render_pixel_passes(refs.scenes["flying_unicorn"], UW, UH, uids, ucounts, 3, SEEDS[:un], want_sub=True,
                                          path=rt.LIST_ROLES)
    assert st["samples"] == 0 and not rgb.any() and not sub.any()


@pytest.mark.parametrize("scene,w,h,lists,k,pool", (("cubes", W, H, CUBE_LISTS, 8, "LIST_FPOOL"),
                                                    ("flying_unicorn", UW, UH, UNICORN_LISTS, 5, "LIST_ROLES")))
def test_device_form_equals_host_form(rt, refs, scene, w, h, lists, k, pool):
    ids, counts, n_seeds = lists[k]
    units = int(counts.astype(np.int64).sum())
    sc = refs.scenes[scene]
    d_ids = torch.from_numpy(ids.astype(np.int32)).to("cuda")  # the same 32 bits
    d_cnt = torch.from_numpy(counts).to("cuda")
    d_sub = torch.zeros((units, 4, 3), dtype=torch.float64, device="cuda")
    d_rgb = torch.zeros((units, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = rt.make_params(w, h, 8, 0, None, rt.FLAG_MEGAKERNEL, 0, 1)
    sd = np.array(SEEDS[:n_seeds], dtype=np.uint64)
    for fam in (getattr(rt, pool), rt.LIST_AUTO):
        st = rt.RenderStats()
        d_sub.zero_()
        d_rgb.zero_()
        torch.cuda.synchronize()
        rt._check(rt.lib.rt_render_pixel_passes_with_device(sc.handle, ctypes.byref(p), V(d_ids.data_ptr()),
                                                            V(d_cnt.data_ptr()), ids.size, units,
                                                            sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n_seeds,
                                                            fam, V(d_rgb.data_ptr()), V(d_sub.data_ptr()), None,
                                                            ctypes.byref(st)))
        assert st.samples == units * 8 and st.vertices > 0
        _check_units(d_rgb.cpu().numpy(), d_sub.cpu().numpy(), refs, scene, w, h, False, 8, ids, counts, (scene, fam))


@pytest.mark.parametrize("scene,w,h,pool", (("cubes", W, H, "LIST_FPOOL"), ("flying_unicorn", UW, UH, "LIST_ROLES")))
def test_raised_cancel_word(rt, gpu_scenes, scene, w, h, pool):
    npix = w * h
    rgb, sub, st = rt.render_pixel_passes(gpu_scenes[scene], w, h, np.arange(npix, dtype=np.uint32), [1] * npix, 64,
                                          SEEDS[:1], want_sub=True, cancel=ctypes.c_int32(1), path=getattr(rt, pool))
    assert st["cancelled"]


@pytest.mark.parametrize("name", ("cubes", "flying_unicorn"))
def test_add_passes_is_the_pass_by_pass_loop(rt, gpu_scenes, name):
    """After two full passes, add_passes with mixed counts (now through the scene's pool) against
    `for i: add_pixels({e : counts[e] > i}, seeds[i])` on a second accumulator: sub, var and the counts are
    bit-identical, and pixels outside the list keep their bits."""
    sc = gpu_scenes[name]
    w, h = UW, UH
    npix = w * h
    rng = np.random.default_rng(31)
    ids = np.sort(rng.choice(npix, size=npix // 4, replace=False)).astype(np.uint32)
    counts = rng.integers(1, 6, size=ids.size).astype(np.uint8)
    counts[0], counts[-1] = 5, 1
    seeds = SEEDS[3:8]
    assert rt.render_pixels_path(sc, w, h, 8, ids.size)[0] in (rt.LIST_FPOOL, rt.LIST_ROLES)
    with rt.Accumulator(w, h) as a, rt.Accumulator(w, h) as b:
        for acc in (a, b):
            acc.add(sc, 8, 11)
            acc.add(sc, 8, 12)
        before = a.resolve(want_var=True)
        st = a.add_passes(sc, ids, counts, 8, seeds)
        assert not st["cancelled"] and st["samples"] == int(counts.astype(np.int64).sum()) * 8
        for i in range(5):
            b.add_pixels(sc, ids[counts > i], 8, seeds[i])
        ka, na = a.counts()
        kb, nb = b.counts()
        assert np.array_equal(ka, kb) and np.array_equal(na, nb)
        assert np.array_equal(ka.reshape(-1)[ids], 2 + counts)
        ra, rb = a.resolve(want_var=True), b.resolve(want_var=True)
        assert _same(ra[0], rb[0]) and _same(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
        outside = np.ones(npix, dtype=bool)
        outside[ids] = False
        outside = outside.reshape(h, w)
        assert outside.any() and _same(ra[0][outside], before[0][outside])
        assert not _same(ra[0], before[0])


def test_add_passes_takes_the_pool(rt, gpu_scenes):
    """rt_accum_add_passes follows RT_LIST_AUTO: at 256 spp the cubes' units plan the query pool's split tail."""
    sc = gpu_scenes["cubes"]
    ids, counts = FIVE
    with rt.Accumulator(W, H) as a:
        a.add(sc, 8, 11)
        a.add(sc, 8, 12)
        rt.render(sc, W, H, 4, 1, megakernel=True)
        assert rt.debug_last_split()["split"] == 0
        st = a.add_passes(sc, ids, counts, 256, SEEDS[:3])
        assert rt.debug_last_split()["split"] > 0 and st["samples"] == 8 * 256


def test_refine_is_plan_then_add_passes(rt, gpu_scenes):
    """rt_accum_refine on the cubes: the plan's lists stay on the device and run the pool; a second accumulator gets the
    host plan and add_passes. Same counts, same bits."""
    w, h, spp = 48, 36, 4
    sc = gpu_scenes["cubes"]
    seeds = SEEDS[:8]
    with rt.Accumulator(w, h) as a, rt.Accumulator(w, h) as b:
        for acc in (a, b):
            acc.add(sc, 8, 21)
            acc.add(sc, 8, 22)
        lo, hi = 0.0, 1.0
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if b.select(mid, 0.0, 0, cap=0)[1] > w * h // 4 else (lo, mid)
        abs_tol = hi
        for gain, max_n in ((1.0, 0), (0.5, 7)):
            ids, counts, info = b.plan(abs_tol, 0.0, max_n, spp // 4, gain, len(seeds))
            assert info["pixels"] > 0 and info["units"] <= w * h
            st = a.refine(sc, spp, seeds, abs_tol, 0.0, max_n, gain)
            assert not st["cancelled"] and st["refine"] == (info["pixels"], info["units"], info["passes"])
            assert st["samples"] == info["units"] * spp
            b.add_passes(sc, ids, counts, spp, seeds)
            ka, na = a.counts()
            kb, nb = b.counts()
            assert np.array_equal(ka, kb) and np.array_equal(na, nb)
            ra, rb = a.resolve(want_var=True), b.resolve(want_var=True)
            assert _same(ra[0], rb[0]) and _same(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
