"""Batched error-target passes on the device: k_render_passes_f64 against rt_render_pixels unit by unit,
the run merge against the pass-by-pass loop, the plan against its numpy restatement (tests/batch_ref.py), all bit for
bit; rt_accum_refine against plan + add_passes; and the batched loop beside the sequential one on cornell_box."""
import ctypes

import numpy as np
import pytest
import torch  # before rt_amd loads, as bench.py: the process's HIP runtime is the one torch brings

import accum_ref as aref
import adapt_ref as dref
import batch_ref as br

pytestmark = pytest.mark.gpu

W, H = 67, 35
FW, FH = 24, 18
SEEDS = [0xBA7C4 + 977 * i * i + (i << 40) for i in range(16)]
V = ctypes.c_void_p


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _total(npix, total, cmax, rng):
    """Random ascending pixels with counts cycling 1 .. cmax, trimmed so that they add up to `total`."""
    counts = []
    while sum(counts) < total:
        counts.append(min(len(counts) % cmax + 1, total - sum(counts)))
    ids = np.sort(rng.choice(npix, size=len(counts), replace=False))
    return ids, counts


def _lists(npix):
    """(ids, counts, n_seeds): one pixel with 16 passes; the first and last pixels; every pixel once (one seed); every
    4th pixel with counts cycling 1 .. 5; unit totals of 63, 64, 65 and 257 (a block of the kernel holds 64
    unit-groups: below, at and above one block, and several blocks)."""
    rng = np.random.default_rng(2025 + npix)
    out = [([npix // 2 + 3], [16], 16), ([0, npix - 1], [3, 1], 3), (np.arange(npix), [1] * npix, 1)]
    every4 = np.arange(0, npix, 4)
    out.append((every4, [i % 5 + 1 for i in range(every4.size)], 16))
    for total in (63, 64, 65, 257):
        ids, counts = _total(npix, total, 3, rng)
        out.append((ids, counts, 3))
    return [(np.asarray(i, dtype=np.uint32), np.asarray(c, dtype=np.uint8), s) for i, c, s in out]


def _scene(rt, gpu_scenes, name):
    if name in gpu_scenes:
        return gpu_scenes[name]
    import test_gpu_render_pixels as trp

    return trp._phong_scene(rt) if name == "phong" else trp._spheres_scene(rt)


def _check_render(rt, sc, w, h, spp, mis):
    """Every unit-group of every list against rt_render_pixels of every pixel with that pass's seed."""
    npix = w * h
    every = np.arange(npix, dtype=np.uint32)
    ref = {}

    def of(i):
        if i not in ref:
            rgb, sub, _ = rt.render_pixels(sc, w, h, every, spp, SEEDS[i], mis=mis, want_sub=True)
            ref[i] = (rgb, sub)
        return ref[i]

    assert of(0)[0].max() > 50 and not _same(of(0)[1], of(1)[1])
    for ids, counts, n_seeds in _lists(npix):
        units = int(counts.astype(np.int64).sum())
        assert units <= npix and counts.max() <= n_seeds
        rgb, sub, st = rt.render_pixel_passes(sc, w, h, ids, counts, spp, SEEDS[:n_seeds], mis=mis, want_sub=True)
        assert not st["cancelled"] and st["samples"] == units * 4 * (spp // 4)
        assert sub.shape == (units, 4, 3) and rgb.shape == (units, 3)
        off = br.offsets(counts)
        for i in range(int(counts.max())):
            has = counts > i
            r_rgb, r_sub = of(i)
            assert np.array_equal(_bits(sub[off[has] + i]), _bits(r_sub[ids[has]])), (spp, mis, ids.size, units, i)
            assert np.array_equal(rgb[off[has] + i], r_rgb[ids[has]])


@pytest.mark.parametrize("spp", (4, 8, 36))
@pytest.mark.parametrize("mis", (False, True))
def test_units_equal_render_pixels_cornell(rt, gpu_scenes, mis, spp):
    _check_render(rt, gpu_scenes["cornell_box"], W, H, spp, mis)


@pytest.mark.parametrize("name", ("cubes", "phong", "spheres"))
def test_units_equal_render_pixels_small(rt, gpu_scenes, name):
    """The fused mesh instance (the cubes' own lists run the query pool), a Phong scene and a scene past the compact
    tables, 24 x 18 at spp 8."""
    _check_render(rt, _scene(rt, gpu_scenes, name), FW, FH, 8, False)


def test_device_form_and_optional_outputs(rt, gpu_scenes):
    sc = gpu_scenes["cornell_box"]
    ids, counts, n_seeds = _lists(W * H)[3]
    units = int(counts.astype(np.int64).sum())
    rgb, sub, _ = rt.render_pixel_passes(sc, W, H, ids, counts, 8, SEEDS[:n_seeds], want_sub=True)
    d_ids = torch.from_numpy(ids.astype(np.int32)).to("cuda")
    d_cnt = torch.from_numpy(counts).to("cuda")
    d_sub = torch.zeros(units * 12, dtype=torch.float64, device="cuda")
    d_rgb = torch.zeros(units * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = rt.make_params(W, H, 8, 0, None, rt.FLAG_MEGAKERNEL, 0, 1)
    sd = np.array(SEEDS[:n_seeds], dtype=np.uint64)
    st = rt.RenderStats()
    rt._check(rt.lib.rt_render_pixel_passes_device(sc.handle, ctypes.byref(p), V(d_ids.data_ptr()), V(d_cnt.data_ptr()),
                                                   ids.size, units, sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                   n_seeds, V(d_rgb.data_ptr()), V(d_sub.data_ptr()), None,
                                                   ctypes.byref(st)))
    assert st.samples == units * 8
    assert _same(d_sub.cpu().numpy().reshape(units, 4, 3), sub) and np.array_equal(d_rgb.cpu().numpy().reshape(units, 3), rgb)
    r2, s2, _ = rt.render_pixel_passes(sc, W, H, ids, counts, 8, SEEDS[:n_seeds], want_sub=False)
    assert s2 is None and np.array_equal(r2, rgb)
    r3, s3, st3 = rt.render_pixel_passes(sc, W, H, ids, counts, 3, SEEDS[:n_seeds], want_sub=True)  # spp < 4: black
    assert st3["samples"] == 0 and not r3.any() and not s3.any()


@pytest.mark.parametrize("name,w,h", (("cornell_box", W, H), ("cubes", FW, FH)))
def test_add_passes_is_the_pass_by_pass_loop(rt, gpu_scenes, name, w, h):
    """After two full passes, add_passes with mixed counts against `for i: add_pixels({e : counts[e] > i}, seeds[i])`
    on a second accumulator: sub, var and the counts are bit-identical, and pixels outside the list keep their bits."""
    sc = gpu_scenes[name]
    npix = w * h
    rng = np.random.default_rng(31)
    ids = np.sort(rng.choice(npix, size=npix // 4, replace=False)).astype(np.uint32)  # ~3 units each
    counts = rng.integers(1, 6, size=ids.size).astype(np.uint8)
    counts[0], counts[-1] = 5, 1
    seeds = SEEDS[3:8]
    with rt.Accumulator(w, h) as a, rt.Accumulator(w, h) as b:
        for acc in (a, b):
            acc.add(sc, 8, 11)
            acc.add(sc, 8, 12)
        before = a.resolve(want_var=True)
        with pytest.raises(rt.RtError):
            a.add_passes(sc, ids[::-1], counts, 8, seeds)  # not ascending
        st = a.add_passes(sc, ids, counts, 8, seeds)
        assert not st["cancelled"] and st["samples"] == int(counts.astype(np.int64).sum()) * 8
        for i in range(5):
            b.add_pixels(sc, ids[counts > i], 8, seeds[i])
        ka, na = a.counts()
        kb, nb = b.counts()
        assert np.array_equal(ka, kb) and np.array_equal(na, nb)
        assert np.array_equal(ka.reshape(-1)[ids], 2 + counts) and np.array_equal(na.reshape(-1)[ids], 4 + 2 * counts.astype(np.uint32))
        ra, rb = a.resolve(want_var=True), b.resolve(want_var=True)
        assert _same(ra[0], rb[0]) and _same(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
        outside = np.ones(npix, dtype=bool)
        outside[ids] = False
        outside = outside.reshape(h, w)
        assert outside.any() and _same(ra[0][outside], before[0][outside])
        assert not _same(ra[0], before[0])
        # a cancelled call merges nothing
        st = a.add_passes(sc, ids, counts, 8, seeds, cancel=ctypes.c_int32(1))
        assert st["cancelled"] and np.array_equal(a.counts()[1], na) and _same(a.resolve()[0], ra[0])


# The plan against tests/batch_ref.py on synthetic accumulators -----------------------------------------------

def _select_passes(width, height, dark, spread=0.2):
    """Two passes (n = 1 each) whose accumulated frame has the subpixel variance d^2 (d = 0.02 +- spread, per pixel)
    and the colour 0.1 + d at the dark pixels, 0.9 + d at the others (test_gpu_adapt.py's construction)."""
    rng = np.random.default_rng(17 + 1000 * width + height)
    d = 0.02 * rng.uniform(1.0 - spread, 1.0 + spread, size=(height, width, 1, 1))
    m1 = np.where(dark[:, :, None, None], 0.1, 0.9) + np.zeros((height, width, 4, 3))
    return m1, m1 + 2.0 * d


def _hot_passes(width, height):
    """Two passes (n = 1 each) of a mid-grey frame whose subpixel scatter is d = 0.01 everywhere but at the pixels
    with (col + 2 row) % 7 == 0, where it is 0.02 .. 0.14: a minority of pixels far above a target of 0.03, so the
    planned counts spread over 1 .. 9 and their total stays below a frame's worth (the cap leaves them alone)."""
    rng = np.random.default_rng(23 + 1000 * width + height)
    yy, xx = np.mgrid[0:height, 0:width]
    f = np.where((xx + 2 * yy) % 7 == 0, rng.uniform(2.0, 14.0, size=(height, width)), 1.0)[:, :, None, None]
    m1 = 0.5 + np.zeros((height, width, 4, 3))
    return m1, m1 + 2.0 * (0.01 * f)


@pytest.mark.parametrize("width,height", ((5, 3), (67, 35), (600, 450)))
def test_plan_counts_vary(rt, gpu_scenes, width, height):
    """Counts that survive the frame cap: x = gain (N_p g / thr^2 - N_p) / n decides, not C'."""
    m1, m2 = _hot_passes(width, height)
    want = dref.Accum(width, height)
    with rt.Accumulator(width, height) as acc:
        for a in (want, acc):
            a.add_sub(m1, 1)
            a.add_sub(m2, 1)
        for abs_tol, n, gain, C, distinct in ((0.03, 1, 1.0, 16, 4), (0.04, 1, 1.0, 16, 3), (0.03, 2, 0.5, 8, 2),
                                              (0.04, 1, 0.6, 4, 2)):
            ids, counts, info = _plan_agrees(acc, want, abs_tol, 0.0, 0, n, gain, C, (abs_tol, n, gain, C))
            assert len(np.unique(counts)) >= distinct and info["passes"] > 1 and info["units"] > info["pixels"]
            assert info["units"] <= width * height


def _plan_agrees(acc, want, abs_tol, rel_tol, max_n, n, gain, C, label):
    ids, counts, info = acc.plan(abs_tol, rel_tol, max_n, n, gain, C)
    e_ids, e_counts, e_units, e_passes = br.plan(want, abs_tol, rel_tol, max_n, n, gain, C)
    assert np.array_equal(ids, e_ids), (label, ids.size, e_ids.size)
    assert np.array_equal(counts, e_counts), label
    assert info == dict(pixels=int(e_ids.size), units=e_units, passes=e_passes), (label, info)
    assert np.array_equal(ids, dref.select(want, abs_tol, rel_tol, max_n))  # the selection's list
    return ids, counts, info


@pytest.mark.parametrize("width,height", ((1, 1), (5, 3), (67, 35), (600, 450)))
def test_plan_matches_restatement(rt, gpu_scenes, width, height):
    """None, all, a checkerboard and only the last pixel active; gains and pass sizes that spread the counts over
    1 .. C; thr = 0; max_n with and without per-pixel counts; a smaller cap."""
    npix = width * height
    big = npix > 100000  # 1055 blocks: the scan spans its 1024 threads' segments; fewer cases (the restatement's time)
    yy, xx = np.mgrid[0:height, 0:width]
    checker = (yy + xx) % 2 == 0
    last = np.zeros((height, width), dtype=bool)
    last[-1, -1] = True
    REL = 0.05
    for dark, name in ((checker, "checker"), (last, "last"))[:1 if big else 2]:
        m1, m2 = _select_passes(width, height, dark, 0.6)
        want = dref.Accum(width, height)
        with rt.Accumulator(width, height) as acc:
            for a in (want, acc):
                a.add_sub(m1, 1)
                a.add_sub(m2, 1)
            _, _, info = _plan_agrees(acc, want, 1.0, 0.0, 0, 4, 1.0, 16, "none")
            assert info == dict(pixels=0, units=0, passes=0)
            _, counts, info = _plan_agrees(acc, want, 0.0, 0.0, 0, 4, 0.5, 16, "all, thr = 0")
            assert info["pixels"] == npix and info["passes"] == 1 and (counts == 1).all()  # everyone wants 16: C' = 1
            ids, counts, info = _plan_agrees(acc, want, 0.0, REL, 0, 1, 0.25, 16, name)
            assert info["pixels"] == int(dark.sum())
            # thresholds inside the spread of sqrt(g) with different gains, pass sizes and C
            for abs_tol, n, gain, C in ((0.008, 1, 1.0, 16), (0.012, 1, 0.5, 8), (0.006, 2, 1.0, 4), (0.015, 4, 0.25, 16),
                                        (0.004, 1, 0.05, 16))[:2 if big else 5]:
                ids, counts, info = _plan_agrees(acc, want, abs_tol, 0.0, 0, n, gain, C, (name, abs_tol, n, gain, C))
            # max_n without per-pixel counts (N = 2 everywhere): at N nothing is listed, above it the clip holds
            _, _, info = _plan_agrees(acc, want, 0.0, 0.0, 2, 1, 1.0, 16, "max_n at N")
            assert info["pixels"] == 0
            for max_n in (3, 5, 40)[:1 if big else 3]:
                _plan_agrees(acc, want, 0.006, 0.0, max_n, 1, 1.0, 16, ("max_n", max_n))
                _plan_agrees(acc, want, 0.006, 0.0, max_n, 2, 1.0, 16, ("max_n, n = 2", max_n))
            # a smaller cap: the first entries, the full totals
            e_ids, e_counts, e_units, e_passes = br.plan(want, 0.008, 0.0, 0, 1, 1.0, 16)
            for cap in (0, 1, max(1, e_ids.size // 2))[1 if big else 0:]:
                ids, counts, info = acc.plan(0.008, 0.0, 0, 1, 1.0, 16, cap=cap)
                assert np.array_equal(ids, e_ids[:cap]) and np.array_equal(counts, e_counts[:cap])
                assert info == dict(pixels=int(e_ids.size), units=e_units, passes=e_passes)
            # per-pixel counts: a sparse pass over the dark pixels takes them to N_p = 5
            sel = np.flatnonzero(dark.reshape(-1)).astype(np.uint32)
            part = dref.gather(m1, sel)
            want.add_sub_pixels(sel, part, 3)
            acc.add_sub_pixels(sel, part, 3)
            for max_n in (0, 3, 5, 6, 9)[:2 if big else 5]:
                _plan_agrees(acc, want, 0.004, 0.0, max_n, 1, 1.0, 16, ("counts, max_n", max_n))
                _plan_agrees(acc, want, 0.0, 0.0, max_n, 2, 1.0, 16, ("counts, thr = 0, max_n", max_n))


def test_plan_frame_cap(rt, gpu_scenes):
    """The cap cases of tests/test_batch_abi.py scaled to 67 x 35 = 2345 pixels, thr = 0 so that every listed pixel
    wants C: every pixel wanting 16 gives C' = 1; 781 pixels wanting 4 give 2343 units at C' = 3 and 3124 at C' = 4, so
    C' = 3; 586 pixels wanting 4 (2344 units) give C' = 4. The listed pixels are those below max_n: the others got a
    sparse pass of 50 samples first. The device form gives the host form's lists."""
    w, h = W, H
    npix = w * h
    rng = np.random.default_rng(5)
    m1, m2 = _select_passes(w, h, np.zeros((h, w), dtype=bool))
    for k, C, c1, units in ((npix, 16, 1, npix), (781, 4, 3, 2343), (586, 4, 4, 2344)):
        chosen = np.sort(rng.choice(npix, size=k, replace=False))
        rest = np.setdiff1d(np.arange(npix), chosen).astype(np.uint32)
        want = dref.Accum(w, h)
        with rt.Accumulator(w, h) as acc:
            for a in (want, acc):
                a.add_sub(m1, 1)
                a.add_sub(m2, 1)
                if rest.size:
                    a.add_sub_pixels(rest, dref.gather(m1, rest), 50)
            ids, counts, info = _plan_agrees(acc, want, 0.0, 0.0, 40, 1, 1.0, C, (k, C))
            assert np.array_equal(ids, chosen) and (counts == c1).all()
            assert info == dict(pixels=k, units=units, passes=c1)
            d_ids = torch.full((npix,), -1, dtype=torch.int32, device="cuda")
            d_cnt = torch.full((npix,), 99, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            n_out, u_out, p_out = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
            rt._check(rt.lib.rt_accum_plan_device(acc.handle, 0.0, 0.0, 40, 1, 1.0, C, V(d_ids.data_ptr()),
                                                  V(d_cnt.data_ptr()), npix, ctypes.byref(n_out), ctypes.byref(u_out),
                                                  ctypes.byref(p_out), None))
            assert (n_out.value, u_out.value, p_out.value) == (k, units, c1)
            got_i, got_c = d_ids.cpu().numpy(), d_cnt.cpu().numpy()
            assert np.array_equal(got_i[:k].astype(np.uint32), ids) and np.array_equal(got_c[:k], counts)
            assert np.all(got_i[k:] == -1) and np.all(got_c[k:] == 99)


def test_refine_is_plan_then_add_passes(rt, gpu_scenes):
    """Passes of 4 spp (n = 1) at the target that leaves about a quarter of the pixels active after two 8-spp passes
    (bisected on the device's own count, so the frame cap leaves room for several passes per pixel), then a second
    step with a gain of 0.5 and a budget."""
    w, h, spp = 48, 36, 4
    sc = gpu_scenes["cornell_box"]
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
            assert max_n or (info["passes"] > 1 and info["units"] > info["pixels"])
            st = a.refine(sc, spp, seeds, abs_tol, 0.0, max_n, gain)
            assert not st["cancelled"] and st["refine"] == (info["pixels"], info["units"], info["passes"])
            assert st["samples"] == info["units"] * spp
            b.add_passes(sc, ids, counts, spp, seeds)
            ka, na = a.counts()
            kb, nb = b.counts()
            assert np.array_equal(ka, kb) and np.array_equal(na, nb)
            ra, rb = a.resolve(want_var=True), b.resolve(want_var=True)
            assert _same(ra[0], rb[0]) and _same(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
            if max_n:
                assert na.reshape(-1)[ids].max() <= max_n - 1 + spp // 4
        # a cancelled refine merges nothing; an empty plan launches nothing
        n0 = a.counts()[1]
        st = a.refine(sc, spp, seeds, abs_tol / 2, 0.0, 0, 0.5, cancel=ctypes.c_int32(1))
        assert st["cancelled"] and np.array_equal(a.counts()[1], n0)
        st = a.refine(sc, spp, seeds, 10.0, 0.0, 0, 0.5)
        assert st["refine"] == (0, 0, 0) and st["samples"] == 0 and np.array_equal(a.counts()[1], n0)


def test_render_to_error_batched_front_end(rt, gpu_scenes):
    """The generator with batch > 0: a frame after the two full passes and after every batch, the mean spp grows, no
    pixel goes past max_spp + pass_spp - 4, and the last frame has nothing active."""
    w, h = 48, 36
    out = list(rt.render_to_error(gpu_scenes["cornell_box"], w, h, abs_tol=0.05, max_spp=48, first=16, pass_spp=16, seed=5,
                                  **rt.ERROR_TARGET_BATCH_DEFAULTS))
    assert len(out) >= 2
    spps = [m for _, m, _ in out]
    assert spps[0] == 16.0 and all(b > a for a, b in zip(spps, spps[1:])) and spps[-1] <= 48.0 + 12.0
    assert out[-1][2] == 0.0 and out[0][2] > 0.0
    for rgb, _, frac in out:
        assert rgb.shape == (h, w, 3) and rgb.dtype == np.uint8 and rgb.max() > 50 and 0.0 <= frac <= 1.0


# The loop end to end --------------------------------------------------------------------------------------------
# The CPU oracle's study (tools/batch_oracle.py, profiles/batch_target.log): cornell_box 96 x 72, seeds
# 77 / 78 / 79. At the chosen defaults (C = 8, gain = 1) seed 77 took 30 render launches after the two full passes
# (sequential: 51); the sequential loop's seed-to-seed spread was 1.84 in the mean spp and 0.001616 in the linear RMSE.
ORACLE_LAUNCHES, SPREAD_SPP, SPREAD_RMSE = 30, 1.84, 0.001616


def _rmse(sub, truth):
    return float(np.sqrt(np.mean((aref.c_of(sub) - truth) ** 2)))


def test_end_to_end(rt, gpu_scenes):
    """cornell_box 96 x 72 with DESIGN.md §13's set-up (abs_tol 0.04, first 16, pass_spp 16, max_spp 496, truth a
    4096-spp frame of seed 999), seed 77: the batched loop at ERROR_TARGET_BATCH_DEFAULTS beside the sequential one.
      * the batched render launches are at most the oracle's count plus one;
      * its mean spp and linear RMSE are at most the sequential loop's plus the sequential loop's seed-to-seed spread on
        the oracle;
      * no pixel is above max_spp + pass_spp - 4.
    The device's figures are printed and recorded in DESIGN.md §17."""
    w, h, abs_tol, seed, max_spp = 96, 72, 0.04, 77, 496
    d = rt.ERROR_TARGET_BATCH_DEFAULTS
    assert (d["batch"], d["gain"]) == (8, 1.0)  # the study's choice, which ORACLE_LAUNCHES belongs to
    sc = gpu_scenes["cornell_box"]
    _, truth_sub, _ = rt.render(sc, w, h, 4096, 999, megakernel=True, want_sub=True)
    truth = aref.c_of(truth_sub)
    max_n = max_spp // 4
    res = {}
    for name in ("sequential", "batched"):
        with rt.Accumulator(w, h) as acc:
            acc.add(sc, 8, rt.pass_seed(seed, 0))
            acc.add(sc, 8, rt.pass_seed(seed, 1))
            k, launches = 2, 0
            while True:
                if name == "sequential":
                    ids, n = acc.select(abs_tol, 0.0, max_n)
                    if n == 0:
                        break
                    acc.add_pixels(sc, ids, 16, rt.pass_seed(seed, k))
                    k += 1
                else:
                    st = acc.refine(sc, 16, [rt.pass_seed(seed, k + i) for i in range(d["batch"])], abs_tol, 0.0, max_n,
                                    d["gain"])
                    if st["refine"][0] == 0:
                        break
                    k += st["refine"][2]
                launches += 1
                assert launches < 200
            n_p = acc.counts()[1].astype(np.float64)
            res[name] = (launches, 4.0 * n_p.mean(), 4.0 * n_p.max(), _rmse(acc.resolve()[0], truth))
    for name, r in res.items():
        print(f"{name}: {r[0]} render launches, mean spp {r[1]:.2f}, max spp {r[2]:.0f}, linear RMSE {r[3]:.6f}")
    seq, bat = res["sequential"], res["batched"]
    assert bat[0] <= ORACLE_LAUNCHES + 1
    assert bat[1] <= seq[1] + SPREAD_SPP
    assert bat[3] <= seq[3] + SPREAD_RMSE
    assert bat[2] <= max_spp + 16 - 4 and seq[2] <= max_spp + 16 - 4
