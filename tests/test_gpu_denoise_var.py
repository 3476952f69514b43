"""The variance-guided a-trous filter (rt_denoise_var, k_atrous_level_var) against its numpy restatement
(tests/accum_ref.py), its exact properties, what it buys at 16 and at 1024 spp, and the progressive front-ends
(rt_amd.render_progressive, server.ProgressiveJob)."""
import asyncio

import numpy as np
import pytest
import torch  # noqa: F401  before rt_amd loads, as bench.py: the process's HIP runtime is the one torch brings

import accum_ref as aref
import denoise_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _accumulate(rt, scene, w, h, passes, spp, seed=SEED):
    """(sub, var) of `passes` passes of `spp` with render_progressive's seeds."""
    with rt.Accumulator(w, h) as acc:
        for k in range(passes):
            acc.add(scene, spp, aref.pass_seed(seed, k))
        sub, var, _ = acc.resolve(want_var=True, want_rgb=False)
    return sub, var


@pytest.fixture(scope="module")
def cornell_96x80(rt, gpu_scenes):
    sub, var = _accumulate(rt, gpu_scenes["cornell_box"], 96, 80, 2, 8)
    return sub, rt.render_features(gpu_scenes["cornell_box"], 96, 80), var


@pytest.mark.parametrize("width,height", ref.SIZES)
def test_filter_matches_restatement(rt, width, height):
    """levels 1, 3, 5 with every sigma on and once with each sigma <= 0, on synthetic inputs and variances in
    [1e-4, 1e-1]: the linear output agrees with the f64 restatement to 8 * D32V absolute, RGB8 to 1 (and is the gamma of
    the linear output), the filtered variance to 8 * D32V_VAR_REL relative. D32V = 8.1e-7 and D32V_VAR_REL = 1.4e-5 are
    the largest differences between the f32 and the f64 restatement over these cases
    (tests/test_accum_abi.py::test_d32v_is_the_recorded_value); the margin of 8 is rt_denoise's (the device's exp,
    reciprocal and division differing from numpy's by an ulp or so per tap over up to five chained levels)."""
    sub, feat = ref.synthetic(width, height)
    var = aref.synthetic_var(width, height)
    worst, worst_v = 0.0, 0.0
    for levels in ref.LEVELS:
        for sig in ref.SIGMA_CASES:
            want, want_v = aref.atrous_var(sub, feat, var, levels, **sig)
            rgb, lin, vout = rt.denoise_var(sub, feat, var, levels=levels, want_linear=True, want_var=True, **sig)
            d = float(np.abs(lin.astype(np.float64) - want).max())
            dv = float((np.abs(vout.astype(np.float64) - want_v) / want_v).max())
            worst, worst_v = max(worst, d), max(worst_v, dv)
            assert d <= 8 * aref.D32V, (levels, sig, d)
            assert dv <= 8 * aref.D32V_VAR_REL, (levels, sig, dv)
            assert np.abs(rgb.astype(np.int32) - ref.rgb8_of(want).astype(np.int32)).max() <= 1
            assert np.array_equal(rgb, ref.rgb8_of(lin))  # RGB8 is the gamma of the linear output
    print(f"{width}x{height}: worst |device - restatement| = {worst:.3e} ({worst / aref.D32V:.2f} d32v), variance "
          f"{worst_v:.3e} relative ({worst_v / aref.D32V_VAR_REL:.2f} of its f32-f64 difference)")


def test_levels_zero_is_rt_render(rt, gpu_scenes):
    """levels = 0: rgb_out is rt_render's rgb_out byte for byte, the linear output is c0, the variance is the input."""
    scene = gpu_scenes["cornell_box"]
    rgb, sub, _ = rt.render(scene, 64, 48, 8, SEED, megakernel=True, want_sub=True)
    feat = rt.render_features(scene, 64, 48)
    var = aref.synthetic_var(64, 48)
    out, lin, vout = rt.denoise_var(sub, feat, var, levels=0, want_linear=True, want_var=True)
    assert np.array_equal(out, rgb) and rgb.max() > 100
    assert np.array_equal(lin, ref.c0_of(sub).astype(np.float32))
    assert np.array_equal(vout, var[..., 3])
    assert np.array_equal(rt.denoise_var(sub, feat, var, levels=0), rgb)


def test_zero_variance_moves_nothing(rt):
    """v = 0: no pixel moves by more than 1e-4 (the bound derived in
    tests/test_accum_abi.py::test_ref_zero_variance_moves_nothing), with every other term off."""
    sub, feat = ref.synthetic(67, 35)
    var = np.zeros((35, 67, 4), dtype=np.float32)
    _, lin, vout = rt.denoise_var(sub, feat, var, levels=3, sigma_c=1.0, sigma_n=0.0, sigma_z=0.0, sigma_a=0.0,
                                  want_linear=True, want_var=True)
    assert np.abs(lin.astype(np.float64) - ref.c0_of(sub)).max() <= 1e-4
    assert np.array_equal(vout, np.zeros_like(vout))


def test_huge_variance_is_denoise_without_colour_term(rt):
    """v = 1e30: the colour term vanishes, leaving rt_denoise with sigma_c = 0, to 8 * D32."""
    sub, feat = ref.synthetic(67, 35)
    var = np.full((35, 67, 4), 1e30, dtype=np.float32)
    for levels in (1, 3, 5):
        _, lin = rt.denoise_var(sub, feat, var, levels=levels, want_linear=True, **ref.SIGMA_ON)
        _, want = rt.denoise(sub, feat, levels=levels, want_linear=True, **dict(ref.SIGMA_ON, sigma_c=0.0))
        assert np.abs(lin.astype(np.float64) - want.astype(np.float64)).max() <= 8 * ref.D32
        assert np.isfinite(lin).all()


def test_same_call_twice_is_bit_identical(rt, cornell_96x80):
    s, f = ref.synthetic(67, 35)
    for sub, feat, var in ((s, f, aref.synthetic_var(67, 35)), cornell_96x80):
        a = rt.denoise_var(sub, feat, var, levels=5, want_linear=True, want_var=True, **ref.SIGMA_ON)
        b = rt.denoise_var(sub, feat, var, levels=5, want_linear=True, want_var=True, **ref.SIGMA_ON)
        assert np.array_equal(a[0], b[0])
        assert np.array_equal(_u32(a[1]), _u32(b[1])) and np.array_equal(_u32(a[2]), _u32(b[2]))


def test_tile_independence(rt, cornell_96x80):
    """levels = 2 reads rows up to 2 (2^2 - 1) = 6 away: rows [14, 66) filtered as their own image, rows [20, 60) of
    it kept, equal those rows of the whole-frame result bit for bit (the lattice and LDS indexing at the edges, and
    the variance tent's outside-the-image marks)."""
    sub, feat, var = cornell_96x80
    p = dict(rt.DENOISE_VAR_DEFAULTS, levels=2)
    rgb, lin, v = rt.denoise_var(sub, feat, var, want_linear=True, want_var=True, **p)
    rgb_t, lin_t, v_t = rt.denoise_var(sub[14:66], feat[14:66], var[14:66], want_linear=True, want_var=True, **p)
    assert np.array_equal(_u32(lin_t[6:46]), _u32(lin[20:60]))
    assert np.array_equal(_u32(v_t[6:46]), _u32(v[20:60]))
    assert np.array_equal(rgb_t[6:46], rgb[20:60])
    assert not np.array_equal(lin, ref.c0_of(sub).astype(np.float32))


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - b) ** 2)))


@pytest.mark.parametrize("name", ("cornell_box", "cubes", "flying_unicorn"))
def test_it_denoises_at_every_sample_count(rt, gpu_scenes, name):
    """96 x 72, truth = a 4096-spp frame of another seed, linear RMSE, DENOISE_VAR_DEFAULTS. With 2 passes x 8 spp the
    variance-guided frame beats the noisy one; with 8 passes x 128 spp it beats the noisy one and rt_denoise with
    DENOISE_DEFAULTS on the same accumulated sub (whose fixed colour term blurs what 1024 spp resolved).
    Measured (noisy / rt_denoise / variance-guided): 16 spp cornell 0.0816 / 0.0487 / 0.0508, cubes 0.0819 / 0.0455 /
    0.0475, unicorn 0.0842 / 0.0522 / 0.0536; 1024 spp cornell 0.0178 / 0.0208 / 0.0118, cubes 0.0157 / 0.0172 /
    0.0101, unicorn 0.0182 / 0.0223 / 0.0133."""
    scene = gpu_scenes[name]
    _, sub_ref, _ = rt.render(scene, 96, 72, 4096, SEED + 77, megakernel=True, want_sub=True)
    truth = ref.c0_of(sub_ref)
    feat = rt.render_features(scene, 96, 72)
    res = {}
    for passes, spp in ((2, 8), (8, 128)):
        sub, var = _accumulate(rt, scene, 96, 72, passes, spp)
        _, lin_v = rt.denoise_var(sub, feat, var, want_linear=True)
        _, lin_f = rt.denoise(sub, feat, want_linear=True)
        res[passes * spp] = (_rmse(ref.c0_of(sub), truth), _rmse(lin_f, truth), _rmse(lin_v, truth))
        print(f"{name} {passes} x {spp} spp: RMSE noisy {res[passes * spp][0]:.4f}, rt_denoise "
              f"{res[passes * spp][1]:.4f}, variance-guided {res[passes * spp][2]:.4f}")
    noisy, _, guided = res[16]
    assert guided < noisy
    noisy, fixed, guided = res[1024]
    assert guided < noisy
    assert guided < fixed


def _by_hand(rt, scene, w, h, passes, seed, **params):
    """The frames render_progressive must yield: an Accumulator driven by hand with the documented seeds."""
    feat = rt.render_features(scene, w, h)
    frames, done = [], 0
    with rt.Accumulator(w, h) as acc:
        for k, spp in enumerate(passes):
            acc.add(scene, spp, aref.pass_seed(seed, k))
            done += spp
            if k >= 1:
                sub, var, _ = acc.resolve(want_var=True, want_rgb=False)
                frames.append((rt.denoise_var(sub, feat, var, **params), done))
    return frames


def test_render_progressive(rt, gpu_scenes):
    """60 x 45, spp 64, first 8: frames at 8, 16, 32 and 64 spp, each the hand-driven accumulator's."""
    scene = gpu_scenes["cornell_box"]
    got = list(rt.render_progressive(scene, 60, 45, 64, first=8, seed=SEED))
    assert [n for _, n in got] == [8, 16, 32, 64]
    want = _by_hand(rt, scene, 60, 45, (4, 4, 8, 16, 32), SEED)
    for (g, gn), (w_, wn) in zip(got, want):
        assert gn == wn and g.shape == (45, 60, 3) and g.dtype == np.uint8 and np.array_equal(g, w_)
    assert not np.array_equal(got[0][0], got[-1][0])
    # denoise parameters pass through; levels = 0 is the accumulated frame itself
    with rt.Accumulator(60, 45) as acc:
        for k, spp in enumerate((4, 4)):
            acc.add(scene, spp, aref.pass_seed(SEED, k))
        plain = acc.resolve()[2]
    first = next(rt.render_progressive(scene, 60, 45, 64, first=8, seed=SEED, levels=0))
    assert first[1] == 8 and np.array_equal(first[0], plain)


def test_server_progressive_job(rt, gpu_scenes):
    """The progressive job emits the chunk messages of render_progressive's frames in order; a stop after the first
    frame ends it."""
    from rt_amd import server

    w, h, spp = 60, 45, 64
    scene = gpu_scenes["cornell_box"]
    frames = _by_hand(rt, scene, w, h, (4, 4, 8, 16, 32), SEED)
    want = [m for rgb, _ in frames for m in server.chunk_messages(rgb, 0)]
    got = []

    async def send(msg):
        got.append(msg)

    job = server.ProgressiveJob(send, first=8)
    assert not job.running()
    assert asyncio.run(job.run(scene, w, h, spp, SEED)) is False
    assert got == want and len(got) == 4 * h and not job.running()

    # a stop once the first frame is out: nothing of the second frame is sent
    got.clear()

    async def send_then_stop(msg):
        got.append(msg)
        if len(got) == h:
            job.stop()

    job.send = send_then_stop
    assert asyncio.run(job.run(scene, w, h, spp, SEED)) is True
    assert got == want[:h] and not job.running()
