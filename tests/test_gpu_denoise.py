"""The a-trous filter (rt_denoise, k_atrous_*) against its numpy restatement (tests/denoise_ref.py), its exact
properties, what it buys at 16 spp, and the server's whole-frame denoising renderer."""
import asyncio

import numpy as np
import pytest

import denoise_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED


@pytest.fixture(scope="module")
def cornell_96x80(rt, gpu_scenes):
    _, sub, _ = rt.render(gpu_scenes["cornell_box"], 96, 80, 8, SEED, megakernel=True, want_sub=True)
    return sub, rt.render_features(gpu_scenes["cornell_box"], 96, 80)


@pytest.mark.parametrize("width,height", ref.SIZES)
def test_filter_matches_restatement(rt, width, height):
    """levels 1, 3, 5 with every sigma on and once with each sigma <= 0, on synthetic inputs: the linear output agrees
    with the f64 restatement to 8 * d32 absolute, RGB8 to 1. d32 = 8.3e-7 is the largest difference between the f32 and
    the f64 restatement over these cases (tests/test_denoise_abi.py::test_d32_is_the_recorded_value); the margin of 8
    covers the device's exp and division differing from numpy's by an ulp or so per tap over up to five chained
    levels."""
    sub, feat = ref.synthetic(width, height)
    worst = 0.0
    for levels in ref.LEVELS:
        for sig in ref.SIGMA_CASES:
            want = ref.atrous(sub, feat, levels, **sig)
            rgb, lin = rt.denoise(sub, feat, levels=levels, want_linear=True, **sig)
            d = float(np.abs(lin.astype(np.float64) - want).max())
            worst = max(worst, d)
            assert d <= 8 * ref.D32, (levels, sig, d)
            assert np.abs(rgb.astype(np.int32) - ref.rgb8_of(want).astype(np.int32)).max() <= 1
            assert np.array_equal(rgb, ref.rgb8_of(lin))  # RGB8 is the gamma of the linear output
    print(f"{width}x{height}: worst |device - restatement| = {worst:.3e} ({worst / ref.D32:.2f} d32)")


def test_levels_zero_is_rt_render(rt, gpu_scenes):
    """levels = 0: rgb_out is rt_render's rgb_out byte for byte, the linear output is c0."""
    scene = gpu_scenes["cornell_box"]
    rgb, sub, _ = rt.render(scene, 64, 48, 8, SEED, megakernel=True, want_sub=True)
    feat = rt.render_features(scene, 64, 48)
    out, lin = rt.denoise(sub, feat, levels=0, want_linear=True)
    assert np.array_equal(out, rgb) and rgb.max() > 100
    assert np.array_equal(lin, ref.c0_of(sub).astype(np.float32))
    assert np.array_equal(rt.denoise(sub, feat, levels=0), rgb)


def test_constant_image_is_a_fixed_point(rt):
    sub, feat = ref.synthetic(67, 35)
    const = np.array([0.3, 0.6, 0.9])
    sub[:] = const
    _, lin = rt.denoise(sub, feat, levels=5, want_linear=True, **ref.SIGMA_ON)
    assert np.abs(lin - const).max() <= 1e-6


def test_albedo_step_is_not_crossed(rt):
    """Albedo 0 | 1 with sigma_a = 0.1 (E = 100 across the step; hipcc keeps f32 subnormals, so the leak is about
    e^-100, not exactly 0): no pixel moves by more than 1e-6."""
    w, h = 48, 24
    sub = np.zeros((h, w, 4, 3))
    sub[:, : w // 2] = (0.2, 0.5, 0.8)
    sub[:, w // 2:] = (0.9, 0.1, 0.4)
    feat = np.zeros((h, w, 8), dtype=np.float32)
    feat[..., 0:3] = (0.0, 0.0, 1.0)
    feat[..., 3] = 10.0
    feat[..., 4:7] = 0.5
    feat[:, w // 2:, 4] = 1.0
    feat[:, : w // 2, 4] = 0.0
    feat[..., 7] = 1.0
    _, lin = rt.denoise(sub, feat, levels=5, sigma_c=0.0, sigma_n=0.5, sigma_z=0.5, sigma_a=0.1, want_linear=True)
    assert np.abs(lin.astype(np.float64) - ref.c0_of(sub)).max() <= 1e-6
    # without the albedo term the step does blur: the check above is the term's doing
    _, blur = rt.denoise(sub, feat, levels=5, sigma_c=0.0, sigma_n=0.5, sigma_z=0.5, sigma_a=0.0, want_linear=True)
    assert np.abs(blur.astype(np.float64) - ref.c0_of(sub)).max() > 0.1


def test_same_call_twice_is_bit_identical(rt, cornell_96x80):
    for sub, feat in (ref.synthetic(67, 35), cornell_96x80):
        a = rt.denoise(sub, feat, levels=5, want_linear=True, **ref.SIGMA_ON)
        b = rt.denoise(sub, feat, levels=5, want_linear=True, **ref.SIGMA_ON)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_tile_independence(rt, cornell_96x80):
    """levels = 2 reads rows up to 2 (2^2 - 1) = 6 away: rows [14, 66) denoised as their own image, rows [20, 60) of
    it kept, equal those rows of the whole-frame result bit for bit (the lattice and LDS indexing at the edges)."""
    sub, feat = cornell_96x80
    p = dict(rt.DENOISE_DEFAULTS, levels=2)
    rgb, lin = rt.denoise(sub, feat, want_linear=True, **p)
    rgb_t, lin_t = rt.denoise(sub[14:66], feat[14:66], want_linear=True, **p)
    assert np.array_equal(lin_t[6:46].view(np.uint32), lin[20:60].view(np.uint32))
    assert np.array_equal(rgb_t[6:46], rgb[20:60])
    assert not np.array_equal(lin, ref.c0_of(sub).astype(np.float32))


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - b) ** 2)))


@pytest.mark.parametrize("name", ("cornell_box", "cubes", "flying_unicorn"))
def test_it_denoises(rt, gpu_scenes, name):
    """96 x 72 at 16 spp, DENOISE_DEFAULTS: the denoised frame's linear RMSE against a 1024-spp frame of another seed
    is below the noisy frame's."""
    scene = gpu_scenes[name]
    _, sub, _ = rt.render(scene, 96, 72, 16, SEED, megakernel=True, want_sub=True)
    _, sub_ref, _ = rt.render(scene, 96, 72, 1024, SEED + 77, megakernel=True, want_sub=True)
    truth = ref.c0_of(sub_ref)
    feat = rt.render_features(scene, 96, 72)
    _, lin = rt.denoise(sub, feat, want_linear=True)
    noisy, den = _rmse(ref.c0_of(sub), truth), _rmse(lin, truth)
    print(f"{name}: RMSE noisy {noisy:.4f} -> denoised {den:.4f} (ratio {den / noisy:.3f})")
    assert den < noisy


def test_server_denoised_frames(rt, gpu_scenes):
    """The whole-frame denoising renderer driven through RenderJob at 60 x 45 yields the chunk messages of
    render_denoised of the same seed."""
    from rt_amd import server

    w, h, spp = 60, 45, 8
    scene = gpu_scenes["cornell_box"]
    got = []

    async def send(msg):
        got.append(msg)

    job = server.RenderJob(send, server.gpu_denoised_frame_renderer(levels=3), band_rows=h)
    assert asyncio.run(job.run(scene, w, h, spp, SEED)) is False
    want = rt.render_denoised(scene, w, h, spp, SEED, levels=3)
    assert got == list(server.chunk_messages(want, 0)) and len(got) == h
    plain, _, _ = rt.render(scene, w, h, spp, SEED, megakernel=True)
    assert not np.array_equal(want, plain)
