"""The accumulator (rt_accum_*, k_accum_add / k_accum_resolve) against its numpy restatement (tests/accum_ref.py) bit
for bit, and rt_accum_add against rt_render."""
import ctypes

import numpy as np
import pytest
import torch  # before rt_amd loads, as bench.py: the process's HIP runtime is the one torch brings

import accum_ref as aref

pytestmark = pytest.mark.gpu

SEED_A, SEED_B = 0x5EED, 0xC0FFEE
NS = (1, 2, 5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def cornell_passes(rt, gpu_scenes):
    """rt_render's frames of cornell_box 64 x 48: (spp 8, seed a) and (spp 16, seed b), megakernel and wavefront."""
    sc = gpu_scenes["cornell_box"]
    out = {}
    for mk in (True, False):
        out[mk] = [rt.render(sc, 64, 48, spp, seed, megakernel=mk, want_sub=True)[:2]
                   for spp, seed in ((8, SEED_A), (16, SEED_B))]
    return out


@pytest.mark.parametrize("width,height", ((1, 1), (5, 3), (67, 35)))
def test_synthetic_passes_match_restatement(rt, gpu_scenes, width, height):
    """n = (1, 2, 5) through add_sub: sub_out, var_out and rgb_out are the restatement's bits after every pass; the
    device entry points give the host ones' bits."""
    passes = aref.synthetic_passes(width, height, NS)
    want = aref.Accum(width, height)
    with rt.Accumulator(width, height) as acc, rt.Accumulator(width, height) as dev:
        for k, (m, n) in enumerate(zip(passes, NS)):
            want.add_sub(m, n)
            acc.add_sub(m, n)
            d_m = torch.from_numpy(m).to("cuda")
            torch.cuda.synchronize()
            rt._check(rt.lib.rt_accum_add_sub_device(dev.handle, ctypes.c_void_p(d_m.data_ptr()), n, None))
            assert acc.info() == dev.info() == dict(passes=k + 1, n=sum(NS[:k + 1]), width=width, height=height)
            sub, var, rgb = acc.resolve(want_var=k >= 1)
            assert _same(sub, want.sub())
            assert np.array_equal(rgb, want.rgb())
            if k >= 1:
                assert _same(var, want.var()) and var[..., 3].max() > 0
            # the device forms
            d_sub = torch.zeros((height, width, 4, 3), dtype=torch.float64, device="cuda")
            d_var = torch.zeros((height, width, 4), dtype=torch.float32, device="cuda")
            d_rgb = torch.zeros((height, width, 3), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rt._check(rt.lib.rt_accum_resolve_device(dev.handle, ctypes.c_void_p(d_sub.data_ptr()),
                                                     ctypes.c_void_p(d_var.data_ptr()) if k >= 1 else None,
                                                     ctypes.c_void_p(d_rgb.data_ptr()), None))
            assert _same(d_sub.cpu().numpy(), sub) and np.array_equal(d_rgb.cpu().numpy(), rgb)
            if k >= 1:
                assert _same(d_var.cpu().numpy(), var)
            # RGB8 alone (through the accumulator's staging sub)
            d_rgb.zero_()
            torch.cuda.synchronize()
            rt._check(rt.lib.rt_accum_resolve_device(dev.handle, None, None, ctypes.c_void_p(d_rgb.data_ptr()), None))
            assert np.array_equal(d_rgb.cpu().numpy(), rgb)
        only_var = acc.resolve(want_sub=False, want_var=True, want_rgb=False)
        assert only_var[0] is None and only_var[2] is None and _same(only_var[1], want.var())


def test_one_add_is_rt_render(rt, gpu_scenes, cornell_passes):
    """One rt_accum_add at spp 8 (n = 2: n m / n is exact): sub_out and rgb_out are rt_render's, bit for bit and byte
    for byte; var_out needs two passes (RT_E_INVAL)."""
    rgb, sub = cornell_passes[True][0]
    with rt.Accumulator(64, 48) as acc:
        st = acc.add(gpu_scenes["cornell_box"], 8, SEED_A)
        assert not st["cancelled"] and st["samples"] == 64 * 48 * 8
        assert acc.info() == dict(passes=1, n=2, width=64, height=48)
        got_sub, _, got_rgb = acc.resolve()
        assert _same(got_sub, sub) and np.array_equal(got_rgb, rgb) and rgb.max() > 100
        with pytest.raises(rt.RtError) as e:
            acc.resolve(want_var=True)
        assert e.value.code == -1


@pytest.mark.parametrize("megakernel", (True, False))
def test_two_adds_equal_add_sub_of_rt_render(rt, gpu_scenes, cornell_passes, megakernel):
    """Two rt_accum_adds (spp 8 seed a, spp 16 seed b) equal add_sub of the two rt_render sub_outs, and the
    restatement, bit for bit."""
    sc = gpu_scenes["cornell_box"]
    (_, sub_a), (_, sub_b) = cornell_passes[megakernel]
    want = aref.Accum(64, 48)
    want.add_sub(sub_a, 2)
    want.add_sub(sub_b, 4)
    with rt.Accumulator(64, 48) as acc, rt.Accumulator(64, 48) as fed:
        acc.add(sc, 8, SEED_A, megakernel=megakernel)
        acc.add(sc, 16, SEED_B, megakernel=megakernel)
        fed.add_sub(sub_a, 2)
        fed.add_sub(sub_b, 4)
        assert acc.info() == fed.info() == dict(passes=2, n=6, width=64, height=48)
        a, b = acc.resolve(want_var=True), fed.resolve(want_var=True)
        for x, y in zip(a[:2], b[:2]):
            assert _same(x, y)
        assert np.array_equal(a[2], b[2])
        assert _same(a[0], want.sub()) and _same(a[1], want.var()) and np.array_equal(a[2], want.rgb())
        assert a[1][..., 3].max() > 0


def test_same_seed_twice_has_no_variance(rt, gpu_scenes):
    """Two passes of one seed are one pass twice: the per-subpixel variance Q / N - m^2 is cancellation noise, at most
    1e-12 m^2 (checked on the sums through the restatement of the resolve: the pixel variance is their sum over 16)."""
    sc = gpu_scenes["cornell_box"]
    with rt.Accumulator(64, 48) as acc:
        acc.add(sc, 8, SEED_A)
        acc.add(sc, 8, SEED_A)
        sub, var, _ = acc.resolve(want_var=True)
    m2 = (sub * sub)
    inside = (sub > 0) & (sub < 1)
    bound = (np.where(inside, 1e-12 * m2, 0.0).sum(2) / 16.0)
    slack = 1.0 + 1e-6  # the f32 rounding of var_out
    assert inside.mean() > 0.5 and np.all(var >= 0)
    assert np.all(var[..., :3].astype(np.float64) <= bound * slack)
    assert np.all(var[..., 3].astype(np.float64) <= bound.sum(-1) * slack)


def test_reset_then_reuse_equals_fresh(rt, gpu_scenes):
    passes = aref.synthetic_passes(67, 35, NS)
    with rt.Accumulator(67, 35) as used, rt.Accumulator(67, 35) as fresh:
        used.add_sub(passes[2], 7)
        used.add_sub(passes[0], 3)
        used.reset()
        assert used.info()["passes"] == 0 and used.info()["n"] == 0
        with pytest.raises(rt.RtError):
            used.resolve()
        for acc in (used, fresh):
            acc.add_sub(passes[0], 1)
            acc.add_sub(passes[1], 2)
        a, b = used.resolve(want_var=True), fresh.resolve(want_var=True)
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("megakernel", (True, False))
def test_cancel_word_already_set(rt, gpu_scenes, megakernel):
    """A cancel word already set: RT_CANCELLED, info and the sums unchanged."""
    sc = gpu_scenes["cornell_box"]
    with rt.Accumulator(64, 48) as acc:
        acc.add(sc, 8, SEED_A, megakernel=megakernel)
        before = acc.resolve()
        st = acc.add(sc, 16, SEED_B, megakernel=megakernel, cancel=ctypes.c_int32(1))
        assert st["cancelled"]
        assert acc.info() == dict(passes=1, n=2, width=64, height=48)
        after = acc.resolve()
        assert _same(before[0], after[0]) and np.array_equal(before[2], after[2])
        # and the accumulator goes on
        assert not acc.add(sc, 16, SEED_B, megakernel=megakernel, cancel=ctypes.c_int32(0))["cancelled"]
        assert acc.info()["passes"] == 2 and acc.info()["n"] == 6
