"""The _device forms that only argument tests reached (rt_denoise_device, rt_denoise_var_device, rt_accum_holes_device)
against their host forms: torch tensors on the device, data_ptr(), the null stream, as tests/test_gpu_accum.py calls
rt_accum_resolve_device. Both forms run the same kernels on the same inputs, so every output is equal bit for bit."""
import ctypes

import numpy as np
import pytest
import torch  # before rt_amd loads, as bench.py: the process's HIP runtime is the one torch brings

from test_gpu_fill import _raw_holes, _views
from test_gpu_reproject import _fill_src, _same

pytestmark = pytest.mark.gpu

SEED = 0x5EED
# no multiple of the filter's 16-pixel patch in either direction; at level 2 (stride 4) the sub-lattices differ in size
W, H = 33, 17
NONE = 0xFFFFFFFF


def _dev(a):
    return ctypes.c_void_p(a.data_ptr()) if a is not None else None


@pytest.fixture(scope="module")
def frame(rt, gpu_scenes):
    """cornell_box at 33 x 17 and 8 spp, as two passes of 4 spp: (sub, feat, var)."""
    sc = gpu_scenes["cornell_box"]
    with rt.Accumulator(W, H) as acc:
        acc.add(sc, 4, SEED)
        acc.add(sc, 4, rt.pass_seed(SEED, 1))
        sub, var, _ = acc.resolve(want_var=True, want_rgb=False)
    assert var[..., 3].max() > 0
    return sub, rt.render_features(sc, W, H), var


def _device_denoise(rt, frame, var, levels, sig, want_lin, want_var):
    """rt_denoise_device (var None) / rt_denoise_var_device on device copies of the frame: (rgb, lin, vout) as numpy."""
    sub, feat, v = frame
    d_sub, d_feat = torch.from_numpy(sub).to("cuda"), torch.from_numpy(feat).to("cuda")
    d_rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    d_lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") if want_lin else None
    d_vout = torch.zeros((H, W), dtype=torch.float32, device="cuda") if want_var else None
    if var:
        d_var = torch.from_numpy(v).to("cuda")
        torch.cuda.synchronize()
        rt._check(rt.lib.rt_denoise_var_device(0, W, H, _dev(d_sub), _dev(d_feat), _dev(d_var), levels, *sig,
                                               _dev(d_rgb), _dev(d_lin), _dev(d_vout), None))
    else:
        torch.cuda.synchronize()
        rt._check(rt.lib.rt_denoise_device(0, W, H, _dev(d_sub), _dev(d_feat), levels, *sig, _dev(d_rgb), _dev(d_lin),
                                           None))
    return [None if t is None else t.cpu().numpy() for t in (d_rgb, d_lin, d_vout)]


@pytest.mark.parametrize("want_lin", (False, True))
@pytest.mark.parametrize("levels", (0, 2))
def test_denoise_device_equals_the_host_form(rt, frame, levels, want_lin):
    sub, feat, _ = frame
    sig = [rt.DENOISE_DEFAULTS[k] for k in ("sigma_c", "sigma_n", "sigma_z", "sigma_a")]
    want = rt.denoise(sub, feat, levels, *sig, want_linear=want_lin)
    rgb, lin, _ = _device_denoise(rt, frame, False, levels, sig, want_lin, False)
    assert np.array_equal(rgb, want[0] if want_lin else want)
    if want_lin:
        assert _same(lin, want[1]) and lin.max() > 0
    if levels == 0:  # the pass-through is rt_render's own RGB8 of the frame
        assert rgb.max() > 0


@pytest.mark.parametrize("want_lin,want_var", ((False, False), (True, False), (False, True), (True, True)))
@pytest.mark.parametrize("levels", (0, 2))
def test_denoise_var_device_equals_the_host_form(rt, frame, levels, want_lin, want_var):
    sub, feat, var = frame
    sig = [rt.DENOISE_VAR_DEFAULTS[k] for k in ("sigma_c", "sigma_n", "sigma_z", "sigma_a")]
    want = rt.denoise_var(sub, feat, var, levels, *sig, want_linear=want_lin, want_var=want_var)
    want = list(want) if isinstance(want, tuple) else [want]
    rgb, lin, vout = _device_denoise(rt, frame, True, levels, sig, want_lin, want_var)
    assert np.array_equal(rgb, want.pop(0)) and rgb.max() > 0
    if want_lin:
        assert _same(lin, want.pop(0)) and lin.max() > 0
    if want_var:
        assert _same(vout, want.pop(0)) and vout.max() > 0


@pytest.mark.parametrize("period,phase", ((0, 0), (3, 0), (3, 2)))
def test_holes_device_equals_the_host_form(rt, gpu_scenes, period, phase):
    """The list, n_out and n_holes of rt_accum_holes_device are rt_accum_holes's, with room for every id, with a cap
    below the count (the count comes back in full, only cap ids are written) and with no room at all."""
    base = gpu_scenes["cornell_box"]
    _, _, view = _views(base, "A")
    src, _ = _fill_src(rt, W, H)
    with src, rt.Accumulator(W, H) as dst:
        n_valid = dst.reproject_from(src, view, base, 6)
        assert 0 < n_valid < W * H  # both kinds of pixel
        _, count, _ = _raw_holes(rt, dst, period, phase, W * H)
        assert count >= 2  # so that half of it is a cap that cuts
        for cap in (W * H, count // 2, 0):
            ids, n, nh = _raw_holes(rt, dst, period, phase, cap)
            assert n == count and nh == W * H - n_valid
            d_ids = torch.full((max(1, cap),), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            d_n, d_nh = ctypes.c_int64(-1), ctypes.c_int64(-1)
            rt._check(rt.lib.rt_accum_holes_device(dst.handle, period, phase, _dev(d_ids), cap, ctypes.byref(d_n),
                                                   ctypes.byref(d_nh), None))
            got = d_ids.cpu().numpy().view(np.uint32)
            assert (d_n.value, d_nh.value) == (n, nh)
            assert np.array_equal(got, ids) and (got[min(n, cap):] == NONE).all()
