"""The range guards of the exact-arithmetic shortcuts (path_f64.h: rcp_safe_all, sqrt_fast_all, div_sqrt).

A shortcut (rcp_rn / qdiv / the unscaled sqrt sequence) is taken only when every lane of the wave is inside
its range (a wave vote), so a lane's bits must not depend on its wave-mates: the fast form and the library
form have to agree bit for bit wherever the fast one can run, and a wave with one lane outside the range
has to give every lane the library's result. The device self-test counts violations of both; the small
renders run every guarded helper of the sphere, plane and mesh paths with mixed lanes, against the oracle.
"""
import ctypes

import pytest

from test_gpu_parity import SEED, _assert_parity

pytestmark = pytest.mark.gpu


def test_selftest_counts_are_zero(rt, gpu_scenes):
    """rt_selftest_arith_n with five outputs on 2^20 operands: reciprocal, quotient, square root, the fused
    normalise a / sqrt(x) over every exponent of [2^-767, 2^1023], and all of them in waves where one lane
    (rotating) holds 0, a subnormal, 2^-800, 2^+-1000, inf, NaN, a negative radicand, or a value at an edge of
    the guards' windows (2^900 and its neighbours, around 2^-900 and 2^-767, the largest finite double); both
    guard forms (the default and the fused mesh instances' G1)."""
    out = (ctypes.c_ulonglong * 5)(*([1 << 40] * 5))
    assert rt.lib.rt_selftest_arith_n(1 << 20, SEED, out, 5) == 0
    counts = [int(v) for v in out]
    print("selftest counts (rcp, qdiv, sqrt, div_sqrt, mixed waves):", counts)
    assert counts == [0, 0, 0, 0, 0]
    # the three-output form is unchanged
    assert rt.selftest_arith(1 << 16) == (0, 0, 0)


@pytest.mark.parametrize("name,spp", [("cornell_box", 16), ("cubes", 8)])
def test_small_frames_match_the_oracle(name, spp, rt, gpu_scenes, oracle_scenes):
    """64x48: the smallest frames at which every guarded helper runs with mixed lanes (waves holding camera,
    diffuse and mirror vertices, sphere misses, ended paths): megakernel and wavefront against the oracle at
    the suite's 1e-9 / RGB8 bounds, and bit-identical to each other."""
    w, h = 64, 48
    rgb_o, sub_o, st_o = oracle_scenes[name].render(w, h, spp, SEED)
    frames = []
    for mk in (True, False):
        rgb_g, sub_g, st = rt.render(gpu_scenes[name], w, h, spp, SEED, megakernel=mk, want_sub=True)
        assert st["samples"] == w * h * 4 * (spp // 4)
        assert 0.9 * st_o["vertices"] <= st["vertices"] <= st_o["vertices"]
        _assert_parity(rgb_g, sub_g, rgb_o, sub_o, f"{name}/{'mk' if mk else 'wf'}")
        frames.append((rgb_g, sub_g))
    assert (frames[0][0] == frames[1][0]).all() and (frames[0][1] == frames[1][1]).all()
