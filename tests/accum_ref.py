"""numpy restatement of progressive accumulation (include/rt_ffi.h rt_accum_*, rt_denoise_var) —
TEST INFRASTRUCTURE ONLY.

  Accum      S = sum_k n_k m_k, Q = sum_k n_k m_k^2 per subpixel and channel, operation by operation as k_accum_add
             (S += n * m; Q += (n * m) * m; the first pass stores), and k_accum_resolve's outputs:
             sub = S / N;  vs = max(0, Q / N - m m) / (K - 1);  v_ch = (sum_j [0 < m_j < 1] vs_j) / 16 in j order;
             var = (v_r, v_g, v_b, (v_r + v_g) + v_b) rounded to f32.  numpy's f64 +, *, / are IEEE, so these are the
             device's bits.
  atrous_var the variance-guided filter in f64 (or, to size the tolerance, f32): denoise_ref.atrous with
             E_colour = |c_p - c_q|^2 * (1 / (sigma_c^2 g_p + 1e-10)), g_p the 3 x 3 tent of the variance at the
             level's step, and v'_p = sum w^2 v_q / (sum w)^2."""
import numpy as np

import denoise_ref as ref

K3 = (1 / 4, 1 / 2, 1 / 4)

# Largest |f32 restatement - f64 restatement| of the filter's linear output over denoise_ref.SIZES x LEVELS x
# SIGMA_CASES on synthetic() inputs with synthetic_var() variances, and the largest relative difference of the filtered
# variance; measured by tests/test_accum_abi.py::test_d32v_is_the_recorded_value (which recomputes them).
D32V = 8.1e-7
D32V_VAR_REL = 1.4e-5


class Accum:
    def __init__(self, width, height):
        self.shape = (height, width, 4, 3)
        self.reset()

    def reset(self):
        self.K, self.N = 0, 0
        self.S = self.Q = None

    def add_sub(self, sub, n):
        m = np.asarray(sub, dtype=np.float64).reshape(self.shape)
        nm = np.float64(n) * m
        if self.K == 0:
            self.S, self.Q = nm, nm * m
        else:
            self.S, self.Q = self.S + nm, self.Q + nm * m
        self.K += 1
        self.N += n

    def sub(self):
        return self.S / np.float64(self.N)

    def var(self):
        assert self.K >= 2
        m = self.sub()
        d = self.Q / np.float64(self.N) - m * m
        vs = np.where(d > 0.0, d, 0.0) / np.float64(self.K - 1)
        inside = (m > 0.0) & (m < 1.0)
        acc = np.zeros(m.shape[:2] + (3,))
        for j in range(4):
            acc = acc + np.where(inside[:, :, j], vs[:, :, j], 0.0)
        v = acc / 16.0
        out = np.zeros(m.shape[:2] + (4,), dtype=np.float32)
        out[..., :3] = v.astype(np.float32)
        out[..., 3] = ((v[..., 0] + v[..., 1]) + v[..., 2]).astype(np.float32)
        return out

    def rgb(self):
        return ref.rgb8_of(c_of(self.sub()))


def c_of(sub):
    """k_finalize_f64's pixel colour in f64: sum_j clamp(sub_j, 0, 1) * 0.25 (not rounded to f32)."""
    sub = np.asarray(sub, dtype=np.float64)
    px = np.zeros(sub.shape[:2] + (3,))
    for j in range(4):
        px = px + np.clip(sub[:, :, j], 0.0, 1.0) * 0.25
    return px


def direct_variance(passes, ns):
    """The weighted variance of the subpixel means by a direct two-pass computation (what S and Q encode):
    sum_k n_k (m_k - mean)^2 / N / (K - 1), mean = sum_k n_k m_k / N."""
    m = np.stack([np.asarray(p, dtype=np.float64) for p in passes])
    n = np.asarray(ns, dtype=np.float64).reshape((-1,) + (1,) * (m.ndim - 1))
    mean = (n * m).sum(0) / n.sum()
    return (n * (m - mean) ** 2).sum(0) / n.sum() / (len(passes) - 1), mean


def atrous_var(sub, feat, var, levels, sigma_c, sigma_n, sigma_z, sigma_a, dtype=np.float64):
    """(filtered linear colour [h, w, 3], filtered variance [h, w]) in `dtype` arithmetic. var: [h, w, 4] (only
    [..., 3] is used) or [h, w]."""
    T = dtype
    c = ref.c0_of(sub).astype(T)
    var = np.asarray(var)
    v = np.maximum((var[..., 3] if var.ndim == 3 else var).astype(np.float32), np.float32(0)).astype(T)
    f = np.asarray(feat).astype(T)
    h, w = c.shape[:2]
    n, z, a, k = f[..., 0:3], f[..., 3], f[..., 4:7], f[..., 7]

    def windows(s, dy, dx):
        y0, y1 = max(0, -s * dy), min(h, h - s * dy)
        x0, x1 = max(0, -s * dx), min(w, w - s * dx)
        if y0 >= y1 or x0 >= x1:
            return None
        return (slice(y0, y1), slice(x0, x1)), (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))

    for i in range(levels):
        s = 1 << i
        gs = np.zeros((h, w), dtype=T)
        gw = np.zeros((h, w), dtype=T)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                pq = windows(s, dy, dx)
                if pq is None:
                    continue
                P, Q = pq
                kk = T(K3[dx + 1]) * T(K3[dy + 1])
                gs[P] += kk * v[Q]
                gw[P] += kk
        with np.errstate(over="ignore"):
            inv_c = T(1) / (T(sigma_c) * T(sigma_c) * (gs / gw) + T(1e-10)) if sigma_c > 0 else None
        num = np.zeros((h, w, 3), dtype=T)
        den = np.zeros((h, w), dtype=T)
        numv = np.zeros((h, w), dtype=T)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                pq = windows(s, dy, dx)
                if pq is None:
                    continue
                P, Q = pq
                E = np.zeros(c[P].shape[:2], dtype=T)
                if sigma_c > 0:
                    E = E + ((c[P] - c[Q]) ** 2).sum(-1) * inv_c[P]
                if sigma_n > 0:
                    E = E + ((n[P] - n[Q]) ** 2).sum(-1) / (T(sigma_n) * T(sigma_n))
                if sigma_z > 0:
                    rz = (z[P] - z[Q]) / (z[P] + z[Q] + T(1e-20))
                    E = E + rz * rz / (T(sigma_z) * T(sigma_z))
                if sigma_a > 0:
                    E = E + (((a[P] - a[Q]) ** 2).sum(-1) + (k[P] - k[Q]) ** 2) / (T(sigma_a) * T(sigma_a))
                with np.errstate(under="ignore"):
                    wgt = T(ref.H5[dx + 2]) * T(ref.H5[dy + 2]) * np.exp(-E)
                    num[P] += wgt[..., None] * c[Q]
                    den[P] += wgt
                    numv[P] += (wgt * wgt) * v[Q]
        c = num / den[..., None]
        v = numv / (den * den)
        assert c.dtype == T and v.dtype == T
    return c, v


def synthetic_var(width, height, seed=4321):
    """[h, w, 4] f32 variances with [..., 3] drawn log-uniformly from [1e-4, 1e-1] (the reciprocal stays well
    conditioned) and the channels a third of it each."""
    rng = np.random.default_rng(seed + 1000 * width + height)
    tot = np.exp(rng.uniform(np.log(1e-4), np.log(1e-1), size=(height, width)))
    var = np.zeros((height, width, 4), dtype=np.float32)
    var[..., :3] = (tot / 3.0)[..., None]
    var[..., 3] = tot
    return var


def synthetic_passes(width, height, ns=(1, 2, 5), seed=99):
    """Passes of subpixel means in [-0.2, 1.6] (the clamp's indicator matters at both ends), one per entry of ns."""
    rng = np.random.default_rng(seed + 1000 * width + height)
    return [rng.uniform(-0.2, 1.6, size=(height, width, 4, 3)) for _ in ns]


def measure_d32v():
    """(largest absolute f32-f64 difference of the linear colour, largest relative one of the filtered variance)."""
    worst_c, worst_v = 0.0, 0.0
    for w, h in ref.SIZES:
        sub, feat = ref.synthetic(w, h)
        var = synthetic_var(w, h)
        for levels in ref.LEVELS:
            for sig in ref.SIGMA_CASES:
                c32, v32 = atrous_var(sub, feat, var, levels, dtype=np.float32, **sig)
                c64, v64 = atrous_var(sub, feat, var, levels, dtype=np.float64, **sig)
                worst_c = max(worst_c, float(np.abs(c32.astype(np.float64) - c64).max()))
                worst_v = max(worst_v, float((np.abs(v32.astype(np.float64) - v64) / v64).max()))
    return worst_c, worst_v


def pass_seed(seed, k):
    """render_progressive's seed of pass k."""
    return (seed + k * 0x9E3779B97F4A7C15) % (1 << 64)
