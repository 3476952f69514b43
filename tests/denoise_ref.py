"""numpy restatement of the denoiser (include/rt_ffi.h rt_denoise) — TEST INFRASTRUCTURE ONLY.

The single source of truth of the GPU tests: the a-trous filter in f64 (or, to size the tolerance, in f32), the
feature buffers from centre rays traced by the CPU oracle, and the synthetic inputs both share.

  c0_p   = sum_j clamp(sub_j, 0, 1) * 0.25 (f64, k_finalize_f64's sum), rounded to f32
  level i, s = 2^i, taps q = p + s (dx, dy), dx, dy in -2..2, inside the image, row-major (dy, dx) order:
  E(p,q) = |c_p - c_q|^2 / (sigma_c 2^-i)^2 + |n_p - n_q|^2 / sigma_n^2
         + ((z_p - z_q) / (z_p + z_q + 1e-20))^2 / sigma_z^2 + (|a_p - a_q|^2 + (k_p - k_q)^2) / sigma_a^2
  w      = h[dx + 2] h[dy + 2] exp(-E),   c'_p = sum_q w c_q / sum_q w,   h = (1/16, 1/4, 3/8, 1/4, 1/16)
A sigma <= 0 drops its term."""
import numpy as np

H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)

# The filter test's cases (tests/test_gpu_denoise.py::test_filter_matches_restatement)
SIZES = ((1, 1), (5, 3), (16, 16), (67, 35), (300, 20))  # (width, height)
LEVELS = (1, 3, 5)
SIGMA_ON = dict(sigma_c=0.8, sigma_n=1.0, sigma_z=1.0, sigma_a=1.0)
SIGMA_CASES = (SIGMA_ON, dict(SIGMA_ON, sigma_c=0.0), dict(SIGMA_ON, sigma_n=0.0), dict(SIGMA_ON, sigma_z=-1.0),
               dict(SIGMA_ON, sigma_a=-1.0))
# Largest |f32 restatement - f64 restatement| of the linear output over SIZES x LEVELS x SIGMA_CASES on synthetic()
# inputs, measured by tests/test_denoise_abi.py::test_d32_is_the_recorded_value (which recomputes it).
D32 = 8.3e-7


def c0_of(sub):
    """[h, w, 4, 3] f64 -> [h, w, 3] f64, the f32-rounded clamp-then-average."""
    sub = np.asarray(sub, dtype=np.float64)
    px = np.zeros(sub.shape[:2] + (3,))
    for j in range(4):
        px = px + np.clip(sub[:, :, j], 0.0, 1.0) * 0.25
    return px.astype(np.float32).astype(np.float64)


def atrous(sub, feat, levels, sigma_c, sigma_n, sigma_z, sigma_a, dtype=np.float64):
    """The filtered linear colour [h, w, 3] in `dtype` arithmetic."""
    T = dtype
    c = c0_of(sub).astype(T)
    f = np.asarray(feat).astype(T)
    h, w = c.shape[:2]
    n, z, a, k = f[..., 0:3], f[..., 3], f[..., 4:7], f[..., 7]
    for i in range(levels):
        s = 1 << i
        num = np.zeros((h, w, 3), dtype=T)
        den = np.zeros((h, w), dtype=T)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                y0, y1 = max(0, -s * dy), min(h, h - s * dy)
                x0, x1 = max(0, -s * dx), min(w, w - s * dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                E = np.zeros((y1 - y0, x1 - x0), dtype=T)
                if sigma_c > 0:
                    sc = T(sigma_c) * T(2.0 ** -i)
                    E = E + ((c[P] - c[Q]) ** 2).sum(-1) / (sc * sc)
                if sigma_n > 0:
                    E = E + ((n[P] - n[Q]) ** 2).sum(-1) / (T(sigma_n) * T(sigma_n))
                if sigma_z > 0:
                    rz = (z[P] - z[Q]) / (z[P] + z[Q] + T(1e-20))
                    E = E + rz * rz / (T(sigma_z) * T(sigma_z))
                if sigma_a > 0:
                    E = E + (((a[P] - a[Q]) ** 2).sum(-1) + (k[P] - k[Q]) ** 2) / (T(sigma_a) * T(sigma_a))
                wgt = T(H5[dx + 2]) * T(H5[dy + 2]) * np.exp(-E)
                num[P] += wgt[..., None] * c[Q]
                den[P] += wgt
        c = num / den[..., None]
        assert c.dtype == T
    return c


def rgb8_of(lin):
    """gamma_correct + `as u8` (server.rs:366-368, :187-189) of a linear image."""
    v = np.clip(np.asarray(lin, dtype=np.float64), 0.0, 1.0) ** (1.0 / 2.2) * 255.0 + 0.5
    return np.clip(np.floor(v), 0, 255).astype(np.uint8)


def synthetic(width, height, seed=1234):
    """sub in [0, 1.5] (the clamp matters), random unit normals, positive depths, random albedo, coverage drawn
    from {0, 1/4, 1/2, 3/4, 1}."""
    rng = np.random.default_rng(seed + 1000 * width + height)
    sub = rng.uniform(0.0, 1.5, size=(height, width, 4, 3))
    nrm = rng.normal(size=(height, width, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    feat = np.zeros((height, width, 8), dtype=np.float32)
    feat[..., 0:3] = nrm
    feat[..., 3] = rng.uniform(0.5, 300.0, size=(height, width))
    feat[..., 4:7] = rng.uniform(0.0, 1.0, size=(height, width, 3))
    feat[..., 7] = rng.integers(0, 5, size=(height, width)) * 0.25
    return sub, feat


def measure_d32():
    worst = 0.0
    for w, h in SIZES:
        sub, feat = synthetic(w, h)
        for levels in LEVELS:
            for sig in SIGMA_CASES:
                d = np.abs(atrous(sub, feat, levels, dtype=np.float32, **sig).astype(np.float64) -
                           atrous(sub, feat, levels, dtype=np.float64, **sig))
                worst = max(worst, float(d.max()))
    return worst


# Feature buffers from the oracle ---------------------------------------------------------------------------

def camera_of(toml_path):
    import tomli

    with open(toml_path, "rb") as f:
        cam = tomli.load(f)["camera"]
    return np.array(cam["pos"], dtype=np.float64), np.array(cam["dir"], dtype=np.float64)


def centre_rays(cam_pos, cam_dir, width, height):
    """The four tent-centre camera rays per pixel (server.rs:328-357 with dx = dy = 0, y = height - row - 1), in f64,
    operation by operation: origins, dirs [height * width * 4, 3], subpixel j = 2 sy + sx."""
    w, h = float(width), float(height)
    cx = np.array([w * 0.5135 / h, 0.0, 0.0])
    cr = np.array([cx[1] * cam_dir[2] - cx[2] * cam_dir[1], cx[2] * cam_dir[0] - cx[0] * cam_dir[2],
                   cx[0] * cam_dir[1] - cx[1] * cam_dir[0]])
    cy = cr / np.sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]) * 0.5135
    row, x, j = np.meshgrid(np.arange(height), np.arange(width), np.arange(4), indexing="ij")
    sx, sy = (j & 1).astype(np.float64), (j >> 1).astype(np.float64)
    y = (height - row - 1).astype(np.float64)
    fx = ((sx + 0.5 + 0.0) / 2.0 + x.astype(np.float64)) / w - 0.5
    fy = ((sy + 0.5 + 0.0) / 2.0 + y) / h - 0.5
    d = (cx[None, :] * fx.reshape(-1, 1) + cy[None, :] * fy.reshape(-1, 1)) + cam_dir[None, :]
    d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    o = np.broadcast_to(cam_pos, d.shape).copy()
    return o, d


def trace_parallel(oracle_scene, origins, dirs, workers=None):
    """OracleScene.trace over chunks of the rays on a few threads (the nearest-triangle oracle tests every triangle
    per ray): t, ids, pos, normal."""
    import os
    from concurrent.futures import ThreadPoolExecutor

    workers = workers or min(16, os.cpu_count() or 1)
    cuts = np.linspace(0, origins.shape[0], 4 * workers + 1).astype(int)
    with ThreadPoolExecutor(workers) as ex:
        parts = list(ex.map(lambda ab: oracle_scene.trace(origins[ab[0]:ab[1]], dirs[ab[0]:ab[1]]),
                            [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


def features_from_hits(t, ids, nrm, width, height):
    """normal [h, w, 3], depth [h, w], coverage [h, w] (means over the rays that hit, (s0 + s1) + (s2 + s3)) and the
    hit objects [h, w, 4]."""
    ids = ids.reshape(height, width, 4)
    hit = (ids >= 0)
    t = np.where(hit, t.reshape(height, width, 4), 0.0)
    nrm = np.where(hit[..., None], nrm.reshape(height, width, 4, 3), 0.0)
    cnt = hit.sum(-1).astype(np.float64)
    div = np.maximum(cnt, 1.0)
    q = lambda v: ((v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3]))
    return q(nrm) / div[..., None], q(t) / div, cnt * 0.25, ids


def nudged(dirs):
    """Each direction component moved one ulp (away from zero on even rays, towards it on odd ones)."""
    even = np.arange(dirs.shape[0])[:, None] % 2 == 0
    return np.nextafter(dirs, np.where(even, 2.0 * dirs, 0.0))
