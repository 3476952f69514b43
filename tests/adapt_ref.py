"""numpy restatement of rendering to a per-pixel error target (include/rt_ffi.h rt_accum_add_sub_pixels, rt_accum_counts,
rt_accum_select) — TEST INFRASTRUCTURE ONLY.

  Accum    accum_ref.Accum with per-pixel counts: cnt = (K_p, N_p) comes with the first sparse merge, filled with the
           frame's (K, N); from then on a full-frame merge adds (1, n) to every pixel and a sparse merge to the listed
           ones, and sub / var use N_p and K_p - 1. Operation by operation as k_accum_add_list / k_accum_resolve_cnt.
  select   rt_accum_select's arithmetic in f64: the 3 x 3 tent of var[..., 3] in row-major (dy, dx) order, the clamped
           pixel colour's channel sum, thr = (rel_tol * y) / 3 + abs_tol, active iff g > thr * thr and N_p < max_n.
  gather   a frame's entries at a pixel list."""
import numpy as np

import accum_ref as aref

K3 = aref.K3


class Accum(aref.Accum):
    def reset(self):
        super().reset()
        self.cnt = None  # [h, w, 2] uint32 once a sparse pass has been merged

    def add_sub(self, sub, n):
        super().add_sub(sub, n)
        if self.cnt is not None:
            self.cnt = self.cnt + np.array([1, n], dtype=np.uint32)

    def add_sub_pixels(self, pixels, sub, n):
        """pixels: unique ids row * width + col; sub[len(pixels), 4, 3]."""
        assert self.K >= 2
        h, w = self.shape[:2]
        px = np.asarray(pixels, dtype=np.int64).reshape(-1)
        m = np.asarray(sub, dtype=np.float64).reshape(px.size, 4, 3)
        if self.cnt is None:
            self.cnt = np.empty((h, w, 2), dtype=np.uint32)
            self.cnt[..., 0], self.cnt[..., 1] = self.K, self.N
        nm = np.float64(n) * m
        S, Q, cnt = self.S.reshape(-1, 4, 3).copy(), self.Q.reshape(-1, 4, 3).copy(), self.cnt.reshape(-1, 2).copy()
        S[px] = S[px] + nm
        Q[px] = Q[px] + nm * m
        cnt[px] = cnt[px] + np.array([1, n], dtype=np.uint32)
        self.S, self.Q, self.cnt = S.reshape(self.shape), Q.reshape(self.shape), cnt.reshape(h, w, 2)

    def counts(self):
        h, w = self.shape[:2]
        if self.cnt is None:
            return np.full((h, w), self.K, dtype=np.uint32), np.full((h, w), self.N, dtype=np.uint32)
        return self.cnt[..., 0].copy(), self.cnt[..., 1].copy()

    def _n(self):
        return self.counts()[1].astype(np.float64)[:, :, None, None]

    def sub(self):
        return self.S / self._n()

    def var(self):
        assert self.K >= 2
        m = self.sub()
        k1 = (self.counts()[0].astype(np.float64) - 1.0)[:, :, None, None]
        d = self.Q / self._n() - m * m
        vs = np.where(d > 0.0, d, 0.0) / k1
        inside = (m > 0.0) & (m < 1.0)
        acc = np.zeros(m.shape[:2] + (3,))
        for j in range(4):
            acc = acc + np.where(inside[:, :, j], vs[:, :, j], 0.0)
        v = acc / 16.0
        out = np.zeros(m.shape[:2] + (4,), dtype=np.float32)
        out[..., :3] = v.astype(np.float32)
        out[..., 3] = ((v[..., 0] + v[..., 1]) + v[..., 2]).astype(np.float32)
        return out


def tent(v):
    """g = sum k[dx] k[dy] v_q / sum k[dx] k[dy] over the 3 x 3 neighbours inside the image, row-major (dy, dx)."""
    v = np.asarray(v, dtype=np.float64)
    h, w = v.shape
    num, den = np.zeros((h, w)), np.zeros((h, w))
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            y0, y1 = max(0, -dy), min(h, h - dy)
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            kk = np.float64(K3[dx + 1]) * np.float64(K3[dy + 1])
            num[y0:y1, x0:x1] = num[y0:y1, x0:x1] + kk * v[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            den[y0:y1, x0:x1] = den[y0:y1, x0:x1] + kk
    return num / den


def select_mask(var, sub, n_p, abs_tol, rel_tol=0.0, max_n=0):
    """The active mask [h, w]. var: [h, w, 4] f32 (the resolve's), sub = S / N_p [h, w, 4, 3], n_p [h, w] counts."""
    g = tent(np.asarray(var, dtype=np.float32)[..., 3].astype(np.float64))
    c = aref.c_of(sub)
    y = (c[..., 0] + c[..., 1]) + c[..., 2]
    thr = (np.float64(np.float32(rel_tol)) * y) / 3.0 + np.float64(np.float32(abs_tol))
    act = g > thr * thr
    if max_n > 0:
        act = act & (np.asarray(n_p).astype(np.int64) < max_n)
    return act


def select(acc, abs_tol, rel_tol=0.0, max_n=0):
    """rt_accum_select on a restated accumulator: the active ids, ascending (uint32)."""
    return np.flatnonzero(select_mask(acc.var(), acc.sub(), acc.counts()[1], abs_tol, rel_tol, max_n)).astype(np.uint32)


def gather(frame, pixels):
    """frame[h, w, ...] at the ids row * width + col: [len(pixels), ...]."""
    frame = np.asarray(frame)
    return frame.reshape((-1,) + frame.shape[2:])[np.asarray(pixels, dtype=np.int64)]
