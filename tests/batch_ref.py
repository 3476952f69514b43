"""numpy restatement of batched error-target passes (include/rt_ffi.h rt_accum_plan, rt_accum_add_passes; DESIGN.md
§17) — TEST INFRASTRUCTURE ONLY. Built on adapt_ref.

  wanted      the pass count each pixel of the selection wants before the frame cap, operation by operation as
              k_plan_count: r = g / (thr thr), need = N_p r - N_p, x = (gain need) / n, c = C if x >= C else
              max(1, ceil(x)), then the max_n clip in integers.
  cap_of      the frame cap: the largest C' in 1 .. C with sum_c H[c] min(c, C') <= width * height.
  plan        rt_accum_plan on a restated accumulator: ids (the selection's), final counts, unit total, largest count.
  offsets     the exclusive prefix sum of the counts: unit-group off[e] + i is pass i of entry e.
  add_runs    the run merge: entry e's counts[e] units, in pass order, with add_sub_pixels' expression."""
import numpy as np

import accum_ref as aref
import adapt_ref as ad

PASSES_MAX = 16


def check_args(n, gain, max_passes):
    g = np.float32(gain)
    return n >= 1 and bool(g > 0) and bool(g <= 1) and 1 <= max_passes <= PASSES_MAX


def wanted(var, sub, n_p, abs_tol, rel_tol, max_n, n, gain, max_passes):
    """[h, w] int64: 0 where the selection does not list the pixel, else the wanted count in 1 .. max_passes."""
    assert check_args(n, gain, max_passes)
    g = ad.tent(np.asarray(var, dtype=np.float32)[..., 3].astype(np.float64))
    c = aref.c_of(sub)
    y = (c[..., 0] + c[..., 1]) + c[..., 2]
    thr = (np.float64(np.float32(rel_tol)) * y) / 3.0 + np.float64(np.float32(abs_tol))
    act = ad.select_mask(var, sub, n_p, abs_tol, rel_tol, max_n)
    Ni = np.asarray(n_p).astype(np.int64)
    Np = Ni.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = g / (thr * thr)
        need = Np * r - Np
        x = (np.float64(np.float32(gain)) * need) / np.float64(n)
    C = int(max_passes)
    big = x >= np.float64(C)
    mid = (x > 1.0) & ~big
    cnt = np.ones(x.shape, dtype=np.int64)
    cnt[mid] = np.ceil(x[mid]).astype(np.int64)
    cnt[big] = C
    if max_n > 0:
        room = (np.int64(max_n) - Ni + np.int64(n) - 1) // np.int64(n)
        cnt = np.minimum(cnt, room)
    return np.where(act, cnt, 0)


def cap_of(want, npix, max_passes):
    """The largest C' in 1 .. max_passes whose unit total fits npix (C' = 1 always fits), and that total. Every C'
    at or above the largest wanted count leaves the same counts: C' is reported as the largest count it leaves."""
    w = np.asarray(want).reshape(-1)
    w = w[w > 0]
    for c1 in range(int(max_passes), 0, -1):
        units = int(np.minimum(w, c1).sum())
        if units <= npix:
            break
    return (min(c1, int(w.max())) if w.size else 0), units


def plan_of(want, max_passes):
    """(ids uint32 ascending, counts uint8, units, passes) of a wanted map."""
    want = np.asarray(want)
    flat = want.reshape(-1)
    ids = np.flatnonzero(flat > 0).astype(np.uint32)
    c1, units = cap_of(flat, flat.size, max_passes)
    counts = np.minimum(flat[ids], c1).astype(np.uint8)
    assert int(counts.astype(np.int64).sum()) == (units if ids.size else 0)
    return ids, counts, (units if ids.size else 0), (int(counts.max()) if ids.size else 0)


def plan(acc, abs_tol, rel_tol=0.0, max_n=0, n=4, gain=1.0, max_passes=PASSES_MAX):
    """rt_accum_plan on a restated accumulator (adapt_ref.Accum)."""
    return plan_of(wanted(acc.var(), acc.sub(), acc.counts()[1], abs_tol, rel_tol, max_n, n, gain, max_passes), max_passes)


def offsets(counts):
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    return np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.int64) if c.size else np.zeros(0, dtype=np.int64)


def add_runs(acc, pixels, counts, units_sub, n):
    """The run merge on a restated accumulator: units_sub[off[e] + i] is pass i of pixel pixels[e]. One sparse merge
    per pass index over the entries that have that pass: the elements of one pixel see their passes in order."""
    px = np.asarray(pixels, dtype=np.int64).reshape(-1)
    ct = np.asarray(counts, dtype=np.int64).reshape(-1)
    m = np.asarray(units_sub, dtype=np.float64).reshape(-1, 4, 3)
    off = offsets(ct)
    assert m.shape[0] == int(ct.sum())
    for i in range(int(ct.max()) if ct.size else 0):
        has = ct > i
        acc.add_sub_pixels(px[has], m[off[has] + i], n)
