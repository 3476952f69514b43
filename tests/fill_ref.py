"""numpy restatement of the hole fill after a reprojection (include/rt_ffi.h rt_accum_holes, rt_accum_fill; DESIGN.md
§15) — TEST INFRASTRUCTURE ONLY.

  check_args   the argument rules of period and phase.
  hole_mask    the predicate per pixel: K_p < 2, or period > 0 and (col + 3 row) mod period == phase.
  holes        rt_accum_holes on a map of K_p: the listed ids, ascending, and the count with K_p < 2.
  Accum        reproject_ref.Accum with the states of the C accumulator: seeded (by a reprojection), covered (by a
               fill), and the full-frame passes since the reprojection; may() restates which calls are accepted.
  Accum.fill   rt_accum_fill: two sparse passes over the lists above, merged operation by operation as
               k_accum_add_list (reproject_ref.Accum.add_sub_pixels).
The selection on a covered accumulator is adapt_ref.select_mask on this Accum's var(), sub() and N."""
import numpy as np

import reproject_ref as rr


def check_args(period, phase):
    """True iff rt_accum_holes / rt_accum_fill accept (period, phase)."""
    return period >= 0 and 0 <= phase < max(period, 1)


def hole_mask(K, period=0, phase=0):
    """[h, w] bool from the per-pixel pass counts K [h, w]."""
    assert check_args(period, phase)
    K = np.asarray(K)
    h, w = K.shape
    mask = K < 2
    if period > 0:
        row, col = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
        mask = mask | ((col + 3 * row) % period == phase)
    return mask


def holes(K, period=0, phase=0, cap=None):
    """(ids uint32 ascending, at most cap of them; the full count; the count with K_p < 2)."""
    ids = np.flatnonzero(hole_mask(K, period, phase)).astype(np.uint32)
    n_holes = int((np.asarray(K) < 2).sum())
    return (ids if cap is None else ids[:cap]), int(ids.size), n_holes


class Accum(rr.Accum):
    def __init__(self, width, height):
        super().__init__(width, height)
        self.seeded = False
        self.covered = False
        self.passes = 0  # full-frame passes since the reset or reprojection: rt_accum_info's K

    def reset(self):
        self.__init__(self.shape[1], self.shape[0])

    def seed(self, S, Q, K, N):
        super().seed(S, Q, K, N)
        self.seeded, self.covered, self.passes = True, False, 0

    def add_sub(self, sub, n):
        super().add_sub(sub, n)
        self.passes += 1  # (a full-frame merge keeps seeded and covered)

    def may(self, what):
        """Is the call accepted? what: "resolve", "var", "select", "sparse" (rt_accum_add_pixels and
        rt_accum_add_sub_pixels*), "reproject_src", "holes" / "fill"."""
        if what in ("holes", "fill"):
            return self.seeded
        need = 1 if what == "resolve" else 2
        return self.covered or self.passes >= need

    def holes(self, period=0, phase=0, cap=None):
        assert self.may("holes")
        return holes(self.K, period, phase, cap)

    def fill(self, render, n, period=0, phase=0, cancel_pass=None):
        """render(k, ids) -> sub[len(ids), 4, 3]: pass k (0: params->seed, 1: seed2) of the listed pixels, n its samples
        per subpixel. cancel_pass: the pass that is cancelled (it and what follows merge nothing). Returns the two
        lists' lengths."""
        assert self.may("fill") and check_args(period, phase)
        lens = [0, 0]
        for k in range(2):
            ids, count, _ = holes(self.K, period if k == 0 else 0, phase if k == 0 else 0)
            lens[k] = count
            if count == 0:
                continue
            if cancel_pass == k:
                return tuple(lens)
            self.add_sub_pixels(ids, render(k, ids), n)
        self.covered = True
        assert (self.K >= 2).all()
        return tuple(lens)
