"""numpy + oracle restatement of camera views and accumulator reprojection (include/rt_ffi.h rt_scene_view,
rt_accum_reproject) — TEST INFRASTRUCTURE ONLY.

  frame / centre_rays  the camera frame of a view and its tent-centre rays, operation by operation in f64.
  classify             steps 1-6 of rt_accum_reproject per dst subpixel: the oracle traces the dst view's centre rays
                       and answers mutually_visible; everything between is numpy in the header's operation order.
  reproject            the seeded S, Q and counts from src's S, Q and per-pixel counts.
  Accum                accum_ref.Accum with per-pixel counts and the seeded state.
numpy's f64 +, -, *, / and floor are IEEE, so these are the device's bits wherever the oracle's hits are the device's
(tests/test_gpu_queries.py pins those ray by ray)."""
import os

import numpy as np

import denoise_ref

REF_RIGHT, REF_FOV = (1.0, 0.0, 0.0), 0.5135
CLASSES = ("miss", "non_diffuse", "behind", "out_of_frame", "back_side", "occluded")

# the camera moves of the issue, relative to a scene's own camera
MOVE_A = dict(dpos=(14.0, 6.0, -40.0), ddir=(-0.10, -0.05, 0.0))
MOVE_B = dict(dpos=(-12.0, -5.0, 30.0), ddir=(0.15, 0.06, 0.0))


def view(pos, dir, right=REF_RIGHT, fov=REF_FOV):
    return dict(pos=np.array(pos, dtype=np.float64), dir=np.array(dir, dtype=np.float64),
                right=np.array(right, dtype=np.float64), fov=float(fov))


def scene_view(toml_path, move=None):
    """The scene's own camera as a view, moved by move = dict(dpos, ddir) when given."""
    pos, d = denoise_ref.camera_of(toml_path)
    if move is not None:
        pos, d = pos + np.array(move["dpos"]), d + np.array(move["ddir"])
    return view(pos, d)


def as_kwargs(v):
    """A view as Scene.view's keyword arguments."""
    return dict(pos=tuple(v["pos"].tolist()), dir=tuple(v["dir"].tolist()), right=tuple(v["right"].tolist()),
                fov=v["fov"])


def moved_toml(toml_path, v, out_dir):
    """The scene's text with the view's [camera] (right and fov must be the reference's), written to out_dir; load it
    with the original scene's assets directory."""
    assert tuple(v["right"]) == REF_RIGHT and v["fov"] == REF_FOV
    text = open(toml_path).read()
    head, rest = text.split("[camera]", 1)
    lines = rest.split("\n")
    body = [ln for ln in lines[1:] if not (ln.startswith("pos") or ln.startswith("dir"))]
    cam = "[camera]\npos = [%s]\ndir = [%s]\n" % (", ".join(repr(float(x)) for x in v["pos"]),
                                                  ", ".join(repr(float(x)) for x in v["dir"]))
    out = os.path.join(str(out_dir), "moved_" + os.path.basename(toml_path))
    with open(out, "w") as f:
        f.write(head + cam + "\n".join(body))
    return out, os.path.join(os.path.dirname(os.path.abspath(toml_path)), "assets")


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _dot_rows(v, a):
    """The device's dot: (x x' + y y') + z z', per row of v."""
    return (v[..., 0] * a[0] + v[..., 1] * a[1]) + v[..., 2] * a[2]


def frame(v, width, height):
    """s = w * fov / h; cx = right * s; cy = norm(cross(cx, dir)) * fov."""
    w, h = float(width), float(height)
    s = w * v["fov"] / h
    cx = v["right"] * s
    cr = _cross(cx, v["dir"])
    cy = cr / np.sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]) * v["fov"]
    return cx, cy


def centre_rays(v, width, height):
    """denoise_ref.centre_rays for a view: origins, dirs [height * width * 4, 3], subpixel j = 2 sy + sx."""
    w, h = float(width), float(height)
    cx, cy = frame(v, width, height)
    row, x, j = np.meshgrid(np.arange(height), np.arange(width), np.arange(4), indexing="ij")
    sx, sy = (j & 1).astype(np.float64), (j >> 1).astype(np.float64)
    y = (height - row - 1).astype(np.float64)
    fx = ((sx + 0.5 + 0.0) / 2.0 + x.astype(np.float64)) / w - 0.5
    fy = ((sy + 0.5 + 0.0) / 2.0 + y) / h - 0.5
    d = (cx[None, :] * fx.reshape(-1, 1) + cy[None, :] * fy.reshape(-1, 1)) + v["dir"][None, :]
    d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    return np.broadcast_to(v["pos"], d.shape).copy(), d


def src_basis(v, width, height):
    """A, B, C: the rows of the inverse of (cx_s | cy_s | dir_s), by cofactors."""
    cx, cy = frame(v, width, height)
    yd, dx, xy = _cross(cy, v["dir"]), _cross(v["dir"], cx), _cross(cx, cy)
    D = (cx[0] * yd[0] + cx[1] * yd[1]) + cx[2] * yd[2]
    return yd / D, dx / D, xy / D


def brdf_kinds(toml_path):
    """Per object: 0 diffuse, 1 specular, 2 phong."""
    import tomli

    with open(toml_path, "rb") as f:
        spec = tomli.load(f)
    return np.array([{"diffuse": 0, "specular": 1, "phong": 2}[o["brdf"]["type"]] for o in spec["objects"]])


def classify(oracle_scene, kinds, dst, src, width, height):
    """Steps 1-6 per dst subpixel. Returns a dict: ok [h, w, 4] bool, q [h, w, 4] source pixel ids and jp [h, w, 4]
    source subpixels (0 where not ok), cls [h, w, 4] int (-1 valid, else the index in CLASSES of the first step that
    failed), and what the device can be cross-checked on: rays (o, d), hits (ids, x, n) and the shadow segments'
    start points with their answer (seg [n, 3], vis [n])."""
    w, h = float(width), float(height)
    o, d = centre_rays(dst, width, height)
    t, ids, x, n = denoise_ref.trace_parallel(oracle_scene, o, d)
    nsub = o.shape[0]
    cls = np.full(nsub, -1, dtype=np.int64)
    cls[ids < 0] = 0
    hit = ids >= 0
    cls[hit & (np.asarray(kinds)[np.maximum(ids, 0)] != 0)] = 1
    A, B, C = src_basis(src, width, height)
    pos_s = src["pos"]
    with np.errstate(all="ignore"):
        v = x - pos_s[None, :]
        al, be, ga = _dot_rows(v, A), _dot_rows(v, B), _dot_rows(v, C)
        cls[(cls < 0) & ~(ga > 0.0)] = 2
        fx = (al / ga + 0.5) * w
        fy = (be / ga + 0.5) * h
        inside = (fx >= 0.0) & (fx < w) & (fy >= 0.0) & (fy < h)
    cls[(cls < 0) & ~inside] = 3
    live = cls < 0
    fx, fy = np.where(live, fx, 0.0), np.where(live, fy, 0.0)
    col, yref = np.floor(fx), np.floor(fy)
    sxp, syp = np.floor((fx - col) * 2.0), np.floor((fy - yref) * 2.0)
    row = (height - 1) - yref.astype(np.int64)
    q = row * width + col.astype(np.int64)
    jp = 2 * syp.astype(np.int64) + sxp.astype(np.int64)
    back = pos_s[None, :] - x
    side = (n[:, 0] * back[:, 0] + n[:, 1] * back[:, 1]) + n[:, 2] * back[:, 2]
    cls[(cls < 0) & ~(side > 0.0)] = 4
    ask = np.flatnonzero(cls < 0)
    vis = np.zeros(0, dtype=bool)
    if ask.size:
        vis = oracle_scene.visible(x[ask], np.broadcast_to(pos_s, (ask.size, 3)).copy())
        cls[ask[~vis]] = 5
    ok = cls < 0
    shape = (height, width, 4)
    return dict(ok=ok.reshape(shape), q=np.where(ok, q, 0).reshape(shape), jp=np.where(ok, jp, 0).reshape(shape),
                cls=cls.reshape(shape), rays=(o, d), hits=(ids, x, n), seg=x[ask], vis=vis, asked=ask)


def class_counts(c):
    return {name: int((c["cls"] == k).sum()) for k, name in enumerate(CLASSES)}


def reproject(S, Q, K, N, c, max_n):
    """src sums S, Q [h, w, 4, 3] and counts K, N [h, w] (integers) -> dst (S, Q, K, N, n_valid)."""
    h, w = c["ok"].shape[:2]
    valid = c["ok"].all(-1)
    qpix, jp = c["q"], c["jp"]
    Kq = np.asarray(K, dtype=np.int64).reshape(-1)[qpix]          # [h, w, 4]
    Nq = np.asarray(N, dtype=np.int64).reshape(-1)[qpix]
    Nq_safe = np.maximum(Nq, 1)
    valid &= (Nq > 0).all(-1)
    Np = np.minimum(np.int64(max_n), Nq.min(-1))
    Kj = (Kq * Np[..., None] + Nq_safe - 1) // Nq_safe
    Kp = np.maximum(np.int64(2), Kj.min(-1))
    Ss = np.asarray(S, dtype=np.float64).reshape(-1, 4, 3)[qpix, jp]  # [h, w, 4, 3]
    Qs = np.asarray(Q, dtype=np.float64).reshape(-1, 4, 3)[qpix, jp]
    np_d, nq_d = Np.astype(np.float64)[..., None, None], Nq_safe.astype(np.float64)[..., None]
    Sd = np.where(valid[..., None, None], np_d * (Ss / nq_d), 0.0)
    Qd = np.where(valid[..., None, None], np_d * (Qs / nq_d), 0.0)
    return Sd, Qd, np.where(valid, Kp, 0).astype(np.uint32), np.where(valid, Np, 0).astype(np.uint32), int(valid.sum())


class Accum:
    """accum_ref.Accum with the per-pixel counts of DESIGN.md §13 and the seeded state of §14."""

    def __init__(self, width, height):
        self.shape = (height, width, 4, 3)
        self.S = np.zeros(self.shape)
        self.Q = np.zeros(self.shape)
        self.K = np.zeros((height, width), dtype=np.int64)
        self.N = np.zeros((height, width), dtype=np.int64)
        self.fresh = True  # neither a pass nor a seed yet: the next pass stores

    def add_sub(self, sub, n):
        m = np.asarray(sub, dtype=np.float64).reshape(self.shape)
        nm = np.float64(n) * m
        if self.fresh:
            self.S, self.Q = nm, nm * m
        else:
            self.S, self.Q = self.S + nm, self.Q + nm * m
        self.fresh = False
        self.K = self.K + 1
        self.N = self.N + n

    def add_sub_pixels(self, pixels, sub, n):
        px = np.asarray(pixels, dtype=np.int64)
        m = np.asarray(sub, dtype=np.float64).reshape(-1, 4, 3)
        nm = np.float64(n) * m
        S, Q = self.S.reshape(-1, 4, 3).copy(), self.Q.reshape(-1, 4, 3).copy()
        S[px] = S[px] + nm
        Q[px] = Q[px] + nm * m
        self.S, self.Q = S.reshape(self.shape), Q.reshape(self.shape)
        K, N = self.K.reshape(-1).copy(), self.N.reshape(-1).copy()
        K[px] += 1
        N[px] += n
        self.K, self.N = K.reshape(self.K.shape), N.reshape(self.N.shape)

    def seed(self, S, Q, K, N):
        self.S, self.Q = S.copy(), Q.copy()
        self.K, self.N = K.astype(np.int64), N.astype(np.int64)
        self.fresh = False

    def sub(self):
        return self.S / self.N.astype(np.float64)[..., None, None]

    def var(self):
        Nd = self.N.astype(np.float64)[..., None, None]
        m = self.S / Nd
        dq = self.Q / Nd - m * m
        vs = np.where(dq > 0.0, dq, 0.0) / (self.K.astype(np.float64) - 1.0)[..., None, None]
        inside = (m > 0.0) & (m < 1.0)
        acc = np.zeros(m.shape[:2] + (3,))
        for j in range(4):
            acc = acc + np.where(inside[:, :, j], vs[:, :, j], 0.0)
        v = acc / 16.0
        out = np.zeros(m.shape[:2] + (4,), dtype=np.float32)
        out[..., :3] = v.astype(np.float32)
        out[..., 3] = ((v[..., 0] + v[..., 1]) + v[..., 2]).astype(np.float32)
        return out


def pixel_colour(sub):
    """k_finalize_f64's linear pixel colour: sum_j clamp(sub_j, 0, 1) * 0.25."""
    sub = np.asarray(sub, dtype=np.float64)
    px = np.zeros(sub.shape[:2] + (3,))
    for j in range(4):
        px = px + np.clip(sub[:, :, j], 0.0, 1.0) * 0.25
    return px


def quality_figures(sub_hist, sub_empty, sub_ref, valid):
    """Linear RMSE against sub_ref of a frame that started from reprojected history and of one that started empty
    (the same new passes), over all pixels and over the valid ones, and the ratios hist / empty."""
    ch, ce, cr = pixel_colour(sub_hist), pixel_colour(sub_empty), pixel_colour(sub_ref)
    rmse = lambda a, m: float(np.sqrt(((a - cr)[m] ** 2).mean()))
    every = np.ones_like(valid)
    out = dict(hist_all=rmse(ch, every), empty_all=rmse(ce, every), hist_valid=rmse(ch, valid),
               empty_valid=rmse(ce, valid))
    out["ratio_all"] = out["hist_all"] / out["empty_all"]
    out["ratio_valid"] = out["hist_valid"] / out["empty_valid"]
    return out


def toml_of(cam_pos, cam_dir, objects):
    """Scene text for Scene.from_desc object dicts (spheres and planes; diffuse or specular)."""
    out = ["[camera]", "pos = %r" % [float(x) for x in cam_pos], "dir = %r" % [float(x) for x in cam_dir], ""]
    for o in objects:
        out.append("[[objects]]")
        if "emitted" in o:
            out.append("emitted = %r" % [float(x) for x in o["emitted"]])
        k = [float(x) for x in o["k"]]
        out.append('brdf = { type = "diffuse", kd = %r }' % k if o.get("brdf_kind", 0) == 0
                   else 'brdf = { type = "specular", ks = %r }' % k)
        p = [float(x) for x in o["pos"]]
        if o["geom_kind"] == 0:
            out.append('geometry = { type = "sphere", pos = %r, r = %r }' % (p, float(o["r"])))
        else:
            out.append('geometry = { type = "plane", pos = %r, n = %r }' % (p, [float(x) for x in o["n"]]))
        out.append("")
    return "\n".join(out)
