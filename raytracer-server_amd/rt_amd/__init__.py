"""Python mirror of the reference's render interface over the C ABI (include/rt_ffi.h).

Reference interface it mirrors (SuneelFreimuth/raytracer-server):
  Scene.from_toml(path)                    <- Scene::from_toml            src/scene.rs:143-150
  sample_pixel(x, y, w, h, spp, scene)     <- sample_pixel + gamma        src/server.rs:320-368
  RenderJob(...).run(scene, w, h, spp)     <- RenderJob::run              src/server.rs:157-199
                                              (same 6-byte header + RGB8 chunk messages)
  Scene.trace_ray(origins, dirs)           <- Scene::trace_ray            src/scene.rs:272-289
Beyond the reference: render_features / denoise / render_denoised, denoised previews at low spp
(rt_render_features, rt_denoise). Accumulator / denoise_var / render_progressive: progressive refinement
(rt_accum_*, rt_denoise_var). render_pixels / Accumulator.select / add_pixels / render_to_error: rendering
to a per-pixel error target with sparse pixel-list passes (rt_render_pixels, rt_accum_select);
render_pixels(path=...) / render_pixels_path: the kernel family that runs a mesh scene's list.
Scene.view / Scene.camera / look_at / Accumulator.reproject_from / render_interactive: camera views of one scene and
an accumulator's history carried across a camera move (rt_scene_view, rt_accum_reproject).
Accumulator.holes / Accumulator.fill / render_interactive(fill_spp, refresh) / FILL_DEFAULTS: after a reprojection,
samples only for the pixels without history (rt_accum_holes, rt_accum_fill).

Everything computes on the GPU through lib/librtamd.so; there is no CPU fallback. Importing this
module without the built library raises ImportError.
"""
import ctypes
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_AMD_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "librtamd.so")

RT_OK = 0
RT_CANCELLED = 1
PASSES_MAX = 16  # RT_PASSES_MAX: the most passes per pixel of a batched render
FLAG_MIS = 1 << 0
FLAG_MEGAKERNEL = 1 << 1
FLAG_FP32 = 1 << 2
FLAG_MESH_NEAREST = 1 << 3  # Mesh::intersect without the octree (geometry.rs:886-903), BVH on the device
# query forms of Scene.diag_trace / diag_visible (include/rt_diag.h RT_DIAG_*)
DIAG_FUSED, DIAG_FUSED_G0, DIAG_SPLIT_SLOTS, DIAG_SPLIT_KIDS, DIAG_SPLIT_FLAT, DIAG_FUSED_G1 = range(6)
DIAG_FUSED_LDS = 6  # Scene.diag_vertex only: the fused megakernel's own instantiation (LDS object table, LdsCold)
DIAG_SPLIT_ROLES = 7  # Scene.diag_vertex only: the roles pool's instantiation (LdsQuerySink, slot walks)
# kernel families of a pixel-list render (include/rt_ffi.h RT_LIST_*): the automatic choice, k_render_list_f64, the
# flat-octree query pool, the role-split pool
LIST_AUTO, LIST_FUSED, LIST_FPOOL, LIST_ROLES = range(4)

BRDF_DIFFUSE, BRDF_SPECULAR, BRDF_PHONG = 0, 1, 2
GEOM_SPHERE, GEOM_PLANE, GEOM_MESH = 0, 1, 2

_D3 = ctypes.c_double * 3


class RenderParams(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("x0", ctypes.c_int32),
                ("y0", ctypes.c_int32), ("tile_w", ctypes.c_int32), ("tile_h", ctypes.c_int32),
                ("spp", ctypes.c_int32), ("seed", ctypes.c_uint64), ("flags", ctypes.c_uint32),
                ("device", ctypes.c_int32), ("row_step", ctypes.c_int32)]


class RenderStats(ctypes.Structure):
    _fields_ = [("samples", ctypes.c_int64), ("vertices", ctypes.c_int64), ("iterations", ctypes.c_int64),
                ("device_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double * 8),
                ("kernel_launches", ctypes.c_int64 * 8)]

    def as_dict(self):
        return dict(samples=self.samples, vertices=self.vertices, iterations=self.iterations,
                    device_ms=self.device_ms, kernel_ms=list(self.kernel_ms),
                    kernel_launches=list(self.kernel_launches))


class ObjectDesc(ctypes.Structure):
    _fields_ = [("emitted", _D3), ("brdf_kind", ctypes.c_int32), ("k", _D3), ("phong_kd", ctypes.c_double),
                ("phong_ks", ctypes.c_double), ("phong_power", ctypes.c_int32), ("color_d", _D3),
                ("color_s", _D3), ("geom_kind", ctypes.c_int32), ("pos", _D3), ("r", ctypes.c_double),
                ("n", _D3), ("mesh", ctypes.c_int32)]


class MeshDesc(ctypes.Structure):
    _fields_ = [("n_vertices", ctypes.c_uint32), ("vertices", ctypes.POINTER(ctypes.c_double)),
                ("n_triangles", ctypes.c_uint32), ("indices", ctypes.POINTER(ctypes.c_uint32)),
                ("bbox_min", _D3), ("bbox_max", _D3), ("surface_area", ctypes.c_double)]


class SceneDesc(ctypes.Structure):
    _fields_ = [("cam_pos", _D3), ("cam_dir", _D3), ("n_objects", ctypes.c_uint32),
                ("objects", ctypes.POINTER(ObjectDesc)), ("n_meshes", ctypes.c_uint32),
                ("meshes", ctypes.POINTER(MeshDesc))]


class View(ctypes.Structure):
    """rt_view: the 10 doubles rt_scene_view / rt_scene_get_view take."""
    _fields_ = [("pos", _D3), ("dir", _D3), ("right", _D3), ("fov", ctypes.c_double)]


_EXPORTS = ["rt_scene_load_toml", "rt_scene_create", "rt_scene_destroy", "rt_scene_info", "rt_scene_mesh",
            "rt_render", "rt_render_device", "rt_render_multi", "rt_band_plan", "rt_trace_rays", "rt_trace_rays_flags", "rt_last_error", "rt_abi_version",
            "rt_device_count", "rt_render_features", "rt_render_features_device", "rt_denoise", "rt_denoise_device",
            "rt_accum_create", "rt_accum_destroy", "rt_accum_reset", "rt_accum_info", "rt_accum_add", "rt_accum_add_sub",
            "rt_accum_add_sub_device", "rt_accum_resolve", "rt_accum_resolve_device", "rt_denoise_var",
            "rt_denoise_var_device", "rt_render_pixels", "rt_render_pixels_device", "rt_accum_add_pixels",
            "rt_accum_add_sub_pixels", "rt_accum_add_sub_pixels_device", "rt_accum_counts", "rt_accum_select",
            "rt_accum_select_device", "rt_scene_view", "rt_scene_get_view", "rt_accum_reproject", "rt_accum_holes",
            "rt_accum_holes_device", "rt_accum_fill", "rt_render_pixels_path", "rt_render_pixels_with",
            "rt_render_pixels_with_device", "rt_render_pixel_passes", "rt_render_pixel_passes_device", "rt_accum_plan",
            "rt_accum_plan_device", "rt_accum_add_passes", "rt_accum_refine", "rt_render_pixel_passes_with",
            "rt_render_pixel_passes_with_device", "rt_scene_object_bvh"]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"rt_amd: native library not built: {LIB_PATH} (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    P = ctypes.POINTER
    vp = ctypes.c_void_p
    L.rt_scene_load_toml.argtypes = [ctypes.c_char_p, ctypes.c_char_p, P(vp)]
    L.rt_scene_create.argtypes = [P(SceneDesc), P(vp)]
    L.rt_scene_destroy.argtypes = [vp]
    L.rt_scene_destroy.restype = None
    L.rt_scene_info.argtypes = [vp, P(ctypes.c_int64)]
    L.rt_scene_mesh.argtypes = [vp, ctypes.c_int32, P(ctypes.c_int64), P(ctypes.c_double), P(ctypes.c_double),
                                P(ctypes.c_double), P(ctypes.c_uint32), P(ctypes.c_int32), P(ctypes.c_int32),
                                P(ctypes.c_int32), P(ctypes.c_int32), P(ctypes.c_int32)]
    if hasattr(L, "rt_scene_object_bvh"):  # absent from libraries built before it existed (A/B variants)
        L.rt_scene_object_bvh.argtypes = [vp, P(ctypes.c_int64), P(ctypes.c_double), P(ctypes.c_int32),
                                          P(ctypes.c_int32), P(ctypes.c_int32), P(ctypes.c_int32), P(ctypes.c_int32)]
    L.rt_render.argtypes = [vp, P(RenderParams), P(ctypes.c_uint8), P(ctypes.c_double), P(ctypes.c_int32),
                            P(RenderStats)]
    L.rt_render_device.argtypes = [vp, P(RenderParams), vp, vp, vp, P(RenderStats)]
    L.rt_render_multi.argtypes = [vp, P(RenderParams), P(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32,
                                  P(ctypes.c_uint8), P(ctypes.c_int32), P(RenderStats)]
    L.rt_band_plan.restype = ctypes.c_int32
    L.rt_band_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P(ctypes.c_int32),
                               P(ctypes.c_int32)]
    L.rt_trace_rays.argtypes = [vp, ctypes.c_int32, ctypes.c_int64, P(ctypes.c_double), P(ctypes.c_double),
                                P(ctypes.c_double), P(ctypes.c_int32), P(ctypes.c_double), P(ctypes.c_double)]
    L.rt_trace_rays_flags.argtypes = [vp, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, P(ctypes.c_double),
                                      P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_int32), P(ctypes.c_double),
                                      P(ctypes.c_double)]
    F, I = ctypes.c_float, ctypes.c_int32
    L.rt_render_features.argtypes = [vp, P(RenderParams), P(F)]
    L.rt_render_features_device.argtypes = [vp, P(RenderParams), vp, vp]
    L.rt_denoise.argtypes = [I, I, I, P(ctypes.c_double), P(F), I, F, F, F, F, P(ctypes.c_uint8), P(F)]
    L.rt_denoise_device.argtypes = [I, I, I, vp, vp, I, F, F, F, F, vp, vp, vp]
    L.rt_accum_create.argtypes = [I, I, I, P(vp)]
    L.rt_accum_destroy.argtypes = [vp]
    L.rt_accum_destroy.restype = None
    L.rt_accum_reset.argtypes = [vp]
    L.rt_accum_info.argtypes = [vp, P(ctypes.c_int64)]
    L.rt_accum_add.argtypes = [vp, vp, P(RenderParams), P(ctypes.c_int32), P(RenderStats)]
    L.rt_accum_add_sub.argtypes = [vp, P(ctypes.c_double), I]
    L.rt_accum_add_sub_device.argtypes = [vp, vp, I, vp]
    L.rt_accum_resolve.argtypes = [vp, P(ctypes.c_double), P(F), P(ctypes.c_uint8)]
    L.rt_accum_resolve_device.argtypes = [vp, vp, vp, vp, vp]
    L.rt_denoise_var.argtypes = [I, I, I, P(ctypes.c_double), P(F), P(F), I, F, F, F, F, P(ctypes.c_uint8), P(F), P(F)]
    L.rt_denoise_var_device.argtypes = [I, I, I, vp, vp, vp, I, F, F, F, F, vp, vp, vp, vp]
    U32, I64, D = ctypes.c_uint32, ctypes.c_int64, ctypes.c_double
    L.rt_render_pixels.argtypes = [vp, P(RenderParams), P(U32), I64, P(ctypes.c_uint8), P(D), P(I), P(RenderStats)]
    L.rt_render_pixels_device.argtypes = [vp, P(RenderParams), vp, I64, vp, vp, vp, P(RenderStats)]
    L.rt_render_pixels_path.argtypes = [vp, P(RenderParams), I64, P(I)]
    L.rt_render_pixels_with.argtypes = [vp, P(RenderParams), P(U32), I64, I, P(ctypes.c_uint8), P(D), P(I), P(RenderStats)]
    L.rt_render_pixels_with_device.argtypes = [vp, P(RenderParams), vp, I64, I, vp, vp, vp, P(RenderStats)]
    L.rt_accum_add_pixels.argtypes = [vp, vp, P(RenderParams), P(U32), I64, P(I), P(RenderStats)]
    L.rt_accum_add_sub_pixels.argtypes = [vp, P(U32), I64, P(D), I]
    L.rt_accum_add_sub_pixels_device.argtypes = [vp, vp, I64, vp, I, vp]
    L.rt_accum_counts.argtypes = [vp, P(U32), P(U32)]
    L.rt_accum_select.argtypes = [vp, F, F, I, P(U32), I64, P(I64)]
    L.rt_accum_select_device.argtypes = [vp, F, F, I, vp, I64, P(I64), vp]
    L.rt_scene_view.argtypes = [vp, P(View), P(vp)]
    L.rt_scene_get_view.argtypes = [vp, P(View)]
    L.rt_accum_reproject.argtypes = [vp, vp, vp, vp, U32, I, P(I64)]
    L.rt_accum_holes.argtypes = [vp, I, I, P(U32), I64, P(I64), P(I64)]
    L.rt_accum_holes_device.argtypes = [vp, I, I, vp, I64, P(I64), P(I64), vp]
    L.rt_accum_fill.argtypes = [vp, vp, P(RenderParams), ctypes.c_uint64, I, I, P(I), P(RenderStats), P(I64)]
    U8, U64 = ctypes.c_uint8, ctypes.c_uint64
    L.rt_render_pixel_passes.argtypes = [vp, P(RenderParams), P(U32), P(U8), I64, P(U64), I, P(U8), P(D), P(I),
                                         P(RenderStats)]
    L.rt_render_pixel_passes_device.argtypes = [vp, P(RenderParams), vp, vp, I64, I64, P(U64), I, vp, vp, vp,
                                                P(RenderStats)]
    L.rt_render_pixel_passes_with.argtypes = [vp, P(RenderParams), P(U32), P(U8), I64, P(U64), I, I, P(U8), P(D), P(I),
                                              P(RenderStats)]
    L.rt_render_pixel_passes_with_device.argtypes = [vp, P(RenderParams), vp, vp, I64, I64, P(U64), I, I, vp, vp, vp,
                                                     P(RenderStats)]
    L.rt_accum_plan.argtypes = [vp, F, F, I, I, F, I, P(U32), P(U8), I64, P(I64), P(I64), P(I64)]
    L.rt_accum_plan_device.argtypes = [vp, F, F, I, I, F, I, vp, vp, I64, P(I64), P(I64), P(I64), vp]
    L.rt_accum_add_passes.argtypes = [vp, vp, P(RenderParams), P(U64), I, P(U32), P(U8), I64, P(I), P(RenderStats)]
    L.rt_accum_refine.argtypes = [vp, vp, P(RenderParams), F, F, I, F, P(U64), I, P(I), P(RenderStats), P(I64)]
    L.rt_last_error.restype = ctypes.c_char_p
    L.rt_last_error.argtypes = []
    L.rt_abi_version.argtypes = []
    L.rt_device_count.argtypes = []
    # diagnostics (include/rt_diag.h)
    if hasattr(L, "rt_selftest_arith"):  # absent from libraries built before it existed (A/B variants)
        L.rt_selftest_arith.argtypes = [ctypes.c_long, ctypes.c_ulonglong, P(ctypes.c_ulonglong)]
    if hasattr(L, "rt_selftest_arith_n"):
        L.rt_selftest_arith_n.argtypes = [ctypes.c_long, ctypes.c_ulonglong, P(ctypes.c_ulonglong), ctypes.c_int]
    if hasattr(L, "rt_selftest_tables"):
        L.rt_selftest_tables.argtypes = [P(ctypes.c_ulonglong), ctypes.c_int, P(ctypes.c_ulonglong)]
    if hasattr(L, "rt_debug_qcheck"):
        L.rt_debug_qcheck.argtypes = [P(ctypes.c_ulonglong)]
    if hasattr(L, "rt_debug_counters"):
        L.rt_debug_counters.argtypes = [P(ctypes.c_ulonglong)]
    if hasattr(L, "rt_debug_regions"):
        L.rt_debug_regions.argtypes = [P(ctypes.c_ulonglong)]
    if hasattr(L, "rt_debug_wave_times"):
        L.rt_debug_wave_times.argtypes = [P(ctypes.c_ulonglong), ctypes.c_int]
    if hasattr(L, "rt_debug_last_split"):
        L.rt_debug_last_split.argtypes = [P(ctypes.c_longlong)]
    if hasattr(L, "rt_diag_trace"):
        D = ctypes.c_double
        L.rt_diag_trace.argtypes = [vp, I, I, ctypes.c_uint32, ctypes.c_int64, P(D), P(D), P(D), P(I), P(I), P(D), P(D)]
        L.rt_diag_visible.argtypes = [vp, I, I, ctypes.c_uint32, ctypes.c_int64, P(D), P(D), P(ctypes.c_uint8),
                                      P(ctypes.c_uint32)]
    if hasattr(L, "rt_diag_vertex"):
        D, U64 = ctypes.c_double, ctypes.c_uint64
        L.rt_diag_vertex.argtypes = [vp, I, I, ctypes.c_uint32, ctypes.c_int64, P(D), P(U64), P(I), P(D), P(U64), P(I),
                                     P(I)]
        L.rt_diag_sincos.argtypes = [I, ctypes.c_int64, P(D), P(D), P(D)]
    return L


lib = _load()


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rt error {code}: {msg}")
        self.code = code


def _check(rc):
    if rc < 0:
        raise RtError(rc, lib.rt_last_error().decode(errors="replace"))
    return rc


def _ptr(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct)) if a is not None else None


class Scene:
    """Immutable scene (SceneSpec::to_scene, scene.rs:357). Share it freely across renders."""

    def __init__(self, handle, base=None):
        self._h = ctypes.c_void_p(handle)
        self._base = base  # a view keeps the scene whose data it shares alive

    def view(self, pos, dir, right=(1.0, 0.0, 0.0), fov=0.5135):
        """A Scene that shares this one's data (host tables, device uploads, workspaces: no copy, no device call) with
        its own camera (rt_scene_view). Every call that takes a scene takes a view. right = (1, 0, 0), fov = 0.5135
        is the reference's camera frame; right's length scales the horizontal field."""
        v = View()
        for j in range(3):
            v.pos[j], v.dir[j], v.right[j] = pos[j], dir[j], right[j]
        v.fov = fov
        h = ctypes.c_void_p()
        _check(lib.rt_scene_view(self._h, ctypes.byref(v), ctypes.byref(h)))
        return Scene(h.value, base=self._base if self._base is not None else self)

    def camera(self):
        """The camera of this scene or view: dict(pos, dir, right, fov) (rt_scene_get_view)."""
        v = View()
        _check(lib.rt_scene_get_view(self._h, ctypes.byref(v)))
        return dict(pos=tuple(v.pos), dir=tuple(v.dir), right=tuple(v.right), fov=v.fov)

    @classmethod
    def from_toml(cls, path, assets_dir=None):
        h = ctypes.c_void_p()
        _check(lib.rt_scene_load_toml(os.fsencode(path), os.fsencode(assets_dir) if assets_dir else None,
                                      ctypes.byref(h)))
        return cls(h.value)

    @classmethod
    def from_desc(cls, cam_pos, cam_dir, objects, meshes=()):
        """objects: list of dicts with ObjectDesc field names; meshes: list of dicts with keys
        vertices (n,3), indices (m,3), bbox_min, bbox_max, surface_area."""
        keep = []
        od = (ObjectDesc * max(1, len(objects)))()
        for i, o in enumerate(objects):
            for k, v in o.items():
                f = getattr(od[i], k)
                if isinstance(f, ctypes.Array):
                    for j, x in enumerate(v):
                        f[j] = x
                else:
                    setattr(od[i], k, v)
        md = (MeshDesc * max(1, len(meshes)))()
        for i, m in enumerate(meshes):
            v = np.ascontiguousarray(m["vertices"], dtype=np.float64)
            ix = np.ascontiguousarray(m["indices"], dtype=np.uint32)
            keep += [v, ix]
            md[i].n_vertices = v.shape[0]
            md[i].vertices = _ptr(v, ctypes.c_double)
            md[i].n_triangles = ix.shape[0]
            md[i].indices = _ptr(ix, ctypes.c_uint32)
            for j in range(3):
                md[i].bbox_min[j] = m["bbox_min"][j]
                md[i].bbox_max[j] = m["bbox_max"][j]
            md[i].surface_area = m["surface_area"]
        d = SceneDesc()
        for j in range(3):
            d.cam_pos[j] = cam_pos[j]
            d.cam_dir[j] = cam_dir[j]
        d.n_objects = len(objects)
        d.objects = od
        d.n_meshes = len(meshes)
        d.meshes = md
        h = ctypes.c_void_p()
        _check(lib.rt_scene_create(ctypes.byref(d), ctypes.byref(h)))
        return cls(h.value)

    def close(self):
        if self._h and self._h.value:
            lib.rt_scene_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def info(self):
        a = np.zeros(16, dtype=np.int64)
        _check(lib.rt_scene_info(self._h, _ptr(a, ctypes.c_int64)))
        keys = ["objects", "light", "meshes", "nodes", "parents", "leaves", "refs", "triangles", "vertices",
                "max_leaf", "max_depth", "slot_tables"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def mesh(self, obj):
        counts = np.zeros(4, dtype=np.int64)
        bbox = np.zeros(6)
        sa = ctypes.c_double()
        _check(lib.rt_scene_mesh(self._h, obj, _ptr(counts, ctypes.c_int64), _ptr(bbox, ctypes.c_double),
                                 ctypes.byref(sa), None, None, None, None, None, None, None))
        nn, nr, nt, nv = (int(x) for x in counts)
        verts = np.zeros((nv, 3))
        idx = np.zeros((nt, 3), dtype=np.uint32)
        kind = np.zeros(nn, dtype=np.int32)
        child = np.zeros((nn, 8), dtype=np.int32)
        off = np.zeros(nn, dtype=np.int32)
        cnt = np.zeros(nn, dtype=np.int32)
        refs = np.zeros(max(1, nr), dtype=np.int32)
        I = ctypes.c_int32
        _check(lib.rt_scene_mesh(self._h, obj, None, None, None, _ptr(verts, ctypes.c_double),
                                 _ptr(idx, ctypes.c_uint32), _ptr(kind, I), _ptr(child, I), _ptr(off, I),
                                 _ptr(cnt, I), _ptr(refs, I)))
        return dict(bbox=bbox, surface_area=sa.value, vertices=verts, indices=idx, kind=kind, child=child,
                    leaf_off=off, leaf_cnt=cnt, refs=refs[:nr])

    def object_bvh(self):
        """The BVH the loader builds over the spheres of a scene past the small-scene tables (rt_scene_object_bvh;
        host data, the kernels do not walk it), or None for a scene without one: boxes[n, 6]
        (min xyz, max xyz), a, count, axis per node in DFS pre-order (count 0: an inner node whose left child is
        the next node and right child a; else a leaf holding refs[a : a + count]), refs = scene object indices,
        rest = the objects outside the tree in scene order, depth = the deepest leaf's (root 0)."""
        counts = np.zeros(4, dtype=np.int64)
        _check(lib.rt_scene_object_bvh(self._h, _ptr(counts, ctypes.c_int64), None, None, None, None, None, None))
        nn, nr, nrest, depth = (int(x) for x in counts)
        if nn == 0:
            return None
        boxes = np.zeros((nn, 6))
        a, cnt, axis = (np.zeros(nn, dtype=np.int32) for _ in range(3))
        refs = np.zeros(max(1, nr), dtype=np.int32)
        rest = np.zeros(max(1, nrest), dtype=np.int32)
        I = ctypes.c_int32
        _check(lib.rt_scene_object_bvh(self._h, None, _ptr(boxes, ctypes.c_double), _ptr(a, I), _ptr(cnt, I),
                                       _ptr(axis, I), _ptr(refs, I), _ptr(rest, I)))
        return dict(boxes=boxes, a=a, count=cnt, axis=axis, refs=refs[:nr], rest=rest[:nrest], depth=depth)

    def trace_ray(self, origins, dirs, device=0, mesh_nearest=False):
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = o.shape[0]
        t = np.zeros(n)
        ids = np.zeros(n, dtype=np.int32)
        pos = np.zeros((n, 3))
        nrm = np.zeros((n, 3))
        D = ctypes.c_double
        _check(lib.rt_trace_rays_flags(self._h, device, FLAG_MESH_NEAREST if mesh_nearest else 0, n, _ptr(o, D),
                                       _ptr(d, D), _ptr(t, D), _ptr(ids, ctypes.c_int32), _ptr(pos, D), _ptr(nrm, D)))
        return t, ids, pos, nrm

    def diag_trace(self, origins, dirs, form=0, device=0, mesh_nearest=False):
        """Scene::trace_ray per ray through the query code of one kernel family (rt_diag.h rt_diag_trace,
        form = DIAG_*): t, object (-1: miss), triangle (-1: none), pos, normal."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = o.shape[0]
        t = np.zeros(n)
        ids = np.zeros(n, dtype=np.int32)
        prim = np.zeros(n, dtype=np.int32)
        pos = np.zeros((n, 3))
        nrm = np.zeros((n, 3))
        D, I = ctypes.c_double, ctypes.c_int32
        _check(lib.rt_diag_trace(self._h, device, form, FLAG_MESH_NEAREST if mesh_nearest else 0, n, _ptr(o, D),
                                 _ptr(d, D), _ptr(t, D), _ptr(ids, I), _ptr(prim, I), _ptr(pos, D), _ptr(nrm, D)))
        return t, ids, prim, pos, nrm

    def diag_visible(self, x, y, form=0, device=0, mesh_nearest=False):
        """Scene::mutually_visible per segment through the query code of one kernel family (rt_diag.h
        rt_diag_visible): visible (bool), and the split forms' mask of meshes near the segment (0 otherwise)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1, 3)
        n = x.shape[0]
        vis = np.zeros(n, dtype=np.uint8)
        near = np.zeros(n, dtype=np.uint32)
        D = ctypes.c_double
        _check(lib.rt_diag_visible(self._h, device, form, FLAG_MESH_NEAREST if mesh_nearest else 0, n, _ptr(x, D),
                                   _ptr(y, D), _ptr(vis, ctypes.c_uint8), _ptr(near, ctypes.c_uint32)))
        return vis.astype(bool), near

    def diag_vertex(self, st, rng, dk, form=0, mis=False, mesh_nearest=False, device=0):
        """One path vertex per row through the integrator of one kernel family (rt_diag.h rt_diag_vertex, form =
        DIAG_*): st (n, 19) = ray origin, ray direction, beta, L, bemit, o, pdf_prev; rng (n, 2) uint64; dk (n, 2)
        int32 = depth, kind. Returns dict(st, rng, dk: the rows after the vertex; info (n, 4) int32 = hit object,
        continue flag, deferred shadow pending, its mesh mask)."""
        st = np.ascontiguousarray(st, dtype=np.float64).reshape(-1, 19)
        rng = np.ascontiguousarray(rng, dtype=np.uint64).reshape(-1, 2)
        dk = np.ascontiguousarray(dk, dtype=np.int32).reshape(-1, 2)
        n = st.shape[0]
        so, ro, do = np.zeros_like(st), np.zeros_like(rng), np.zeros_like(dk)
        info = np.zeros((n, 4), dtype=np.int32)
        D, U64, I = ctypes.c_double, ctypes.c_uint64, ctypes.c_int32
        flags = (FLAG_MIS if mis else 0) | (FLAG_MESH_NEAREST if mesh_nearest else 0)
        _check(lib.rt_diag_vertex(self._h, device, form, flags, n, _ptr(st, D), _ptr(rng, U64), _ptr(dk, I),
                                  _ptr(so, D), _ptr(ro, U64), _ptr(do, I), _ptr(info, I)))
        return dict(st=so, rng=ro, dk=do, info=info)


def make_params(width, height, spp, seed=0x5EED, tile=None, flags=0, device=0, row_step=1):
    """tile = (x0, y0, tile_w, tile_h); with row_step k > 1, tile row i is screen row y0 + i*k."""
    x0, y0, tw, th = tile if tile is not None else (0, 0, width, height)
    return RenderParams(width, height, x0, y0, tw, th, spp, seed, flags, device, row_step)


def render(scene, width, height, spp, seed=0x5EED, tile=None, mis=False, megakernel=False, device=0,
           want_sub=False, cancel=None, row_step=1, mesh_nearest=False, fp32=False):
    """Renders a tile to host memory. Returns (rgb[th, tw, 3] u8, sub[th, tw, 4, 3] f64 or None, stats).
    mesh_nearest: Mesh::intersect's `octree: None` semantics (RT_FLAG_MESH_NEAREST, megakernel only).
    fp32: the f32 perf mode (RT_FLAG_FP32: statistical parity only; meshes with nearest-triangle semantics)."""
    flags = (FLAG_MIS if mis else 0) | (FLAG_MEGAKERNEL if megakernel else 0) | (FLAG_MESH_NEAREST if mesh_nearest else 0)
    flags |= FLAG_FP32 if fp32 else 0
    p = make_params(width, height, spp, seed, tile, flags, device, row_step)
    rgb = np.zeros((p.tile_h, p.tile_w, 3), dtype=np.uint8)
    sub = np.zeros((p.tile_h, p.tile_w, 4, 3), dtype=np.float64) if want_sub else None
    st = RenderStats()
    cflag = cancel if cancel is not None else None
    rc = _check(lib.rt_render(scene.handle, ctypes.byref(p), _ptr(rgb, ctypes.c_uint8), _ptr(sub, ctypes.c_double),
                              ctypes.byref(cflag) if cflag is not None else None, ctypes.byref(st)))
    out = st.as_dict()
    out["cancelled"] = rc == RT_CANCELLED
    return rgb, sub, out


def render_device(scene, params, d_rgb, d_sub=None, stream=None, stats=False):
    """Enqueues a render into device buffers (raw device pointers as ints) on a HIP stream handle."""
    st = RenderStats() if stats else None
    _check(lib.rt_render_device(scene.handle, ctypes.byref(params), ctypes.c_void_p(d_rgb),
                                ctypes.c_void_p(d_sub) if d_sub else None,
                                ctypes.c_void_p(stream) if stream else None,
                                ctypes.byref(st) if st is not None else None))
    return st.as_dict() if st is not None else None


def render_multi(scene, width, height, spp, devices, seed=0x5EED, tile=None, mis=False, band_rows=0, cancel=None,
                 row_step=1, fp32=False, mesh_nearest=False):
    """rt_render_multi: one worker thread per entry of `devices` (ordinals may repeat), bands of rows
    handed out dynamically, RGB8 gathered on the host. Returns (rgb[th, tw, 3] u8, stats)."""
    flags = FLAG_MEGAKERNEL | (FLAG_MIS if mis else 0) | (FLAG_FP32 if fp32 else 0) | \
        (FLAG_MESH_NEAREST if mesh_nearest else 0)
    p = make_params(width, height, spp, seed, tile, flags, devices[0], row_step)
    rgb = np.zeros((p.tile_h, p.tile_w, 3), dtype=np.uint8)
    devs = (ctypes.c_int32 * len(devices))(*devices)
    st = RenderStats()
    rc = _check(lib.rt_render_multi(scene.handle, ctypes.byref(p), devs, len(devices), band_rows,
                                    _ptr(rgb, ctypes.c_uint8), ctypes.byref(cancel) if cancel is not None else None,
                                    ctypes.byref(st)))
    out = st.as_dict()
    out["cancelled"] = rc == RT_CANCELLED
    return rgb, out


# Defaults of denoise / render_denoised (the C ABI has none: every parameter is the caller's). Chosen on a small
# grid by the linear RMSE of a denoised 16-spp frame against a 1024-spp frame.
DENOISE_DEFAULTS = dict(levels=3, sigma_c=0.6, sigma_n=0.3, sigma_z=0.05, sigma_a=0.3)


def render_features(scene, width, height, tile=None, mesh_nearest=False, device=0, row_step=1):
    """First-hit feature buffers of a tile (rt_render_features): float32[th, tw, 8] = mean hit normal (3), mean hit
    distance, mean albedo (3), coverage, over the four tent-centre camera rays of each pixel."""
    p = make_params(width, height, 0, 0, tile, FLAG_MESH_NEAREST if mesh_nearest else 0, device, row_step)
    feat = np.zeros((p.tile_h, p.tile_w, 8), dtype=np.float32)
    _check(lib.rt_render_features(scene.handle, ctypes.byref(p), _ptr(feat, ctypes.c_float)))
    return feat


def denoise(sub, feat, levels=None, sigma_c=None, sigma_n=None, sigma_z=None, sigma_a=None, want_linear=False,
            device=0):
    """Edge-avoiding a-trous filter (rt_denoise) over sub[h, w, 4, 3] f64 (render's want_sub output for the whole
    image) guided by feat[h, w, 8]. Parameters left None come from DENOISE_DEFAULTS; levels=0 is the pass-through; a
    sigma <= 0 drops its term. Returns rgb[h, w, 3] u8, or (rgb, linear float32[h, w, 3]) with want_linear."""
    d = DENOISE_DEFAULTS
    levels = d["levels"] if levels is None else levels
    sig = [d[k] if v is None else v for k, v in (("sigma_c", sigma_c), ("sigma_n", sigma_n), ("sigma_z", sigma_z),
                                                 ("sigma_a", sigma_a))]
    sub = np.ascontiguousarray(sub, dtype=np.float64)
    feat = np.ascontiguousarray(feat, dtype=np.float32)
    h, w = sub.shape[:2]
    if sub.shape != (h, w, 4, 3) or feat.shape != (h, w, 8):
        raise ValueError(f"denoise: sub {sub.shape} / feat {feat.shape} are not [h, w, 4, 3] / [h, w, 8]")
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    lin = np.zeros((h, w, 3), dtype=np.float32) if want_linear else None
    _check(lib.rt_denoise(device, w, h, _ptr(sub, ctypes.c_double), _ptr(feat, ctypes.c_float), levels, *sig,
                          _ptr(rgb, ctypes.c_uint8), _ptr(lin, ctypes.c_float)))
    return (rgb, lin) if want_linear else rgb


def render_denoised(scene, width, height, spp, seed=0x5EED, device=0, cancel=None, mesh_nearest=False,
                    want_linear=False, **denoise_params):
    """A denoised preview of the whole frame: megakernel render + feature buffers + denoise. denoise_params: levels
    and sigma_* (DENOISE_DEFAULTS otherwise). Returns what denoise returns, or None when cancelled."""
    _, sub, st = render(scene, width, height, spp, seed, megakernel=True, device=device, want_sub=True, cancel=cancel,
                        mesh_nearest=mesh_nearest)
    if st["cancelled"]:
        return None
    feat = render_features(scene, width, height, mesh_nearest=mesh_nearest, device=device)
    return denoise(sub, feat, want_linear=want_linear, device=device, **denoise_params)


# Progressive accumulation -------------------------------------------------------------------

# Defaults of denoise_var / render_progressive (the C ABI has none). Chosen on a grid by the linear RMSE of the
# filtered accumulated frame against a 4096-spp frame of another seed, at 16, 64 and 1024 spp on the three scenes
# (tools/denoise_probe.py --var-grid).
DENOISE_VAR_DEFAULTS = dict(levels=3, sigma_c=4.0, sigma_n=0.3, sigma_z=0.05, sigma_a=0.3)

PASS_SEED_STEP = 0x9E3779B97F4A7C15  # render_progressive: pass k renders with seed + k * PASS_SEED_STEP (mod 2^64)


class Accumulator:
    """rt_accum: merges render passes of one width x height frame on one device and estimates each pixel's variance
    from the pass-to-pass scatter. Not thread-safe. The device memory (192 bytes per pixel, plus 115 of staging) comes
    with the first pass."""

    def __init__(self, width, height, device=0):
        h = ctypes.c_void_p()
        _check(lib.rt_accum_create(device, width, height, ctypes.byref(h)))
        self._h = h
        self.width, self.height, self.device = width, height, device

    def close(self):
        if self._h is not None and self._h.value:
            lib.rt_accum_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def reset(self):
        _check(lib.rt_accum_reset(self._h))

    def info(self):
        a = np.zeros(4, dtype=np.int64)
        _check(lib.rt_accum_info(self._h, _ptr(a, ctypes.c_int64)))
        return dict(passes=int(a[0]), n=int(a[1]), width=int(a[2]), height=int(a[3]))

    def add(self, scene, spp, seed, mis=False, megakernel=True, mesh_nearest=False, fp32=False, cancel=None):
        """Renders the whole frame at `spp` with `seed` (rt_accum_add) and merges it with n = spp // 4. Returns the
        render's stats; stats["cancelled"] is True when the cancel word stopped the pass (nothing was merged)."""
        flags = (FLAG_MIS if mis else 0) | (FLAG_MEGAKERNEL if megakernel else 0) | \
            (FLAG_MESH_NEAREST if mesh_nearest else 0) | (FLAG_FP32 if fp32 else 0)
        p = make_params(self.width, self.height, spp, seed, None, flags, self.device, 1)
        st = RenderStats()
        rc = _check(lib.rt_accum_add(self._h, scene.handle, ctypes.byref(p),
                                     ctypes.byref(cancel) if cancel is not None else None, ctypes.byref(st)))
        out = st.as_dict()
        out["cancelled"] = rc == RT_CANCELLED
        return out

    def add_sub(self, sub, n):
        """Merges a pass rendered elsewhere: sub[h, w, 4, 3] f64 (render's want_sub output), n = its spp // 4."""
        sub = np.ascontiguousarray(sub, dtype=np.float64)
        if sub.shape != (self.height, self.width, 4, 3):
            raise ValueError(f"Accumulator.add_sub: sub {sub.shape} is not [{self.height}, {self.width}, 4, 3]")
        _check(lib.rt_accum_add_sub(self._h, _ptr(sub, ctypes.c_double), n))

    def resolve(self, want_sub=True, want_var=False, want_rgb=True):
        """The accumulated frame: (sub[h, w, 4, 3] f64, var[h, w, 4] f32, rgb[h, w, 3] u8), None for what was not
        asked for. var (the variance of the clamped pixel colour: r, g, b and their sum) needs two passes."""
        h, w = self.height, self.width
        sub = np.zeros((h, w, 4, 3), dtype=np.float64) if want_sub else None
        var = np.zeros((h, w, 4), dtype=np.float32) if want_var else None
        rgb = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb else None
        _check(lib.rt_accum_resolve(self._h, _ptr(sub, ctypes.c_double), _ptr(var, ctypes.c_float),
                                    _ptr(rgb, ctypes.c_uint8)))
        return sub, var, rgb

    def counts(self):
        """The per-pixel maps (K_p[h, w], N_p[h, w]) uint32: passes and samples per subpixel merged into each pixel
        (rt_accum_counts); the frame's K and N everywhere while no sparse pass has been merged."""
        k = np.zeros((self.height, self.width), dtype=np.uint32)
        n = np.zeros((self.height, self.width), dtype=np.uint32)
        _check(lib.rt_accum_counts(self._h, _ptr(k, ctypes.c_uint32), _ptr(n, ctypes.c_uint32)))
        return k, n

    def select(self, abs_tol, rel_tol=0.0, max_n=0, cap=None):
        """The pixels whose estimated error is above abs_tol + rel_tol * luminance / 3 and that hold fewer than max_n
        samples per subpixel (max_n <= 0: no limit), ascending ids row * width + col (rt_accum_select; needs two
        passes). Returns (ids uint32[min(count, cap)], count); cap=None: every active pixel."""
        cap = self.width * self.height if cap is None else cap
        ids = np.zeros(max(1, cap), dtype=np.uint32)
        n = ctypes.c_int64(0)
        _check(lib.rt_accum_select(self._h, abs_tol, rel_tol, max_n, _ptr(ids, ctypes.c_uint32), cap, ctypes.byref(n)))
        return ids[:min(n.value, cap)], n.value

    def add_pixels(self, scene, pixels, spp, seed, mis=False, cancel=None):
        """Renders the listed pixels (strictly ascending ids) at `spp` with `seed` and merges them with n = spp // 4
        (rt_accum_add_pixels; needs two full-frame passes first). Returns the render's stats; stats["cancelled"] is True
        when the cancel word stopped the pass (nothing was merged)."""
        px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        p = make_params(self.width, self.height, spp, seed, None, FLAG_MEGAKERNEL | (FLAG_MIS if mis else 0),
                        self.device, 1)
        st = RenderStats()
        rc = _check(lib.rt_accum_add_pixels(self._h, scene.handle, ctypes.byref(p), _ptr(px, ctypes.c_uint32), px.size,
                                            ctypes.byref(cancel) if cancel is not None else None, ctypes.byref(st)))
        out = st.as_dict()
        out["cancelled"] = rc == RT_CANCELLED
        return out

    def add_sub_pixels(self, pixels, sub, n):
        """Merges a compact pass rendered elsewhere: sub[len(pixels), 4, 3] f64 (render_pixels' want_sub output),
        n = its spp // 4."""
        px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        sub = np.ascontiguousarray(sub, dtype=np.float64)
        if sub.shape != (px.size, 4, 3):
            raise ValueError(f"Accumulator.add_sub_pixels: sub {sub.shape} is not [{px.size}, 4, 3]")
        _check(lib.rt_accum_add_sub_pixels(self._h, _ptr(px, ctypes.c_uint32), px.size, _ptr(sub, ctypes.c_double), n))


    def reproject_from(self, src, dst_scene, src_scene, max_n, mesh_nearest=False):
        """Seeds this accumulator (its frame seen from dst_scene) from accumulator `src` (seen from src_scene, a view
        of the same base): every pixel whose four tent-centre first hits are diffuse, project into src's frame and are
        visible from src's camera inherits the nearest src subpixels' history, at most max_n samples per subpixel
        (rt_accum_reproject). Whatever this accumulator held is dropped. Returns the number of pixels
        that received history; info() then counts the full-frame passes since the reprojection."""
        n = ctypes.c_int64(0)
        _check(lib.rt_accum_reproject(self._h, src.handle, dst_scene.handle, src_scene.handle,
                                      FLAG_MESH_NEAREST if mesh_nearest else 0, max_n, ctypes.byref(n)))
        return n.value

    def holes(self, period=0, phase=0, cap=None):
        """The pixels of a seeded accumulator (after reproject_from) that need samples: those with fewer than two
        passes and, with period > 0, those with (col + 3 * row) % period == phase, ascending ids row * width + col
        (rt_accum_holes). Returns (ids uint32[min(count, cap)], n_holes): n_holes counts the pixels with
        fewer than two passes; cap=None: every listed pixel."""
        cap = self.width * self.height if cap is None else cap
        ids = np.zeros(max(1, cap), dtype=np.uint32)
        n, nh = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(lib.rt_accum_holes(self._h, period, phase, _ptr(ids, ctypes.c_uint32), cap, ctypes.byref(n),
                                  ctypes.byref(nh)))
        return ids[:min(n.value, cap)], nh.value

    def fill(self, scene, spp, seed, seed2, period=0, phase=0, mis=False, cancel=None):
        """Gives every hole of a seeded accumulator two passes of `spp` (seeds `seed` and `seed2`) without a full-frame
        pass, and the pixels of the refresh pattern (period, phase: see holes) one (rt_accum_fill).
        Afterwards the accumulator is covered: resolve with the variance, select, add_pixels and reproject_from (as
        src) work although info() reports no full-frame pass. Returns the two renders' summed stats with
        stats["fill"] = (pass-1 list length, pass-2 list length); stats["cancelled"] is True when the cancel word
        stopped a pass (that pass merged nothing, the accumulator is not covered, a later fill completes it)."""
        p = make_params(self.width, self.height, spp, seed, None, FLAG_MEGAKERNEL | (FLAG_MIS if mis else 0),
                        self.device, 1)
        st = RenderStats()
        lens = (ctypes.c_int64 * 2)()
        rc = _check(lib.rt_accum_fill(self._h, scene.handle, ctypes.byref(p), seed2, period, phase,
                                      ctypes.byref(cancel) if cancel is not None else None, ctypes.byref(st), lens))
        out = st.as_dict()
        out["fill"] = (int(lens[0]), int(lens[1]))
        out["cancelled"] = rc == RT_CANCELLED
        return out

    def plan(self, abs_tol, rel_tol=0.0, max_n=0, n=4, gain=1.0, max_passes=PASSES_MAX, cap=None):
        """select plus a pass count per listed pixel (rt_accum_plan): how many passes of n samples per
        subpixel each active pixel should get at once, gain * (N_p g_p / thr^2 - N_p) / n rounded up, within
        1 .. max_passes, clipped by max_n and by a frame's worth of units in all. Returns (ids uint32, counts uint8,
        info) with info = dict(pixels, units, passes): the list's full length, the sum of the counts and the largest
        count."""
        cap = self.width * self.height if cap is None else cap
        ids = np.zeros(max(1, cap), dtype=np.uint32)
        cnt = np.zeros(max(1, cap), dtype=np.uint8)
        n_out, units, passes = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _check(lib.rt_accum_plan(self._h, abs_tol, rel_tol, max_n, n, gain, max_passes, _ptr(ids, ctypes.c_uint32),
                                 _ptr(cnt, ctypes.c_uint8), cap, ctypes.byref(n_out), ctypes.byref(units),
                                 ctypes.byref(passes)))
        m = min(n_out.value, cap)
        return ids[:m], cnt[:m], dict(pixels=n_out.value, units=units.value, passes=passes.value)

    def add_passes(self, scene, pixels, counts, spp, seeds, mis=False, cancel=None):
        """Renders counts[e] passes of pixel pixels[e] at `spp`, pass i with seeds[i], in one launch and merges them in
        pass order (rt_accum_add_passes): bit for bit what add_pixels of {e : counts[e] > i} with seeds[i] gives, pass
        by pass. Returns the render's stats; stats["cancelled"] is True when nothing was merged."""
        px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        ct = np.ascontiguousarray(counts, dtype=np.uint8).reshape(-1)
        if ct.size != px.size:
            raise ValueError(f"Accumulator.add_passes: {ct.size} counts for {px.size} pixels")
        sd = np.ascontiguousarray([int(x) % (1 << 64) for x in seeds], dtype=np.uint64)
        p = make_params(self.width, self.height, spp, 0, None, FLAG_MEGAKERNEL | (FLAG_MIS if mis else 0),
                        self.device, 1)
        st = RenderStats()
        rc = _check(lib.rt_accum_add_passes(self._h, scene.handle, ctypes.byref(p), _ptr(sd, ctypes.c_uint64), sd.size,
                                            _ptr(px, ctypes.c_uint32), _ptr(ct, ctypes.c_uint8), px.size,
                                            ctypes.byref(cancel) if cancel is not None else None, ctypes.byref(st)))
        out = st.as_dict()
        out["cancelled"] = rc == RT_CANCELLED
        return out

    def refine(self, scene, spp, seeds, abs_tol, rel_tol=0.0, max_n=0, gain=1.0, mis=False, cancel=None):
        """plan(abs_tol, rel_tol, max_n, n = spp // 4, gain, max_passes = len(seeds)) followed by add_passes of the
        planned lists, which stay on the device (rt_accum_refine). Returns the render's stats with
        stats["refine"] = (pixels, units, passes used); an empty plan launches nothing."""
        sd = np.ascontiguousarray([int(x) % (1 << 64) for x in seeds], dtype=np.uint64)
        p = make_params(self.width, self.height, spp, 0, None, FLAG_MEGAKERNEL | (FLAG_MIS if mis else 0),
                        self.device, 1)
        st = RenderStats()
        out3 = (ctypes.c_int64 * 3)()
        rc = _check(lib.rt_accum_refine(self._h, scene.handle, ctypes.byref(p), abs_tol, rel_tol, max_n, gain,
                                        _ptr(sd, ctypes.c_uint64), sd.size,
                                        ctypes.byref(cancel) if cancel is not None else None, ctypes.byref(st), out3))
        out = st.as_dict()
        out["refine"] = (int(out3[0]), int(out3[1]), int(out3[2]))
        out["cancelled"] = rc == RT_CANCELLED
        return out


def look_at(pos, target, up=(0.0, 1.0, 0.0), fov=0.5135):
    """The arguments of Scene.view for a camera at pos looking at target: dict(pos, dir, right, fov) with
    dir = norm(target - pos) and right = norm(cross(dir, up)), both unit length. For the shipped scenes' camera
    (looking down -z, up = +y) right is the reference's (1, 0, 0)."""
    pos = np.asarray(pos, dtype=np.float64)
    d = np.asarray(target, dtype=np.float64) - pos
    d = d / np.sqrt(d.dot(d))
    r = np.cross(d, np.asarray(up, dtype=np.float64))
    r = r / np.sqrt(r.dot(r))
    return dict(pos=tuple(pos.tolist()), dir=tuple(d.tolist()), right=tuple(r.tolist()), fov=fov)


def render_pixels(scene, width, height, pixels, spp, seed=0x5EED, mis=False, device=0, want_sub=False, want_rgb=True,
                  cancel=None, path=LIST_AUTO):
    """Renders only the listed pixels of the width x height frame (rt_render_pixels_with): pixels are strictly ascending
    ids row * width + col. Returns (rgb[n, 3] u8 or None, sub[n, 4, 3] f64 or None, stats); entry e is what render gives
    for pixel pixels[e], bit for bit. f64 megakernels only. path: LIST_AUTO (rt_render_pixels' own choice, see
    render_pixels_path) or the kernel family to run; a family the scene has no instance of raises."""
    px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
    p = make_params(width, height, spp, seed, None, FLAG_MEGAKERNEL | (FLAG_MIS if mis else 0), device, 1)
    rgb = np.zeros((px.size, 3), dtype=np.uint8) if want_rgb else None
    sub = np.zeros((px.size, 4, 3), dtype=np.float64) if want_sub else None
    st = RenderStats()
    rc = _check(lib.rt_render_pixels_with(scene.handle, ctypes.byref(p), _ptr(px, ctypes.c_uint32), px.size, path,
                                          _ptr(rgb, ctypes.c_uint8), _ptr(sub, ctypes.c_double),
                                          ctypes.byref(cancel) if cancel is not None else None, ctypes.byref(st)))
    out = st.as_dict()
    out["cancelled"] = rc == RT_CANCELLED
    return rgb, sub, out


def render_pixel_passes(scene, width, height, pixels, counts, spp, seeds, mis=False, device=0, want_sub=False,
                        want_rgb=True, cancel=None, path=LIST_AUTO):
    """render_pixels with counts[e] passes of pixel pixels[e] in one launch, pass i drawing from seeds[i]
    (rt_render_pixel_passes_with; counts in 1 .. len(seeds) <= PASSES_MAX, at most width * height
    units in all). Returns (rgb[units, 3] u8 or None, sub[units, 4, 3] f64 or None, stats), indexed by unit-group
    off[e] + i with off the exclusive prefix sum of counts; each is what render_pixels gives that pixel for
    seeds[i], bit for bit. path: LIST_AUTO (the scene's pool kernel wherever it has one, see render_pixels_path) or the
    kernel family to run; a family the scene has no instance of raises."""
    px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
    ct = np.ascontiguousarray(counts, dtype=np.uint8).reshape(-1)
    if ct.size != px.size:
        raise ValueError(f"render_pixel_passes: {ct.size} counts for {px.size} pixels")
    sd = np.ascontiguousarray([int(x) % (1 << 64) for x in seeds], dtype=np.uint64)
    units = int(ct.astype(np.int64).sum())
    p = make_params(width, height, spp, 0, None, FLAG_MEGAKERNEL | (FLAG_MIS if mis else 0), device, 1)
    rgb = np.zeros((units, 3), dtype=np.uint8) if want_rgb else None
    sub = np.zeros((units, 4, 3), dtype=np.float64) if want_sub else None
    st = RenderStats()
    rc = _check(lib.rt_render_pixel_passes_with(scene.handle, ctypes.byref(p), _ptr(px, ctypes.c_uint32),
                                                _ptr(ct, ctypes.c_uint8), px.size, _ptr(sd, ctypes.c_uint64), sd.size,
                                                path, _ptr(rgb, ctypes.c_uint8), _ptr(sub, ctypes.c_double),
                                                ctypes.byref(cancel) if cancel is not None else None, ctypes.byref(st)))
    out = st.as_dict()
    out["cancelled"] = rc == RT_CANCELLED
    return rgb, sub, out


def render_pixels_path(scene, width, height, spp, n_pixels, mis=False, flags=0):
    """(family, pool) of a pixel-list render (rt_render_pixels_path): the LIST_* family render_pixels takes for a list
    of n_pixels of this frame, and the pool family the scene has under these flags at all (LIST_FUSED: none). Needs no
    GPU."""
    p = make_params(width, height, spp, 0, None, FLAG_MEGAKERNEL | (FLAG_MIS if mis else 0) | flags, 0, 1)
    out = (ctypes.c_int32 * 2)()
    _check(lib.rt_render_pixels_path(scene.handle, ctypes.byref(p), n_pixels, out))
    return int(out[0]), int(out[1])


def denoise_var(sub, feat, var, levels=None, sigma_c=None, sigma_n=None, sigma_z=None, sigma_a=None,
                want_linear=False, want_var=False, device=0):
    """Variance-guided a-trous filter (rt_denoise_var): denoise with the colour term scaled by var[h, w, 4]
    (Accumulator.resolve's; only [..., 3] is used). Parameters left None come from DENOISE_VAR_DEFAULTS. Returns
    rgb[h, w, 3] u8, followed by the linear float32[h, w, 3] with want_linear and the filtered variance
    float32[h, w] with want_var."""
    d = DENOISE_VAR_DEFAULTS
    levels = d["levels"] if levels is None else levels
    sig = [d[k] if v is None else v for k, v in (("sigma_c", sigma_c), ("sigma_n", sigma_n), ("sigma_z", sigma_z),
                                                 ("sigma_a", sigma_a))]
    sub = np.ascontiguousarray(sub, dtype=np.float64)
    feat = np.ascontiguousarray(feat, dtype=np.float32)
    var = np.ascontiguousarray(var, dtype=np.float32)
    h, w = sub.shape[:2]
    if sub.shape != (h, w, 4, 3) or feat.shape != (h, w, 8) or var.shape != (h, w, 4):
        raise ValueError(f"denoise_var: sub {sub.shape} / feat {feat.shape} / var {var.shape} are not [h, w, 4, 3] / "
                         "[h, w, 8] / [h, w, 4]")
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    lin = np.zeros((h, w, 3), dtype=np.float32) if want_linear else None
    vout = np.zeros((h, w), dtype=np.float32) if want_var else None
    F = ctypes.c_float
    _check(lib.rt_denoise_var(device, w, h, _ptr(sub, ctypes.c_double), _ptr(feat, F), _ptr(var, F), levels, *sig,
                              _ptr(rgb, ctypes.c_uint8), _ptr(lin, F), _ptr(vout, F)))
    out = (rgb,) + ((lin,) if want_linear else ()) + ((vout,) if want_var else ())
    return out if len(out) > 1 else rgb


def progressive_passes(spp, first=8):
    """The pass sizes of render_progressive: first/2, first/2, then each pass as large as the total so far, the last
    cut to reach 4 * floor(spp / 4). Every pass is a multiple of 4 (first/2 is rounded down to one, at least 4)."""
    total = 4 * (spp // 4)
    if total < 4:
        raise ValueError("progressive_passes: spp must be >= 4")
    half = max(4, first // 2 // 4 * 4)
    sizes, done = [], 0
    while done < total:
        size = min(half if len(sizes) < 2 else done, total - done)
        sizes.append(size)
        done += size
    return sizes


def render_progressive(scene, width, height, spp, first=8, seed=0x5EED, device=0, cancel=None, **denoise_params):
    """A generator that refines a frame pass by pass and yields (rgb[h, w, 3] u8, spp so far). Passes:
    progressive_passes(spp, first); pass k renders with seed + k * PASS_SEED_STEP (mod 2^64) on the megakernel and is
    merged into an Accumulator. After every pass from the second on: resolve, render_features (once), denoise_var
    (denoise_params: levels / sigma_*, DENOISE_VAR_DEFAULTS otherwise). A frame of one pass only (spp < 8) is yielded
    unfiltered. A raised cancel word ends the generator."""
    sizes = progressive_passes(spp, first)
    feat, done = None, 0
    with Accumulator(width, height, device) as acc:
        for k, size in enumerate(sizes):
            st = acc.add(scene, size, pass_seed(seed, k), cancel=cancel)
            if st["cancelled"]:
                return
            done += size
            if k == 0:
                if len(sizes) == 1:
                    yield acc.resolve(want_sub=False)[2], done
                continue
            sub, var, _ = acc.resolve(want_var=True, want_rgb=False)
            if feat is None:
                feat = render_features(scene, width, height, device=device)
            yield denoise_var(sub, feat, var, device=device, **denoise_params), done


# Rendering to an error target ----------------------------------------------------------------

# Defaults of render_to_error (the C ABI has none). rel_tol stays 0: on the CPU oracle a relative criterion
# (rel_tol 0.15, abs_tol 0.01) gave a linear RMSE 1.32x (cornell_box) and 1.35x (cubes) the uniform render's at equal
# samples, the absolute one 1.000x and 0.999x.
ERROR_TARGET_DEFAULTS = dict(abs_tol=0.04, rel_tol=0.0, first=16, pass_spp=16)


# The measured choice of render_to_error's batch and gain (batch stays 0 by default: the sequential
# loop). Pass them as render_to_error(..., **ERROR_TARGET_BATCH_DEFAULTS).
ERROR_TARGET_BATCH_DEFAULTS = dict(batch=8, gain=1.0)


def pass_seed(seed, k):
    """The seed of pass k of render_progressive and render_to_error."""
    return (seed + k * PASS_SEED_STEP) % (1 << 64)


def render_to_error(scene, width, height, abs_tol=None, max_spp=512, first=None, pass_spp=None, seed=0x5EED,
                    rel_tol=None, device=0, cancel=None, batch=0, gain=None, **denoise_params):
    """A generator that refines a frame until every pixel's estimated standard error (the 3 x 3 tent of the
    accumulator's variance) is below abs_tol + rel_tol * luminance / 3, or holds max_spp samples. It yields
    (rgb[h, w, 3] u8, mean spp, active fraction) after the two full passes of first / 2 and after every sparse pass of
    pass_spp over the pixels Accumulator.select returned (max_n = max_spp // 4 enforces the budget); pass k renders
    with pass_seed(seed, k). Each frame is filtered with denoise_var on the per-pixel-count variance (denoise_params:
    levels / sigma_*, DENOISE_VAR_DEFAULTS otherwise). Parameters left None come from ERROR_TARGET_DEFAULTS. A raised
    cancel word ends the generator.
    batch = C > 0 (at most PASSES_MAX) runs up to C passes per pixel in one launch (Accumulator.refine):
    a batch plans gain (None: ERROR_TARGET_BATCH_DEFAULTS) of each active pixel's predicted need, pass i of the batch
    renders with pass_seed(seed, k + i), k advances by the passes used, and the generator yields after every batch.
    batch = 0 is the sequential loop."""
    d = ERROR_TARGET_DEFAULTS
    abs_tol = d["abs_tol"] if abs_tol is None else abs_tol
    rel_tol = d["rel_tol"] if rel_tol is None else rel_tol
    first = d["first"] if first is None else first
    pass_spp = max(4, (d["pass_spp"] if pass_spp is None else pass_spp) // 4 * 4)
    half = max(4, first // 2 // 4 * 4)
    max_n = max(1, max_spp // 4)
    npix = width * height
    with Accumulator(width, height, device) as acc:
        for k in range(2):
            if acc.add(scene, half, pass_seed(seed, k), cancel=cancel)["cancelled"]:
                return
        feat = render_features(scene, width, height, device=device)
        k = 2
        if batch:
            gain = ERROR_TARGET_BATCH_DEFAULTS["gain"] if gain is None else gain
            n_active = acc.select(abs_tol, rel_tol, max_n, cap=0)[1]
            while True:
                sub, var, _ = acc.resolve(want_var=True, want_rgb=False)
                mean_spp = 4.0 * float(acc.counts()[1].mean())
                yield denoise_var(sub, feat, var, device=device, **denoise_params), mean_spp, n_active / npix
                if n_active == 0:
                    return
                st = acc.refine(scene, pass_spp, [pass_seed(seed, k + i) for i in range(batch)], abs_tol, rel_tol, max_n,
                                gain, cancel=cancel)
                if st["cancelled"]:
                    return
                k += st["refine"][2]
                n_active = acc.select(abs_tol, rel_tol, max_n, cap=0)[1]
        while True:
            ids, _ = acc.select(abs_tol, rel_tol, max_n)
            sub, var, _ = acc.resolve(want_var=True, want_rgb=False)
            mean_spp = 4.0 * float(acc.counts()[1].mean())
            yield denoise_var(sub, feat, var, device=device, **denoise_params), mean_spp, ids.size / npix
            if ids.size == 0:
                return
            if acc.add_pixels(scene, ids, pass_spp, pass_seed(seed, k), cancel=cancel)["cancelled"]:
                return
            k += 1


# Orbiting a scene ---------------------------------------------------------------------------

# The measured choice of render_interactive's fill_spp and refresh (the function's own defaults stay
# 0, 0: the flow of §14). Pass them as render_interactive(..., **FILL_DEFAULTS), or **fill_defaults_for(scene).
FILL_DEFAULTS = dict(fill_spp=16, refresh=4)


def fill_defaults_for(scene):
    """render_interactive's fill_spp and refresh for `scene`: FILL_DEFAULTS for a scene of spheres and planes, off
    (0, 0) for a scene with meshes. On the MI355X the fill won on cornell_box (0.70 of the per-view time at a lower
    RMSE) and lost on the mesh scenes, whose list renders run the fused per-vertex walk: cubes no faster at the same
    RMSE, flying_unicorn 3.3 times slower."""
    return dict(FILL_DEFAULTS) if scene.info()["meshes"] == 0 else dict(fill_spp=0, refresh=0)


def render_interactive(scene, views, width, height, first=8, max_n=64, abs_tol=None, rel_tol=0.0, view_spp=0,
                       pass_spp=16, seed=0x5EED, device=0, cancel=None, fill_spp=0, refresh=0, **denoise_params):
    """A generator over camera views of one scene that carries the accumulated samples across the camera moves. views:
    an iterable (read lazily, one view per frame) of Scene.view keyword dicts (look_at makes them; a "view_spp" key
    overrides the budget for that view) or Scene objects that are views of `scene`. For each view it
      1. seeds an accumulator from the previous view's (Accumulator.reproject_from, at most max_n samples per subpixel
         of history; two accumulators take turns),
      2. merges two full-frame passes of `first` spp each, which give the pixels without history a variance,
      3. with abs_tol set, spends sparse passes of pass_spp on the pixels Accumulator.select returns (their estimated
         error above abs_tol + rel_tol * luminance / 3, fewer than max_n samples per subpixel) until none is left or
         the view's samples reach view_spp per pixel on average,
      4. resolves, computes the view's features and filters with denoise_var (denoise_params: levels / sigma_*),
    and yields (rgb[h, w, 3] u8, fraction of pixels that received history, camera samples traced for this view). Pass k
    of the whole sequence renders with pass_seed(seed, k): one counter over all views, so no pass repeats a seed the
    history already holds. A raised cancel word ends the generator.
    fill_spp > 0 replaces step 2, for every view after the first, by Accumulator.fill: two sparse
    passes of fill_spp over the pixels without history only, plus, with refresh = R > 0, one pass over the pixels
    with (col + 3 * row) % R == view index % R, so that every pixel receives a fresh pass once in R views (refresh = 0:
    a pixel with history is never sampled again by step 2, and the nearest-subpixel fetch's resampling error compounds
    from view to view). The first view still gets its two full passes; fill_spp = 0 is the flow above, bit for bit.
    FILL_DEFAULTS holds the measured choice of (fill_spp, refresh)."""
    half = max(4, first // 4 * 4)
    fill_spp = max(4, fill_spp // 4 * 4) if fill_spp > 0 else 0
    pass_spp = max(4, pass_spp // 4 * 4)
    npix = width * height
    default_spp = view_spp
    accs = [Accumulator(width, height, device), Accumulator(width, height, device)]
    try:
        prev_view, k = None, 0
        for i, view in enumerate(views):
            view_spp = default_spp
            if isinstance(view, dict):  # a view dict may carry its own budget
                view = dict(view)
                view_spp = view.pop("view_spp", default_spp)
            v = view if isinstance(view, Scene) else scene.view(**view)
            acc, prev = accs[i & 1], accs[(i & 1) ^ 1]
            n_valid = 0
            if prev_view is not None:
                n_valid = acc.reproject_from(prev, v, prev_view, max_n)
            else:
                acc.reset()
            samples = 0
            if fill_spp > 0 and prev_view is not None:
                st = acc.fill(v, fill_spp, pass_seed(seed, k), pass_seed(seed, k + 1), period=refresh,
                              phase=i % refresh if refresh > 0 else 0, cancel=cancel)
                if st["cancelled"]:
                    return
                k += 2
                samples += sum(st["fill"]) * fill_spp
            else:
                for _ in range(2):
                    if acc.add(v, half, pass_seed(seed, k), cancel=cancel)["cancelled"]:
                        return
                    k += 1
                    samples += npix * half
            while abs_tol is not None and samples + pass_spp <= view_spp * npix:
                ids, _ = acc.select(abs_tol, rel_tol, max_n)
                ids = ids[:(view_spp * npix - samples) // pass_spp]
                if ids.size == 0:
                    break
                if acc.add_pixels(v, ids, pass_spp, pass_seed(seed, k), cancel=cancel)["cancelled"]:
                    return
                k += 1
                samples += int(ids.size) * pass_spp
            sub, var, _ = acc.resolve(want_var=True, want_rgb=False)
            feat = render_features(v, width, height, device=device)
            yield denoise_var(sub, feat, var, device=device, **denoise_params), n_valid / npix, samples
            prev_view = v
    finally:
        for a in accs:
            a.close()


def band_plan(tile_h, n_workers, band_rows=0):
    """The band plan rt_render_multi hands out: (first tile row, rows) per band, in handout order."""
    n = lib.rt_band_plan(tile_h, n_workers, band_rows, 0, None, None)
    first = np.zeros(max(1, n), dtype=np.int32)
    rows = np.zeros(max(1, n), dtype=np.int32)
    lib.rt_band_plan(tile_h, n_workers, band_rows, n, _ptr(first, ctypes.c_int32), _ptr(rows, ctypes.c_int32))
    return first[:n].tolist(), rows[:n].tolist()


def sample_pixel(x, y, width, height, samples_per_pixel, scene, seed=0x5EED, mis=False):
    """server.rs:320-368 for one pixel: returns the gamma-corrected RGB8 triple of pixel (x, y) where
    y counts from the BOTTOM as in the reference (RenderJob::run passes height - row - 1)."""
    row = height - y - 1
    rgb, _, _ = render(scene, width, height, samples_per_pixel, seed, tile=(x, row, 1, 1), mis=mis)
    return tuple(int(c) for c in rgb[0, 0])


PIXELS_PER_MSG = 60  # server.rs:145


def chunk_messages(rgb, x0=0, y0=0):
    """Packs a rendered tile into the reference's binary messages (server.rs:173-190):
    [u8 type=0][u8 n][u16le x][u16le y][n x RGB8], rows top-first, 60-pixel windows."""
    th, tw, _ = rgb.shape
    for r in range(th):
        for x in range(0, tw, PIXELS_PER_MSG):
            n = min(PIXELS_PER_MSG, tw - x)
            yield struct.pack("<BBHH", 0, n, x0 + x, y0 + r) + rgb[r, x:x + n].tobytes()


class RenderJob:
    """RenderJob::run (server.rs:157-199) on the GPU: renders the frame, then yields the chunk
    messages the WebSocket server sends. `stop()` cancels between bounce iterations."""

    def __init__(self, device=0, seed=0x5EED):
        self.device = device
        self.seed = seed
        self._cancel = ctypes.c_int32(0)

    def stop(self):
        self._cancel.value = 1

    def run(self, scene, width, height, spp, mis=False):
        self._cancel.value = 0
        rgb, _, st = render(scene, width, height, spp, self.seed, mis=mis, device=self.device, cancel=self._cancel)
        if st["cancelled"]:
            return []
        return list(chunk_messages(rgb))


def selftest_arith(n=1 << 24, seed=0x5EED):
    """Device check of the exact-arithmetic shortcuts: (reciprocal, quotient, square-root mismatches)."""
    out = (ctypes.c_ulonglong * 3)()
    _check(lib.rt_selftest_arith_n(n, seed, out, 3))
    return int(out[0]), int(out[1]), int(out[2])


def selftest_tables(ptrs):
    """Device round trips of the per-call pointer views (include/rt_diag.h rt_selftest_tables): per address
    p, (tables() via the kernarg view, tables() of the by-value argument, the round-4 sign-extending form,
    kernarg ctab, kernarg node_slot [= p + 16], kernarg RenderArgs.tail_buf [= p + 32])."""
    n = len(ptrs)
    inp = (ctypes.c_ulonglong * n)(*ptrs)
    out = (ctypes.c_ulonglong * (6 * n))()
    _check(lib.rt_selftest_tables(inp, n, out))
    return [tuple(int(out[6 * i + k]) for k in range(6)) for i in range(n)]


def diag_sincos(x, device=0):
    """The device sincos_2pi (csrc/device/path_f64.h) of an array of doubles in [0, 2 pi] (rt_diag.h
    rt_diag_sincos): (sin, cos)."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    s, c = np.zeros_like(x), np.zeros_like(x)
    D = ctypes.c_double
    _check(lib.rt_diag_sincos(device, x.shape[0], _ptr(x, D), _ptr(s, D), _ptr(c, D)))
    return s, c


def debug_qcheck():
    """RT_QCHECK builds: LDS hand-off protocol violation counters since the last call (4 ints), or
    None when the loaded library was built without the checks."""
    out = (ctypes.c_ulonglong * 4)()
    rc = lib.rt_debug_qcheck(out)
    if rc < 0:
        raise RtError(rc, "rt_debug_qcheck")
    return None if rc == 1 else [int(v) for v in out]


def debug_last_split():
    """The split tail of this thread's last f64 megakernel render (rt_diag.h rt_debug_last_split):
    dict(split=subpixels handed out as sample chunks, want=the kernel family's split before the scratch
    buffer capped it, chunk=samples per chunk)."""
    out = (ctypes.c_longlong * 3)()
    _check(lib.rt_debug_last_split(out))
    return dict(split=int(out[0]), want=int(out[1]), chunk=int(out[2]))


def device_count():
    return lib.rt_device_count()
