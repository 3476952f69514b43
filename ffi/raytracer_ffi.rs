//! Rust bindings of the MI355X render kernel's C ABI (`include/rt_ffi.h`, ABI version 3), for the
//! reference host (SuneelFreimuth/raytracer-server). A maintainer adds this file as
//! `src/raytracer_ffi.rs` and links `librtamd.so` (`raytracer-server_amd/lib/`, built by
//! `make -C raytracer-server_amd`), e.g. from `build.rs`:
//!
//! ```ignore
//! println!("cargo:rustc-link-search=native=/path/to/raytracer-server_amd/lib");
//! println!("cargo:rustc-link-lib=dylib=rtamd");
//! ```
//!
//! Not compiled in this repository (no Rust toolchain in the build image); the declarations mirror
//! `rt_ffi.h` field for field, and `tests/test_abi.py` checks that header's struct layouts and
//! exported symbols. What each entry point replaces in the reference:
//!
//! | entry point          | reference                                                              |
//! |----------------------|------------------------------------------------------------------------|
//! | `rt_scene_load_toml` | `Scene::from_toml` (src/scene.rs:143-150, `SceneSpec::to_scene` :357-441) |
//! | `rt_scene_create`    | `Scene::new` + `Mesh::accelerate` (src/scene.rs:126-141, src/geometry.rs:835-837) |
//! | `rt_render`          | `RenderJob::run`'s per-pixel loop (src/server.rs:157-199) over `sample_pixel` + `gamma_correct` (:320-368) |
//! | `rt_render_device`   | the same, device-resident output on a caller HIP stream                |
//! | `rt_render_multi`    | the row-band fan-out of `RenderJob::run` (src/server.rs:165-168) over several GPUs |
//! | `rt_trace_rays`      | `Scene::trace_ray` (src/scene.rs:272-289), batch form                  |
//!
//! Conventions: a scene is immutable after creation and may be shared by concurrent renders (the
//! reference's `Arc<HashMap<String, Scene>>`, src/server.rs:24); errors are return codes (`RT_OK`,
//! `RT_CANCELLED`, negative `RT_E_*`) with a thread-local message from `rt_last_error`; images are
//! row-major RGB8 with row 0 at the top (the `height - y - 1` flip of src/server.rs:181); `spp`
//! keeps the reference's `spp / 4` samples per subpixel (src/server.rs:332).

#![allow(non_camel_case_types, dead_code)]

use std::os::raw::{c_char, c_int, c_void};

pub const RT_ABI_VERSION: c_int = 3;

pub const RT_OK: c_int = 0;
pub const RT_CANCELLED: c_int = 1;
pub const RT_E_INVAL: c_int = -1;
pub const RT_E_HIP: c_int = -2;
pub const RT_E_OOM: c_int = -3;
pub const RT_E_IO: c_int = -4;
pub const RT_E_PARSE: c_int = -5;
pub const RT_E_NODEVICE: c_int = -6;

/// `config.toml`'s `use_mis` (dead in the reference, src/scene.rs:188): build-defined balance heuristic.
pub const RT_FLAG_MIS: u32 = 1 << 0;
/// Fused per-lane path loop (the fast path) instead of the wavefront pipeline.
pub const RT_FLAG_MEGAKERNEL: u32 = 1 << 1;
/// f32 perf mode: statistical parity only; implies the megakernel.
pub const RT_FLAG_FP32: u32 = 1 << 2;
/// `Mesh::intersect` without the octree (src/geometry.rs:886-903), a BVH on the device.
pub const RT_FLAG_MESH_NEAREST: u32 = 1 << 3;

/// The kernel family of a pixel-list render (`rt_render_pixels_with`, `rt_render_pixels_path`).
pub const RT_LIST_AUTO: i32 = 0;
/// `k_render_list_f64`, the fused megakernel's list instance (per-lane walks).
pub const RT_LIST_FUSED: i32 = 1;
/// The flat-octree query pool's list instance.
pub const RT_LIST_FPOOL: i32 = 2;
/// The role-split pool's list instance.
pub const RT_LIST_ROLES: i32 = 3;
/// The most passes per list entry of a batched render (`rt_render_pixel_passes`), and so the most seeds.
pub const RT_PASSES_MAX: i32 = 16;

pub const RT_BRDF_DIFFUSE: i32 = 0;
pub const RT_BRDF_SPECULAR: i32 = 1;
pub const RT_BRDF_PHONG: i32 = 2;
pub const RT_GEOM_SPHERE: i32 = 0;
pub const RT_GEOM_PLANE: i32 = 1;
pub const RT_GEOM_MESH: i32 = 2;

/// Opaque scene handle (`rt_scene`).
#[repr(C)]
pub struct RtScene {
    _private: [u8; 0],
}

/// `rt_object_desc`: one reference `Object` (src/scene.rs:10-15) with its BRDF and geometry flattened.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct RtObjectDesc {
    pub emitted: [f64; 3],
    pub brdf_kind: i32,
    pub k: [f64; 3],
    pub phong_kd: f64,
    pub phong_ks: f64,
    pub phong_power: i32,
    pub color_d: [f64; 3],
    pub color_s: [f64; 3],
    pub geom_kind: i32,
    pub pos: [f64; 3],
    pub r: f64,
    pub n: [f64; 3],
    pub mesh: i32,
}

/// `rt_mesh_desc`: a mesh after its transforms (src/geometry.rs:427-510); `bbox_*` as the reference
/// holds `Mesh.bounding_box` (the octree root box, src/geometry.rs:1153).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct RtMeshDesc {
    pub n_vertices: u32,
    pub vertices: *const f64,
    pub n_triangles: u32,
    pub indices: *const u32,
    pub bbox_min: [f64; 3],
    pub bbox_max: [f64; 3],
    pub surface_area: f64,
}

/// `rt_scene_desc`: camera (src/scene.rs:104) plus flattened objects and meshes.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct RtSceneDesc {
    pub cam_pos: [f64; 3],
    pub cam_dir: [f64; 3],
    pub n_objects: u32,
    pub objects: *const RtObjectDesc,
    pub n_meshes: u32,
    pub meshes: *const RtMeshDesc,
}

/// `rt_render_params`: a tile of a `width x height` frame (screen rows, row 0 = top).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct RtRenderParams {
    pub width: i32,
    pub height: i32,
    pub x0: i32,
    pub y0: i32,
    pub tile_w: i32,
    pub tile_h: i32,
    pub spp: i32,
    pub seed: u64,
    pub flags: u32,
    pub device: i32,
    /// 0 or 1: contiguous tile rows; k > 1: tile row i is screen row y0 + i * k.
    pub row_step: i32,
}

/// `rt_render_stats`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct RtRenderStats {
    pub samples: i64,
    pub vertices: i64,
    pub iterations: i64,
    pub device_ms: f64,
    pub kernel_ms: [f64; 8],
    pub kernel_launches: [i64; 8],
}

extern "C" {
    pub fn rt_scene_load_toml(toml_path: *const c_char, assets_dir: *const c_char, out: *mut *mut RtScene) -> c_int;
    pub fn rt_scene_create(desc: *const RtSceneDesc, out: *mut *mut RtScene) -> c_int;
    pub fn rt_scene_destroy(scene: *mut RtScene);
    pub fn rt_scene_info(scene: *const RtScene, info: *mut i64 /* [16] */) -> c_int;
    pub fn rt_scene_mesh(
        scene: *const RtScene, object: i32, counts: *mut i64 /* [4] */, bbox: *mut f64 /* [6] */,
        surface_area: *mut f64, vertices: *mut f64, indices: *mut u32, kind: *mut i32, child: *mut i32,
        leaf_off: *mut i32, leaf_cnt: *mut i32, refs: *mut i32,
    ) -> c_int;
    /// The host-side BVH over the spheres of a scene beyond the small-scene tables (nodes in DFS pre-order,
    /// leaf runs of scene object indices, the rest list of planes and meshes); any output may be null.
    pub fn rt_scene_object_bvh(
        scene: *const RtScene, counts: *mut i64 /* [4] */, boxes: *mut f64, a: *mut i32, count: *mut i32,
        axis: *mut i32, refs: *mut i32, rest: *mut i32,
    ) -> c_int;

    /// Host buffers: `rgb_out` tile_w * tile_h * 3 bytes; `sub_out` (nullable) tile_w * tile_h * 12
    /// f64 subpixel means before the clamp. `cancel` (nullable): the job's `AtomicBool`
    /// (src/server.rs:226-251) viewed as an `i32`, read while the render runs; it may be shared by
    /// concurrent renders and is never registered with HIP. Returns `RT_CANCELLED` when it stopped
    /// the render.
    pub fn rt_render(
        scene: *const RtScene, params: *const RtRenderParams, rgb_out: *mut u8, sub_out: *mut f64,
        cancel: *const i32, stats: *mut RtRenderStats,
    ) -> c_int;
    /// Device buffers on `params.device`, enqueued on `stream` (a `hipStream_t`, null = default
    /// stream); synchronous with respect to the stream only when `stats` is non-null.
    pub fn rt_render_device(
        scene: *const RtScene, params: *const RtRenderParams, d_rgb: *mut c_void, d_sub: *mut c_void,
        stream: *mut c_void, stats: *mut RtRenderStats,
    ) -> c_int;
    /// Several devices (one worker thread per entry of `devices`; ordinals may repeat), bands of
    /// `band_rows` rows (<= 0: about 8 per worker) handed out dynamically, host gather into `rgb_out`.
    pub fn rt_render_multi(
        scene: *const RtScene, params: *const RtRenderParams, devices: *const i32, n_devices: i32,
        band_rows: i32, rgb_out: *mut u8, cancel: *const i32, stats: *mut RtRenderStats,
    ) -> c_int;
    /// The band plan of `rt_render_multi` (no GPU); returns the band count, writes at most `cap`.
    pub fn rt_band_plan(
        tile_h: i32, n_workers: i32, band_rows: i32, cap: i32, first_row: *mut i32, rows: *mut i32,
    ) -> i32;

    pub fn rt_trace_rays(
        scene: *const RtScene, device: i32, n: i64, origins: *const f64, dirs: *const f64, t: *mut f64,
        object: *mut i32, pos: *mut f64, normal: *mut f64,
    ) -> c_int;
    pub fn rt_trace_rays_flags(
        scene: *const RtScene, device: i32, flags: u32, n: i64, origins: *const f64, dirs: *const f64,
        t: *mut f64, object: *mut i32, pos: *mut f64, normal: *mut f64,
    ) -> c_int;

    /// First-hit feature buffers of the tile: `feat_out` tile_w * tile_h * 8 floats (mean normal, mean hit
    /// distance, mean albedo, coverage; rt_ffi.h).
    pub fn rt_render_features(scene: *const RtScene, params: *const RtRenderParams, feat_out: *mut f32) -> c_int;
    /// The same into a device buffer, enqueued on `stream`.
    pub fn rt_render_features_device(
        scene: *const RtScene, params: *const RtRenderParams, d_feat: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    /// Edge-avoiding a-trous filter over `rt_render`'s `sub_out` (whole image) guided by the features;
    /// `levels` 0..8 (0: pass-through), a sigma <= 0 drops its term; `lin_out` nullable.
    pub fn rt_denoise(
        device: i32, width: i32, height: i32, sub: *const f64, feat: *const f32, levels: i32, sigma_c: f32,
        sigma_n: f32, sigma_z: f32, sigma_a: f32, rgb_out: *mut u8, lin_out: *mut f32,
    ) -> c_int;
    /// The same on device buffers; waits for the filter and frees its scratch before returning.
    pub fn rt_denoise_device(
        device: i32, width: i32, height: i32, sub: *const f64, feat: *const f32, levels: i32, sigma_c: f32,
        sigma_n: f32, sigma_z: f32, sigma_a: f32, rgb_out: *mut u8, lin_out: *mut f32, stream: *mut c_void,
    ) -> c_int;

    /// Progressive accumulation (rt_ffi.h). The accumulator handle is an opaque pointer; one call
    /// at a time per accumulator. `rt_accum_create` makes no device call.
    pub fn rt_accum_create(device: i32, width: i32, height: i32, out: *mut *mut c_void) -> c_int;
    pub fn rt_accum_destroy(accum: *mut c_void);
    pub fn rt_accum_reset(accum: *mut c_void) -> c_int;
    /// `info`: K (passes), N (samples per subpixel), width, height.
    pub fn rt_accum_info(accum: *const c_void, info: *mut i64 /* [4] */) -> c_int;
    /// Renders `params` (the accumulator's whole frame, spp >= 4) and merges it; `RT_CANCELLED` leaves the
    /// accumulator untouched.
    pub fn rt_accum_add(
        accum: *mut c_void, scene: *const RtScene, params: *const RtRenderParams, cancel: *const i32,
        stats: *mut RtRenderStats,
    ) -> c_int;
    /// Merges a pass rendered elsewhere: `sub` width * height * 12 f64 (host), `n` >= 1 samples per subpixel.
    pub fn rt_accum_add_sub(accum: *mut c_void, sub: *const f64, n: i32) -> c_int;
    pub fn rt_accum_add_sub_device(accum: *mut c_void, d_sub: *const c_void, n: i32, stream: *mut c_void) -> c_int;
    /// The accumulated frame; any output may be null. `var_out` (width * height * 4 f32) needs two passes.
    pub fn rt_accum_resolve(accum: *mut c_void, sub_out: *mut f64, var_out: *mut f32, rgb_out: *mut u8) -> c_int;
    pub fn rt_accum_resolve_device(
        accum: *mut c_void, d_sub: *mut c_void, d_var: *mut c_void, d_rgb: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    /// `rt_denoise` with the colour term scaled by the pixel's variance (`var`: `rt_accum_resolve`'s `var_out`);
    /// `var_out` (nullable): width * height f32, the filtered variance.
    pub fn rt_denoise_var(
        device: i32, width: i32, height: i32, sub: *const f64, feat: *const f32, var: *const f32, levels: i32,
        sigma_c: f32, sigma_n: f32, sigma_z: f32, sigma_a: f32, rgb_out: *mut u8, lin_out: *mut f32,
        var_out: *mut f32,
    ) -> c_int;
    pub fn rt_denoise_var_device(
        device: i32, width: i32, height: i32, sub: *const f64, feat: *const f32, var: *const f32, levels: i32,
        sigma_c: f32, sigma_n: f32, sigma_z: f32, sigma_a: f32, rgb_out: *mut u8, lin_out: *mut f32,
        var_out: *mut f32, stream: *mut c_void,
    ) -> c_int;

    /// Rendering to a per-pixel error target (rt_ffi.h). Renders only the listed pixels of the
    /// whole frame `params`: `pixels` are `n_pixels` strictly ascending ids `row * width + col`; entry `e` of
    /// `rgb_out` (n * 3, nullable) and `sub_out` (n * 12, nullable) is `rt_render`'s output of that pixel.
    pub fn rt_render_pixels(
        scene: *const RtScene, params: *const RtRenderParams, pixels: *const u32, n_pixels: i64, rgb_out: *mut u8,
        sub_out: *mut f64, cancel: *const i32, stats: *mut RtRenderStats,
    ) -> c_int;
    /// The same with device buffers, enqueued on `stream`; the list is the caller's contract.
    pub fn rt_render_pixels_device(
        scene: *const RtScene, params: *const RtRenderParams, d_pixels: *const c_void, n_pixels: i64,
        d_rgb: *mut c_void, d_sub: *mut c_void, stream: *mut c_void, stats: *mut RtRenderStats,
    ) -> c_int;
    /// `path_out[0]`: the kernel family (`RT_LIST_*`) `rt_render_pixels` takes for a list of `n_pixels`;
    /// `path_out[1]`: the pool family the scene has under these flags (`RT_LIST_FUSED`: none). No GPU needed.
    pub fn rt_render_pixels_path(
        scene: *const RtScene, params: *const RtRenderParams, n_pixels: i64, path_out: *mut i32,
    ) -> c_int;
    /// `rt_render_pixels` with the kernel family chosen by the caller (`RT_LIST_AUTO`: `rt_render_pixels` itself);
    /// a family the scene has no instance of is `RT_E_INVAL`. Same bits whichever family runs.
    pub fn rt_render_pixels_with(
        scene: *const RtScene, params: *const RtRenderParams, pixels: *const u32, n_pixels: i64, path: i32,
        rgb_out: *mut u8, sub_out: *mut f64, cancel: *const i32, stats: *mut RtRenderStats,
    ) -> c_int;
    pub fn rt_render_pixels_with_device(
        scene: *const RtScene, params: *const RtRenderParams, d_pixels: *const c_void, n_pixels: i64, path: i32,
        d_rgb: *mut c_void, d_sub: *mut c_void, stream: *mut c_void, stats: *mut RtRenderStats,
    ) -> c_int;
    /// Renders the listed pixels and merges them (needs two full-frame passes first); `RT_CANCELLED` merges nothing.
    pub fn rt_accum_add_pixels(
        accum: *mut c_void, scene: *const RtScene, params: *const RtRenderParams, pixels: *const u32, n_pixels: i64,
        cancel: *const i32, stats: *mut RtRenderStats,
    ) -> c_int;
    /// Merges a compact pass: `sub` n_pixels * 12 f64 (host), `n` >= 1 samples per subpixel.
    pub fn rt_accum_add_sub_pixels(
        accum: *mut c_void, pixels: *const u32, n_pixels: i64, sub: *const f64, n: i32,
    ) -> c_int;
    pub fn rt_accum_add_sub_pixels_device(
        accum: *mut c_void, d_pixels: *const c_void, n_pixels: i64, d_sub: *const c_void, n: i32, stream: *mut c_void,
    ) -> c_int;
    /// The per-pixel passes and samples per subpixel (width * height u32 each, either nullable).
    pub fn rt_accum_counts(accum: *mut c_void, k_out: *mut u32, n_out: *mut u32) -> c_int;
    /// The pixels whose estimated error is above the target, ascending; at most `cap` are written, `n_out` is the
    /// full count. `max_n` > 0 excludes pixels that already hold that many samples per subpixel.
    pub fn rt_accum_select(
        accum: *mut c_void, abs_tol: f32, rel_tol: f32, max_n: i32, pixels_out: *mut u32, cap: i64, n_out: *mut i64,
    ) -> c_int;
    pub fn rt_accum_select_device(
        accum: *mut c_void, abs_tol: f32, rel_tol: f32, max_n: i32, d_pixels: *mut c_void, cap: i64, n_out: *mut i64,
        stream: *mut c_void,
    ) -> c_int;

    /// Camera views and accumulator reprojection (rt_ffi.h). `view`: an `RtView`, the 10 doubles of
    /// an `rt_view`. The new handle shares `base`'s data (no device call, no copy) and has its own camera; `base`
    /// must outlive it; `rt_scene_destroy` releases it.
    pub fn rt_scene_view(base: *const RtScene, view: *const f64 /* [10] */, out: *mut *mut RtScene) -> c_int;
    /// The camera of a scene or view, as an `RtView`.
    pub fn rt_scene_get_view(scene: *const RtScene, view_out: *mut f64 /* [10] */) -> c_int;
    /// Seeds accumulator `dst` (view `dst_view`) from `src` (view `src_view`): `max_n` >= 1 caps the inherited
    /// samples per subpixel; `n_valid` (nullable): dst pixels that received history.
    pub fn rt_accum_reproject(
        dst: *mut c_void, src: *mut c_void, dst_view: *const RtScene, src_view: *const RtScene, flags: u32,
        max_n: i32, n_valid: *mut i64,
    ) -> c_int;

    /// Filling the holes of a reprojection (rt_ffi.h). The pixels of a seeded accumulator with
    /// fewer than two passes, plus, with `period` > 0, those with `(col + 3 * row) % period == phase`; ascending,
    /// at most `cap` written, `n_out` the full count, `n_holes` (nullable) the count with fewer than two passes.
    pub fn rt_accum_holes(
        accum: *mut c_void, period: i32, phase: i32, pixels_out: *mut u32, cap: i64, n_out: *mut i64,
        n_holes: *mut i64,
    ) -> c_int;
    pub fn rt_accum_holes_device(
        accum: *mut c_void, period: i32, phase: i32, d_pixels: *mut c_void, cap: i64, n_out: *mut i64,
        n_holes: *mut i64, stream: *mut c_void,
    ) -> c_int;
    /// Two sparse passes (seeds `params.seed` and `seed2`) that give every hole two passes; afterwards the
    /// accumulator is covered and resolves, selects and reprojects without a full-frame pass. `fill_out`
    /// (nullable): the two lists' lengths. `RT_CANCELLED` leaves it uncovered; a later fill completes it.
    pub fn rt_accum_fill(
        accum: *mut c_void, scene: *const RtScene, params: *const RtRenderParams, seed2: u64, period: i32, phase: i32,
        cancel: *const i32, stats: *mut RtRenderStats, fill_out: *mut i64 /* [2] */,
    ) -> c_int;

    /// Batched passes: `rt_render_pixels` with `counts[e]` passes (1 ..= `n_seeds` <= `RT_PASSES_MAX`)
    /// of pixel `pixels[e]` in one launch, pass `i` drawing from `seeds[i]`; the outputs are indexed by unit-group
    /// `off[e] + i` (`off`: the exclusive prefix sum of `counts`), each bit for bit `rt_render_pixels`' for that seed.
    pub fn rt_render_pixel_passes(
        scene: *const RtScene, params: *const RtRenderParams, pixels: *const u32, counts: *const u8, n_pixels: i64,
        seeds: *const u64, n_seeds: i32, rgb_out: *mut u8, sub_out: *mut f64, cancel: *const i32,
        stats: *mut RtRenderStats,
    ) -> c_int;
    /// The same with device lists and outputs; `units` is the sum of the counts; `seeds` stay on the host; waits.
    pub fn rt_render_pixel_passes_device(
        scene: *const RtScene, params: *const RtRenderParams, d_pixels: *const c_void, d_counts: *const c_void,
        n_pixels: i64, units: i64, seeds: *const u64, n_seeds: i32, d_rgb: *mut c_void, d_sub: *mut c_void,
        stream: *mut c_void, stats: *mut RtRenderStats,
    ) -> c_int;
    /// `rt_render_pixel_passes` with the kernel family chosen by the caller (`RT_LIST_*`), by
    /// `rt_render_pixels_with`'s rules: `RT_LIST_AUTO` is the plain call; a family the scene has no instance of is
    /// `RT_E_INVAL` before any device call. Same bits whichever family runs.
    pub fn rt_render_pixel_passes_with(
        scene: *const RtScene, params: *const RtRenderParams, pixels: *const u32, counts: *const u8, n_pixels: i64,
        seeds: *const u64, n_seeds: i32, path: i32, rgb_out: *mut u8, sub_out: *mut f64, cancel: *const i32,
        stats: *mut RtRenderStats,
    ) -> c_int;
    /// `rt_render_pixel_passes_device` with the family chosen by the caller, by the same rules.
    pub fn rt_render_pixel_passes_with_device(
        scene: *const RtScene, params: *const RtRenderParams, d_pixels: *const c_void, d_counts: *const c_void,
        n_pixels: i64, units: i64, seeds: *const u64, n_seeds: i32, path: i32, d_rgb: *mut c_void,
        d_sub: *mut c_void, stream: *mut c_void, stats: *mut RtRenderStats,
    ) -> c_int;
    /// `rt_accum_select` plus a pass count per listed pixel (`n` samples per subpixel per pass, `gain` in (0, 1],
    /// `max_passes` in 1 ..= `RT_PASSES_MAX`), capped to a frame's worth of units in all.
    pub fn rt_accum_plan(
        accum: *mut c_void, abs_tol: f32, rel_tol: f32, max_n: i32, n: i32, gain: f32, max_passes: i32,
        pixels_out: *mut u32, counts_out: *mut u8, cap: i64, n_out: *mut i64, units_out: *mut i64,
        passes_out: *mut i64,
    ) -> c_int;
    pub fn rt_accum_plan_device(
        accum: *mut c_void, abs_tol: f32, rel_tol: f32, max_n: i32, n: i32, gain: f32, max_passes: i32,
        d_pixels: *mut c_void, d_counts: *mut c_void, cap: i64, n_out: *mut i64, units_out: *mut i64,
        passes_out: *mut i64, stream: *mut c_void,
    ) -> c_int;
    /// Renders the listed pixels' passes and merges each entry's units in pass order: the bits of `counts[e]`
    /// successive sparse merges. `RT_CANCELLED` merges nothing.
    pub fn rt_accum_add_passes(
        accum: *mut c_void, scene: *const RtScene, params: *const RtRenderParams, seeds: *const u64, n_seeds: i32,
        pixels: *const u32, counts: *const u8, n_pixels: i64, cancel: *const i32, stats: *mut RtRenderStats,
    ) -> c_int;
    /// Plan, expand, render and merge with the lists on the device; `out` (nullable) = pixels, units, passes used.
    pub fn rt_accum_refine(
        accum: *mut c_void, scene: *const RtScene, params: *const RtRenderParams, abs_tol: f32, rel_tol: f32,
        max_n: i32, gain: f32, seeds: *const u64, n_seeds: i32, cancel: *const i32, stats: *mut RtRenderStats,
        out: *mut i64 /* [3] */,
    ) -> c_int;

    pub fn rt_last_error() -> *const c_char;
    pub fn rt_abi_version() -> c_int;
    pub fn rt_device_count() -> c_int;
}

/// Owned scene handle: destroyed on drop; `Send + Sync` because the library allows concurrent
/// renders on one scene (rt_ffi.h), like the reference's shared `Arc<Scene>`.
pub struct Scene(pub *mut RtScene);
unsafe impl Send for Scene {}
unsafe impl Sync for Scene {}
impl Drop for Scene {
    fn drop(&mut self) {
        unsafe { rt_scene_destroy(self.0) }
    }
}

/// `rt_view` as the ABI passes it: pos[3], dir[3], right[3], fov (the reference's camera is
/// right = (1, 0, 0), fov = 0.5135, src/server.rs:328-331).
pub type RtView = [f64; 10];

/// A handle on `base`'s scene data with its own camera (`rt_scene_view`). The caller keeps `base` alive for as long
/// as the view lives.
pub fn scene_view(base: &Scene, view: &RtView) -> Result<Scene, String> {
    let mut s: *mut RtScene = std::ptr::null_mut();
    let rc = unsafe { rt_scene_view(base.0, view.as_ptr(), &mut s) };
    if rc == RT_OK {
        Ok(Scene(s))
    } else {
        Err(format!("rt_scene_view: {} ({})", rc, last_error()))
    }
}

/// The library's last error on this thread.
pub fn last_error() -> String {
    unsafe {
        let p = rt_last_error();
        if p.is_null() {
            String::new()
        } else {
            std::ffi::CStr::from_ptr(p).to_string_lossy().into_owned()
        }
    }
}

/// Loads a scene the way `Scene::from_toml` does (meshes from `<toml dir>/assets`).
pub fn load_scene(toml_path: &str) -> Result<Scene, String> {
    let path = std::ffi::CString::new(toml_path).map_err(|e| e.to_string())?;
    let mut s: *mut RtScene = std::ptr::null_mut();
    let rc = unsafe { rt_scene_load_toml(path.as_ptr(), std::ptr::null(), &mut s) };
    if rc == RT_OK {
        Ok(Scene(s))
    } else {
        Err(format!("rt_scene_load_toml: {} ({})", rc, last_error()))
    }
}

/// `RenderJob::run`'s frame (src/server.rs:157-199) in one call: the RGB8 frame, or `None` when the
/// job was cancelled. `cancel` is the job's stop flag kept as an `AtomicI32` (the reference's
/// `AtomicBool`, src/server.rs:226-251; `stop()` stores 1); it is read while the render runs. The caller
/// then emits the reference's chunk messages per screen row `y` and 60-pixel window `x`
/// (src/server.rs:169-192): `[0u8, n as u8, x as u16 LE, y as u16 LE]` followed by
/// `rgb[(y * width + x) * 3 ..][.. 3 * n]`. Call it from `tokio::task::spawn_blocking`.
pub fn render_frame(
    scene: &Scene, width: i32, height: i32, spp: i32, seed: u64, cancel: &std::sync::atomic::AtomicI32,
) -> Result<Option<Vec<u8>>, String> {
    let p = RtRenderParams {
        width, height, x0: 0, y0: 0, tile_w: width, tile_h: height, spp, seed,
        flags: RT_FLAG_MEGAKERNEL, device: 0, row_step: 1,
    };
    let mut rgb = vec![0u8; (width as usize) * (height as usize) * 3];
    let rc = unsafe {
        rt_render(scene.0, &p, rgb.as_mut_ptr(), std::ptr::null_mut(), cancel.as_ptr() as *const i32,
                  std::ptr::null_mut())
    };
    match rc {
        RT_OK => Ok(Some(rgb)),
        RT_CANCELLED => Ok(None),
        _ => Err(format!("rt_render: {} ({})", rc, last_error())),
    }
}
