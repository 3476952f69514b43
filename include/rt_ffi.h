/*
 * rt_ffi.h — C ABI of the MI355X-native path-tracing render kernel.
 *
 * Drop-in boundary for the per-pixel sample loop of SuneelFreimuth/raytracer-server. Each entry
 * point names the reference interface it replaces (paths relative to the reference repo root):
 *
 *   rt_scene_load_toml  <- Scene::from_toml                  src/scene.rs:143-150 (+ SceneSpec::to_scene :357-441)
 *   rt_scene_create     <- Scene::new + Mesh::accelerate     src/scene.rs:126-141, src/geometry.rs:835-837
 *                          (for a host that keeps its own loader and hands over flattened objects)
 *   rt_render           <- RenderJob::run's per-pixel loop   src/server.rs:157-199 calling
 *                          sample_pixel + gamma_correct      src/server.rs:320-368 (and the `as u8` at :187-189)
 *   rt_render_device    <- same, device-resident output, enqueued on a caller HIP stream (no host sync)
 *   rt_render_multi     <- same, bands handed out dynamically to several devices (the row-band fan-out of
 *                          RenderJob::run, server.rs:165-168), host gather
 *   rt_trace_rays       <- Scene::trace_ray                  src/scene.rs:272-289 (batch form, for parity tests)
 *   rt_render_features, rt_denoise: no counterpart in the reference (denoised previews at low spp)
 *   rt_accum_*, rt_denoise_var: no counterpart either (progressive refinement: merged passes, their variance, and
 *                          a filter guided by it)
 *   rt_render_pixels, rt_accum_select, rt_accum_add_pixels: no counterpart either (rendering to a per-pixel error
 *                          target with sparse pixel-list passes)
 *   rt_render_pixels_path, rt_render_pixels_with: no counterpart either (which kernel family runs a pixel list of
 *                          a mesh scene: the pool kernel of its full frame, or the fused per-lane walk)
 *   rt_render_pixel_passes, rt_render_pixel_passes_with, rt_accum_plan, rt_accum_add_passes, rt_accum_refine: no
 *                          counterpart either (several error-target passes per pixel in one launch, by the same
 *                          families)
 *   rt_scene_view, rt_accum_reproject: no counterpart either (camera views of one scene, and an accumulator's
 *                          history carried across a camera move)
 *   rt_accum_holes, rt_accum_fill: no counterpart either (after a reprojection, samples only for the pixels that
 *                          received no history)
 *
 * Conventions (mirroring the reference's):
 *   - a scene is immutable after creation and may be shared by concurrent rt_render calls
 *     (the reference shares Arc<HashMap<String, Scene>>, server.rs:24);
 *   - errors never abort: every call returns RT_OK (0), RT_CANCELLED (1) or a negative RT_E_*
 *     code, and rt_last_error() gives a thread-local message (the reference panics instead);
 *   - images are row-major RGB8, row 0 = top; pixel (x, row) is the reference's
 *     sample_pixel(x, height - row - 1, ...) (server.rs:179-186);
 *   - spp follows the reference: 4 * floor(spp / 4) samples are traced (server.rs:332); spp < 4
 *     renders black exactly like the reference.
 *   - randomness: counter-based, one stream per camera sample: Philox4x32-10 keyed by the seed, with
 *     counter (global pixel, sample, 0, subpixel), seeds an xoroshiro128++ stream that the path consumes
 *     in the reference's draw order; output is independent of tiling, device count and
 *     kernel mode.
 */
#ifndef RT_FFI_H
#define RT_FFI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 3  /* 2: rt_render_params.row_step; 3: rt_render_multi. The denoised-preview entry points
                             (rt_render_features*, rt_denoise*) are additive: no struct or existing call changed, so
                             the version stays 3; likewise progressive accumulation (rt_accum_*, rt_denoise_var*) and
                             the error-target calls (rt_render_pixels*, rt_accum_add_pixels, rt_accum_add_sub_pixels*,
                             rt_accum_counts, rt_accum_select*) and the views and reprojection (rt_scene_view,
                             rt_scene_get_view, rt_accum_reproject) and the hole fill (rt_accum_holes*,
                             rt_accum_fill) and the pixel-list kernel families (rt_render_pixels_path,
                             rt_render_pixels_with*, RT_LIST_*) and the batched passes with their families
                             (rt_render_pixel_passes*, rt_accum_plan*, rt_accum_add_passes, rt_accum_refine) */

/* return codes */
#define RT_OK 0
#define RT_CANCELLED 1
#define RT_E_INVAL (-1)
#define RT_E_HIP (-2)
#define RT_E_OOM (-3)
#define RT_E_IO (-4)
#define RT_E_PARSE (-5)
#define RT_E_NODEVICE (-6)

/* rt_render_params.flags */
#define RT_FLAG_MIS (1u << 0)        /* config.toml `use_mis` (dead in the reference, scene.rs:188): build-defined balance heuristic */
#define RT_FLAG_MEGAKERNEL (1u << 1) /* fused per-lane path loop instead of the wavefront pipeline */
#define RT_FLAG_FP32 (1u << 2)       /* f32 perf mode (statistical parity only): diffuse/mirror BRDFs and
                                        sphere lights (RT_E_INVAL otherwise), meshes with nearest-triangle semantics;
                                        implies the megakernel. Default is the reference's f64 */
#define RT_FLAG_MESH_NEAREST (1u << 3) /* Mesh::intersect's `octree: None` branch (geometry.rs:886-903: nearest
                                          triangle, strict < in index order) instead of the octree walk, accelerated on
                                          the device by a BVH; megakernel only (RT_E_INVAL with the wavefront) */

typedef struct rt_scene rt_scene;

enum { RT_BRDF_DIFFUSE = 0, RT_BRDF_SPECULAR = 1, RT_BRDF_PHONG = 2 };   /* scene.rs:18-28 */
enum { RT_GEOM_SPHERE = 0, RT_GEOM_PLANE = 1, RT_GEOM_MESH = 2 };       /* geometry.rs:388-392 */

typedef struct {
    double emitted[3];          /* Object.emitted (scene.rs:12) */
    int32_t brdf_kind;          /* RT_BRDF_* */
    double k[3];                /* Diffuse kd / Specular ks */
    double phong_kd, phong_ks;  /* Phong (scene.rs:21-27) */
    int32_t phong_power;
    double color_d[3], color_s[3];
    int32_t geom_kind;          /* RT_GEOM_* */
    double pos[3];              /* sphere centre / plane point */
    double r;                   /* sphere radius */
    double n[3];                /* plane normal */
    int32_t mesh;               /* index into rt_scene_desc.meshes (RT_GEOM_MESH) */
} rt_object_desc;

typedef struct {
    uint32_t n_vertices;
    const double* vertices;     /* 3 per vertex, after transforms (geometry.rs:427-510) */
    uint32_t n_triangles;
    const uint32_t* indices;    /* 3 per triangle (0-based) */
    double bbox_min[3];         /* Mesh.bounding_box exactly as the reference holds it after */
    double bbox_max[3];         /*   transforms (octree root box, geometry.rs:1153) */
    double surface_area;        /* Mesh.surface_area (geometry.rs:771; mesh-light pdf) */
} rt_mesh_desc;

typedef struct {
    double cam_pos[3], cam_dir[3];   /* Scene.camera (scene.rs:104) */
    uint32_t n_objects;
    const rt_object_desc* objects;
    uint32_t n_meshes;
    const rt_mesh_desc* meshes;
} rt_scene_desc;

typedef struct {
    int32_t width, height;       /* full image (camera frame uses these, server.rs:328-331) */
    int32_t x0, y0;              /* tile origin, screen coordinates (row 0 = top) */
    int32_t tile_w, tile_h;      /* tile size; output buffers are tile_w * tile_h pixels */
    int32_t spp;                 /* reference semantics (server.rs:332) */
    uint64_t seed;
    uint32_t flags;              /* RT_FLAG_* */
    int32_t device;              /* HIP device ordinal */
    int32_t row_step;            /* tile row i is screen row y0 + i * row_step (0 or 1: contiguous rows);
                                    k > 1 interleaves rows across k workers (multi-GPU load balance) */
} rt_render_params;

typedef struct {
    int64_t samples;             /* camera samples traced = tile pixels * 4 * floor(spp/4) */
    int64_t vertices;            /* path vertices (extension rays that hit) */
    int64_t iterations;          /* wavefront bounce iterations (0 for the megakernel) */
    double device_ms;            /* device time of the render (HIP events on the render stream) */
    double kernel_ms[8];         /* per-stage device time (wavefront: extend, shade, shadow, regen, finalize) */
    int64_t kernel_launches[8];
} rt_render_stats;

/* Scene construction ---------------------------------------------------------------------- */
int rt_scene_load_toml(const char* toml_path, const char* assets_dir /* NULL: <toml dir>/assets */, rt_scene** out);
int rt_scene_create(const rt_scene_desc* desc, rt_scene** out);
void rt_scene_destroy(rt_scene* scene);

/* Scene inspection (host prep parity: octree shape etc.). info[16] int64:
 * [0]=objects [1]=light index [2]=meshes [3]=total octree nodes [4]=parents [5]=leaves
 * [6]=triangle refs [7]=triangles [8]=vertices [9]=max leaf size [10]=max leaf depth
 * [11]=1 if the octree walks use the child-slot tables (subtree culls), 0 if they read the plain child
 * tables (octrees whose node ids exceed the slot encoding, 2^23; same results either way) */
int rt_scene_info(const rt_scene* scene, int64_t info[16]);
/* Per-object mesh data after transforms: bbox[6], surface area, octree in DFS pre-order
 * (kind: 0 parent/1 leaf, child[8*n], leaf_off, leaf_cnt, refs). Any output pointer may be NULL. */
int rt_scene_mesh(const rt_scene* scene, int32_t object, int64_t counts[4] /* nodes, refs, tris, verts */,
                  double bbox[6], double* surface_area, double* vertices, uint32_t* indices,
                  int32_t* kind, int32_t* child, int32_t* leaf_off, int32_t* leaf_cnt, int32_t* refs);
/* The object BVH (host data, no GPU needed): for a scene that does not fit the kernels' small-scene
 * tables (more than 16 objects, 4 spheres, 4 axis planes per axis or 8 other objects) and has a sphere, the loader
 * builds a BVH over the spheres (binned SAH, leaves of at most 4); planes and meshes go on a rest list. This call
 * reports it. It is not part of the device scene: the kernels test every object of such a scene, as before.
 * counts: nodes, leaf refs (= spheres), rest-list length, depth of the deepest leaf (root = 0); all 0 without a tree.
 * Nodes are in DFS pre-order (an inner node's left child is the next node): boxes[n][6] = min xyz, max xyz;
 * count[n] = 0 for an inner node, whose a[n] is its right child and axis[n] its split axis, else the leaf's size,
 * its spheres being refs[a[n] .. a[n] + count[n]) (scene object indices, ascending). rest[] = the objects outside the
 * tree, in scene order. Any output pointer may be NULL. Views answer for their base. */
int rt_scene_object_bvh(const rt_scene* scene, int64_t counts[4] /* nodes, leaf refs, rest, depth */, double* boxes,
                        int32_t* a, int32_t* count, int32_t* axis, int32_t* refs, int32_t* rest);

/* Rendering ------------------------------------------------------------------------------- */
/* Host buffers: rgb_out tile_w*tile_h*3 u8; sub_out (optional) tile_w*tile_h*4*3 f64 subpixel
 * means before the clamp; cancel (optional; nonzero = stop, returns RT_CANCELLED): read by the
 * calling thread while the render runs and copied into a pinned word the megakernels poll between
 * subpixels (the wavefront: between bounce batches). The flag is never registered with HIP and may be
 * shared by concurrent renders. stats optional. */
int rt_render(const rt_scene* scene, const rt_render_params* params, uint8_t* rgb_out, double* sub_out,
              const volatile int32_t* cancel, rt_render_stats* stats);
/* Device buffers on params->device; enqueued on `stream` (hipStream_t, NULL = default stream).
 * Synchronous with respect to the stream only when stats != NULL. */
int rt_render_device(const rt_scene* scene, const rt_render_params* params, void* d_rgb, void* d_sub,
                     void* stream, rt_render_stats* stats);

/* One process, several devices (replaces the row-band fan-out of RenderJob::run,
 * server.rs:165-168): the tile's rows are cut into bands of `band_rows` tile rows (<= 0: about 8 bands per
 * worker) handed out dynamically from a host atomic counter to one worker thread per entry of `devices`
 * (an ordinal may repeat: several workers on one device). A worker renders each band with the device path on
 * its own streams (two bands in flight, so one band's tail overlaps the next band's start) and copies the RGB8
 * rows straight into rgb_out: the gather is host-side, no collective. The image is byte-identical to rt_render
 * of the same params (the RNG is keyed by global pixel). cancel is checked between bands and relayed to
 * the running bands' kernels as in rt_render. stats (optional):
 * samples and vertices summed over the bands, device_ms = wall time of the whole call.
 * Errors, checked before any band runs: RT_E_NODEVICE when no HIP device is visible (or the runtime is
 * absent), RT_E_INVAL for a device ordinal outside [0, device count). */
int rt_render_multi(const rt_scene* scene, const rt_render_params* params, const int32_t* devices, int32_t n_devices,
                    int32_t band_rows, uint8_t* rgb_out, const volatile int32_t* cancel, rt_render_stats* stats);
/* The band plan rt_render_multi hands out (no GPU): band b = tile rows [first_row[b], first_row[b] + rows[b]),
 * in handout order. Returns the band count; writes at most `cap` entries (either array may be NULL). */
int32_t rt_band_plan(int32_t tile_h, int32_t n_workers, int32_t band_rows, int32_t cap, int32_t* first_row,
                     int32_t* rows);

/* Scene::trace_ray on the device for n host rays: t, object id (-1: no hit), hit pos/normal. */
int rt_trace_rays(const rt_scene* scene, int32_t device, int64_t n, const double* origins, const double* dirs,
                  double* t, int32_t* object, double* pos, double* normal);
/* The same with render flags (RT_FLAG_MESH_NEAREST selects the nearest-triangle mesh semantics). */
int rt_trace_rays_flags(const rt_scene* scene, int32_t device, uint32_t flags, int64_t n, const double* origins,
                        const double* dirs, double* t, int32_t* object, double* pos, double* normal);

/* Denoised previews -------------------------------------------------------------- */
/* First-hit feature buffers of the tile of `params` (width, height, x0, y0, tile_w, tile_h, row_step, device and
 * RT_FLAG_MESH_NEAREST are used; spp, seed and the other flags are ignored). Per subpixel, the camera ray through the
 * tent filter's centre (the ray sample_pixel would trace with dx = dy = 0) is traced like rt_trace_rays; the pixel's
 * four results are summed as (s0 + s1) + (s2 + s3) in f64. feat_out: tile_w * tile_h * 8 floats, per pixel
 *   [0..2] mean hit normal (as rt_trace_rays reports it, not renormalised)   [3] mean hit distance t
 *   [4..6] mean albedo: clamp(base + emitted, 0, 1) per channel, base = k (diffuse, specular) or
 *          phong_kd * color_d + phong_ks * color_s (Phong)                   [7] coverage = hits / 4
 * each mean over the rays that hit, 0 when none did. */
int rt_render_features(const rt_scene* scene, const rt_render_params* params, float* feat_out);
/* The same into a device buffer on params->device, enqueued on `stream` (hipStream_t, NULL = default stream);
 * returns without waiting for the device. */
int rt_render_features_device(const rt_scene* scene, const rt_render_params* params, void* d_feat, void* stream);
/* Edge-avoiding a-trous wavelet filter. sub: width * height * 12 f64, rt_render's sub_out of the whole image being
 * filtered; feat: width * height * 8 floats as above. c0 = sum_j clamp(sub_j, 0, 1) * 0.25 (f64, rounded to f32); for
 * level i = 0 .. levels - 1, step s = 2^i, taps q = p + s (dx, dy), dx, dy in -2..2, inside the image, in row-major
 * (dy, dx) order, h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *   E = |c_p - c_q|^2 / (sigma_c 2^-i)^2 + |n_p - n_q|^2 / sigma_n^2
 *     + ((z_p - z_q) / (z_p + z_q + 1e-20))^2 / sigma_z^2 + (|a_p - a_q|^2 + (k_p - k_q)^2) / sigma_a^2
 *   c'_p = sum_q w c_q / sum_q w,   w = h[dx + 2] h[dy + 2] exp(-E)
 * (n, z, a, k: feat[0..2], [3], [4..6], [7]; f32 arithmetic). A sigma <= 0 drops its term. levels is 0..8; 0 is the
 * pass-through: rgb_out is then rt_render's rgb_out byte for byte. rgb_out: width * height * 3 u8 through rt_render's
 * gamma and `as u8`; lin_out (optional): width * height * 3 floats, the filtered linear colour. No hidden defaults:
 * every parameter is the caller's. */
int rt_denoise(int32_t device, int32_t width, int32_t height, const double* sub, const float* feat, int32_t levels,
               float sigma_c, float sigma_n, float sigma_z, float sigma_a, uint8_t* rgb_out, float* lin_out);
/* The same on device buffers of `device` (sub and feat 16-byte aligned), enqueued on `stream`; the call waits for the
 * filter. Its scratch (32 bytes per pixel) is freed before it returns, except that one idle buffer of at most 128 MiB is
 * kept for the next call. */
int rt_denoise_device(int32_t device, int32_t width, int32_t height, const double* sub, const float* feat,
                      int32_t levels, float sigma_c, float sigma_n, float sigma_z, float sigma_a, uint8_t* rgb_out,
                      float* lin_out, void* stream);

/* Progressive accumulation -------------------------------------------------------- */
/* An accumulator merges render passes of one width x height frame on one device and estimates each pixel's variance
 * from the pass-to-pass scatter. Its handle is an opaque pointer (void*: made by rt_accum_create, released by
 * rt_accum_destroy). It is not thread-safe: one call at a time per accumulator. Per subpixel and channel
 * (width * height * 12) it holds two f64 sums on the device,
 *   S = sum_k n_k m_k        Q = sum_k n_k m_k^2
 * m_k: pass k's subpixel mean (rt_render's sub_out, before the clamp), n_k = floor(spp_k / 4) its samples per
 * subpixel; on the host K (passes) and N = sum_k n_k. That is 192 bytes per pixel (398 MB at 1920 x 1080), allocated
 * by the first pass, plus a staging area of 115 bytes per pixel (a pass's sub, a variance image, an RGB8 frame:
 * 238 MB at 1920 x 1080) allocated by the first call that needs one (rt_accum_add, the host forms, an RGB8 resolve
 * without a sub buffer). rt_accum_create itself makes no device call.
 * Arithmetic, fixed so that a numpy restatement gives the same bits (no FMA contraction): per element
 *   S += (double)n * m;  Q += ((double)n * m) * m;      the first pass after create or reset stores without reading.
 * Every call waits for the device work it enqueued before it returns. */
int rt_accum_create(int32_t device, int32_t width, int32_t height, void** out);
void rt_accum_destroy(void* accum);
/* Forgets every pass (K = N = 0); the device memory is kept. */
int rt_accum_reset(void* accum);
/* info[4] = K, N, width, height */
int rt_accum_info(const void* accum, int64_t info[4]);
/* Renders `params` (rt_render's enqueue path: every flag passes through, the caller chooses the seed) into the
 * accumulator's staging buffer and merges it with n = floor(spp / 4). params must be the accumulator's whole frame:
 * its width, height and device, x0 = y0 = 0, tile_w = width, tile_h = height, row_step 0 or 1, spp >= 4; RT_E_INVAL
 * otherwise, before any device call. cancel and stats as in rt_render; a cancelled pass returns RT_CANCELLED and
 * leaves S, Q, K and N untouched. */
int rt_accum_add(void* accum, const rt_scene* scene, const rt_render_params* params, const volatile int32_t* cancel,
                 rt_render_stats* stats);
/* Merges a pass rendered elsewhere (another device's or host's rt_render sub_out of the whole frame; synthetic passes
 * in tests): sub is width * height * 12 f64 on the host, n >= 1 its samples per subpixel. */
int rt_accum_add_sub(void* accum, const double* sub, int32_t n);
/* The same from a device buffer of the accumulator's device (16-byte aligned), enqueued on `stream`. */
int rt_accum_add_sub_device(void* accum, const void* d_sub, int32_t n, void* stream);
/* The accumulated frame (K >= 1, else RT_E_INVAL); any output may be NULL.
 *   sub_out: width * height * 12 f64, S / N (IEEE division)
 *   rgb_out: width * height * 3 u8, sub_out through rt_render's clamp, average, gamma and `as u8` (k_finalize_f64)
 *   var_out: width * height * 4 floats (v_r, v_g, v_b, v_r + v_g + v_b); needs K >= 2, else RT_E_INVAL. The variance
 *            of the clamped pixel colour of the accumulated frame, through the clamp by the delta method: per
 *            subpixel j and channel, m = S / N, vs = max(0, Q / N - m m) / (K - 1);
 *            v_ch = (sum_{j = 0..3} [0 < m_j < 1] vs_j) / 16, summed in j order in f64; [3] = (v_r + v_g) + v_b in
 *            f64; each rounded to f32. */
int rt_accum_resolve(void* accum, double* sub_out, float* var_out, uint8_t* rgb_out);
/* The same into device buffers of the accumulator's device (d_sub and d_var 16-byte aligned), enqueued on `stream`. */
int rt_accum_resolve_device(void* accum, void* d_sub, void* d_var, void* d_rgb, void* stream);

/* Variance-guided a-trous filter: rt_denoise with the colour term scaled by the pixel's variance.
 * sub, feat, levels, sigma_n, sigma_z, sigma_a, rgb_out, lin_out: as rt_denoise. var: width * height * 4 floats as
 * rt_accum_resolve's var_out; only [3] is used, v0_p = max(var[p][3], 0). c0 as rt_denoise. Level i, s = 2^i, the
 * taps, their order and h of rt_denoise:
 *   g_p  = sum k[dx] k[dy] v_q / sum k[dx] k[dy],   q = p + s (dx, dy), dx, dy in -1..1, inside the image,
 *          k = (1/4, 1/2, 1/4), row-major (dy, dx) order
 *   E    = |c_p - c_q|^2 * (1 / (sigma_c^2 g_p + 1e-10)) + the normal, depth and albedo / coverage terms of rt_denoise
 *   w    = h[dx + 2] h[dy + 2] exp(-E),   c'_p = sum_q w c_q / sum_q w,   v'_p = sum_q w^2 v_q / (sum_q w)^2
 * (no 2^-i on sigma_c: the variance shrinks by itself; f32 arithmetic). sigma_c <= 0 drops the colour term; levels = 0
 * is rt_denoise's pass-through, byte for byte. var_out (optional): width * height floats, the filtered variance. */
int rt_denoise_var(int32_t device, int32_t width, int32_t height, const double* sub, const float* feat,
                   const float* var, int32_t levels, float sigma_c, float sigma_n, float sigma_z, float sigma_a,
                   uint8_t* rgb_out, float* lin_out, float* var_out);
/* The same on device buffers of `device` (sub, feat and var 16-byte aligned), enqueued on `stream`; the call waits
 * for the filter. Scratch as rt_denoise_device (32 bytes per pixel: the variance rides in the colour's fourth
 * component). */
int rt_denoise_var_device(int32_t device, int32_t width, int32_t height, const double* sub, const float* feat,
                          const float* var, int32_t levels, float sigma_c, float sigma_n, float sigma_z,
                          float sigma_a, uint8_t* rgb_out, float* lin_out, float* var_out, void* stream);

/* Rendering to a per-pixel error target ------------------------------------------- */
/* Renders only the listed pixels of the frame of `params`. pixels: n_pixels frame pixel ids, id = row * width + col
 * (row 0 = top), strictly ascending, each < width * height. params must be the whole frame, as rt_accum_add requires
 * it: x0 = y0 = 0, tile_w = width, tile_h = height, row_step 0 or 1. Entry e of the outputs is pixel pixels[e]:
 * sub_out[e] (12 f64) is rt_render's sub_out of that pixel for the same seed, spp and flags, bit for bit, and
 * rgb_out[e] its RGB8, byte for byte. The f64 fused megakernel's own body runs it (its list instance k_render_list_f64), or, for
 * a mesh scene whose full frame runs a pool kernel, that kernel's pixel-list instance (rt_render_pixels_path names the
 * family; the bits are the same whichever runs):
 * RT_FLAG_MIS passes through, RT_FLAG_MEGAKERNEL is implied; RT_FLAG_FP32 and RT_FLAG_MESH_NEAREST are out of scope
 * (RT_E_INVAL). n_pixels * 4 must fit an int32. The host form checks the list (RT_E_INVAL before any device call);
 * n_pixels = 0 returns RT_OK without a launch and leaves the outputs untouched. cancel and stats as in rt_render;
 * stats->samples = n_pixels * 4 * floor(spp / 4). Every argument check runs without a GPU. */
int rt_render_pixels(const rt_scene* scene, const rt_render_params* params, const uint32_t* pixels, int64_t n_pixels,
                     uint8_t* rgb_out /* n * 3, may be NULL */, double* sub_out /* n * 12, may be NULL */,
                     const volatile int32_t* cancel, rt_render_stats* stats);
/* The same with device buffers on params->device (d_pixels 4-byte, d_sub 16-byte aligned; d_rgb, d_sub nullable),
 * enqueued on `stream`; synchronous with respect to the stream only when stats != NULL. A strictly ascending
 * in-range list is the caller's contract here: it is not checked. */
int rt_render_pixels_device(const rt_scene* scene, const rt_render_params* params, const void* d_pixels,
                            int64_t n_pixels, void* d_rgb, void* d_sub, void* stream, rt_render_stats* stats);

/* The kernel family of a pixel-list render. */
#define RT_LIST_AUTO  0
#define RT_LIST_FUSED 1   /* k_render_list_f64, the fused megakernel's list instance */
#define RT_LIST_FPOOL 2   /* the flat-octree query pool */
#define RT_LIST_ROLES 3   /* the role-split pool */
/* path_out[0]: the kernel family rt_render_pixels takes for this scene, these params and a list of n_pixels;
 * path_out[1]: the pool family this scene and these flags have at all (RT_LIST_FUSED: none). params and n_pixels
 * are checked as rt_render_pixels checks them. No GPU needed. */
int rt_render_pixels_path(const rt_scene* scene, const rt_render_params* params, int64_t n_pixels, int32_t path_out[2]);
/* rt_render_pixels with the family chosen by the caller: RT_LIST_AUTO is rt_render_pixels; a family the scene has
 * no instance of is RT_E_INVAL before any device call. Same bits whichever family runs. */
int rt_render_pixels_with(const rt_scene* scene, const rt_render_params* params, const uint32_t* pixels,
                          int64_t n_pixels, int32_t path, uint8_t* rgb_out, double* sub_out,
                          const volatile int32_t* cancel, rt_render_stats* stats);
/* rt_render_pixels_device with the family chosen by the caller, by the same rules. */
int rt_render_pixels_with_device(const rt_scene* scene, const rt_render_params* params, const void* d_pixels,
                                 int64_t n_pixels, int32_t path, void* d_rgb, void* d_sub, void* stream,
                                 rt_render_stats* stats);

/* Sparse passes into an accumulator. The first sparse merge gives the accumulator per-pixel counts (K_p, N_p), 8 bytes
 * per pixel (allocated together with a pixel-list buffer and the selection's scratch, about 12.2 bytes per pixel in
 * all, by the first sparse merge or selection), filled with the frame's (K, N) at that moment; from then on a full-frame merge adds (1, n) to every
 * pixel, a sparse merge to the listed ones, and rt_accum_resolve uses N_p and K_p - 1 where it used N and K - 1. An
 * accumulator that never receives a sparse pass computes exactly what it did before. A sparse merge needs K >= 2
 * full-frame passes first (RT_E_INVAL otherwise), so every K_p >= 2. rt_accum_info keeps reporting the full-frame
 * passes' K and N only; rt_accum_reset forgets the per-pixel counts too.
 * rt_accum_add_pixels renders the listed pixels (rt_render_pixels' rules for params, flags and the list; spp >= 4 and
 * params->device the accumulator's) into the staging buffer and merges them with n = floor(spp / 4); a cancelled pass
 * returns RT_CANCELLED and merges nothing. */
int rt_accum_add_pixels(void* accum, const rt_scene* scene, const rt_render_params* params, const uint32_t* pixels,
                        int64_t n_pixels, const volatile int32_t* cancel, rt_render_stats* stats);
/* Merges a compact pass rendered elsewhere: sub[e] (12 f64, host) belongs to pixel pixels[e] (host; strictly
 * ascending, each < width * height, checked), n >= 1 its samples per subpixel. n_pixels = 0 merges nothing. */
int rt_accum_add_sub_pixels(void* accum, const uint32_t* pixels, int64_t n_pixels, const double* sub, int32_t n);
/* The same from device buffers of the accumulator's device (d_sub 16-byte aligned), enqueued on `stream`; the list
 * is the caller's contract (unique ids in range). */
int rt_accum_add_sub_pixels_device(void* accum, const void* d_pixels, int64_t n_pixels, const void* d_sub, int32_t n,
                                   void* stream);
/* The per-pixel maps K_p and N_p (width * height uint32 each, host, either may be NULL); the frame's K and N
 * everywhere while no sparse pass has been merged (then without a device call). */
int rt_accum_counts(void* accum, uint32_t* k_out, uint32_t* n_out);
/* The pixels whose estimated error is still above a target (K >= 2; tolerances >= 0 and not NaN; RT_E_INVAL
 * otherwise). Arithmetic, fixed in f64 without FMA contraction so that numpy gives the same bits: with var the
 * resolve's var_out and m = S / N_p,
 *   g_p = sum k[dx] k[dy] (double)var[q][3] / sum k[dx] k[dy],   q = p + (dx, dy), dx, dy in -1..1, inside the image,
 *         row-major (dy, dx) order, k = (1/4, 1/2, 1/4) (the tent of rt_denoise_var)
 *   c   = sum_j clamp(m_j, 0, 1) * 0.25 in j order,   y = (c_r + c_g) + c_b
 *   thr = ((double)rel_tol * y) / 3.0 + (double)abs_tol
 * pixel p is active iff g_p > thr * thr and (max_n <= 0 or N_p < max_n). pixels_out receives the active ids in
 * ascending order, at most cap of them (cap >= 0; pixels_out may be NULL when cap = 0); *n_out is always the full
 * count. */
int rt_accum_select(void* accum, float abs_tol, float rel_tol, int32_t max_n, uint32_t* pixels_out, int64_t cap,
                    int64_t* n_out);
/* The same into a device buffer of the accumulator's device, enqueued on `stream`; the call waits for the selection
 * and then writes *n_out on the host. */
int rt_accum_select_device(void* accum, float abs_tol, float rel_tol, int32_t max_n, void* d_pixels, int64_t cap,
                           int64_t* n_out, void* stream);

/* Camera views and accumulator reprojection ---------------------------------------- */
/* A camera: position, viewing direction, the image's right-hand direction and the vertical field factor of
 * server.rs:330 (0.5135 there). On the wire a view is its 10 doubles in this order (pos, dir, right, fov): the calls
 * below take `const double view[10]`, which is what a `const rt_view*` points to (no padding; cast it). */
typedef struct { double pos[3], dir[3], right[3]; double fov; } rt_view;
/* A scene handle that shares base's host data, packed tables, device uploads and workspace pool, with its own camera.
 * No device call, no copy of the geometry. A view of a view refers to the root base. The base must outlive its views
 * (the caller's contract); rt_scene_destroy releases a view without touching shared data. Every entry point that takes
 * an rt_scene* accepts a view and behaves as if the base had been created with that camera (rt_scene_info and
 * rt_scene_mesh answer for the base). Camera frame, with w, h the image size as doubles (server.rs:328-331 at
 * right = (1, 0, 0), fov = 0.5135, bit for bit):
 *   s = w * fov / h;   cx = right * s per component;   cy = norm(cross(cx, dir)) * fov
 * dir and right are used as given (right's length scales the horizontal field). RT_E_INVAL, without a GPU, for a null
 * argument, a non-finite component, fov <= 0, or cross(right, dir) zero or not finite. */
int rt_scene_view(const rt_scene* base, const double view[10], rt_scene** out);
/* The camera of a scene or view; a loaded / created scene reports right = (1, 0, 0), fov = 0.5135. */
int rt_scene_get_view(const rt_scene* scene, double view_out[10]);

/* Seeds accumulator dst (view dst_view) from accumulator src (view src_view) of the same width, height and device.
 * flags: 0 or RT_FLAG_MESH_NEAREST. max_n >= 1: the most samples per subpixel of history a pixel may inherit.
 * *n_valid (nullable): dst pixels that received history. RT_E_INVAL, before any device call, for a null handle,
 * dst == src, different size or device, views that do not share a base, src with K < 2, max_n < 1, an unknown flag.
 * Arithmetic: f64 without FMA contraction, so that numpy gives the same bits. With
 *   cross(a, b) = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x),  dot(a, b) = (a_x b_x + a_y b_y) + a_z b_z,
 * pos_s, dir_s the src view's camera and cx_s, cy_s its frame at this width and height, the host computes
 *   D = dot(cx_s, cross(cy_s, dir_s))
 *   A = cross(cy_s, dir_s) / D,   B = cross(dir_s, cx_s) / D,   C = cross(cx_s, cy_s) / D     (per component)
 * For dst pixel p (id = row * width + col, row 0 = top) and subpixel j = 2 sy + sx (rt_render's order):
 *  1. the dst view's camera ray through the tent filter's centre (rt_render_features' ray) is traced like
 *     rt_trace_rays_flags(flags); a miss is invalid;
 *  2. the hit object's BRDF must be RT_BRDF_DIFFUSE (emission allowed), anything else is invalid; x, n = the hit
 *     position and normal as rt_trace_rays reports them (n faces the dst camera);
 *  3. v = x - pos_s;  al = dot(v, A), be = dot(v, B), ga = dot(v, C); invalid unless ga > 0;
 *  4. fx = (al / ga + 0.5) * w,  fy = (be / ga + 0.5) * h; invalid unless 0 <= fx < w and 0 <= fy < h (NaN fails);
 *     col' = floor(fx), sx' = floor((fx - col') * 2), yref = floor(fy), sy' = floor((fy - yref) * 2),
 *     row' = height - 1 - yref; the source is subpixel j' = 2 sy' + sx' of pixel q = row' * width + col' (nearest
 *     subpixel, no interpolation);
 *  5. invalid unless dot(n, pos_s - x) > 0 (the src camera is on the side the dst camera sees);
 *  6. invalid unless Scene::mutually_visible(x, pos_s) (scene.rs:258-270, the shadow query of rt_render).
 * The pixel is valid iff its four subpixels are. With (K_q, N_q) the src counts of each subpixel's source pixel
 * (rt_accum_counts of src), all integers 64-bit:
 *   N_p = min(max_n, min_j N_qj)        K_p = max(2, min_j ceil(K_qj * N_p / N_qj))
 *   S_dst[p][j][c] = (double)N_p * (S_src[q_j][j'][c] / (double)N_qj),  Q_dst likewise from Q_src,  counts (K_p, N_p)
 * (dividing first keeps the subpixel mean and Q / N - m m; K scales with N: the shortened history counts as fewer
 * passes of the same size). An invalid pixel gets zeros in all 24 sums and counts (0, 0); every dst entry is written.
 * Afterwards dst is reset and seeded: its per-pixel counts are live, rt_accum_info reports K = N = 0 (the full-frame
 * passes since the reprojection), and the next merge adds to the seeded sums instead of storing. rt_accum_reset
 * clears the seeded state. rt_accum_resolve keeps its K >= 1 rule and the variance its K >= 2 rule: after two
 * full-frame passes every K_p >= 2, so rt_accum_select and the sparse merges work unchanged. src is only read. */
int rt_accum_reproject(void* dst, void* src, const rt_scene* dst_view, const rt_scene* src_view, uint32_t flags,
                       int32_t max_n, int64_t* n_valid);

/* Filling the holes of a reprojection ---------------------------------------------- */
/* The pixels of a seeded accumulator (one that rt_accum_reproject wrote as dst, until rt_accum_reset or the next
 * reprojection into it) that need samples. Pixel p = row * width + col is listed iff
 *   K_p < 2   (a hole: no history, or not yet two passes), or
 *   period > 0 and (col + 3 * row) mod period == phase   (the refresh pattern: every pixel once in `period` views).
 * period >= 0, 0 <= phase < max(period, 1), cap >= 0 (pixels_out may be NULL when cap = 0), a non-null accum and n_out,
 * a seeded accumulator: RT_E_INVAL otherwise, before any device call (the seeded state is asked for last).
 * pixels_out receives the ids in ascending order, at most cap of them; *n_out is always the full count, *n_holes
 * (nullable) the count of pixels with K_p < 2. The list is deterministic: a ballot compaction, no atomics on the
 * order. */
int rt_accum_holes(void* accum, int32_t period, int32_t phase, uint32_t* pixels_out, int64_t cap, int64_t* n_out,
                   int64_t* n_holes);
/* The same into a device buffer of the accumulator's device, enqueued on `stream`; the call waits for the list and
 * then writes *n_out and *n_holes on the host. */
int rt_accum_holes_device(void* accum, int32_t period, int32_t phase, void* d_pixels, int64_t cap, int64_t* n_out,
                          int64_t* n_holes, void* stream);
/* Two sparse passes that give every hole of a seeded accumulator two passes. params as rt_accum_add_pixels takes them
 * (the whole frame, the accumulator's device, spp >= 4; RT_FLAG_MIS passes through, RT_FLAG_FP32 and
 * RT_FLAG_MESH_NEAREST are RT_E_INVAL); period and phase as rt_accum_holes. Every check runs before any device call.
 *   pass 1 renders the list of rt_accum_holes(period, phase) with params->seed and merges it with n = floor(spp / 4);
 *   pass 2 renders the pixels that still have K_p < 2 with seed2 and merges them the same way.
 * The lists stay on the device; an empty list launches nothing. fill_out (nullable) receives the two lists' lengths,
 * stats (nullable) the two renders' sums (samples = (fill_out[0] + fill_out[1]) * 4 * floor(spp / 4)). A hole's sums
 * are zeros, so afterwards it holds S = n m1 + n m2 with counts (2, 2 n): bit for bit what two rt_accum_add calls with
 * the same seeds and spp give that pixel. A refreshed pixel with history gains (1, n).
 * On RT_OK the accumulator is covered: every K_p >= 2, and it is accepted wherever K >= 1 or K >= 2 is asked for
 * (rt_accum_resolve* with the variance, rt_accum_select*, rt_accum_add_pixels, rt_accum_add_sub_pixels*, src of
 * rt_accum_reproject) although rt_accum_info keeps reporting the full-frame passes since the reprojection, possibly 0.
 * rt_accum_reset and rt_accum_reproject (on dst) clear the state; full-frame merges keep it. A cancelled pass merges
 * nothing and returns RT_CANCELLED (the passes before it stay merged); the accumulator is then not covered, and a
 * later rt_accum_fill completes it. */
int rt_accum_fill(void* accum, const rt_scene* scene, const rt_render_params* params, uint64_t seed2, int32_t period,
                  int32_t phase, const volatile int32_t* cancel, rt_render_stats* stats, int64_t fill_out[2]);

/* Batched passes: several error-target passes per pixel in one launch ---------------- */
/* The most passes one list entry may hold, and so the most seeds a call takes. */
#define RT_PASSES_MAX 16
/* rt_render_pixels with a pass count per listed pixel and a seed per pass. Entry e of the list has counts[e] passes,
 * each count in 1 .. n_seeds, n_seeds in 1 .. RT_PASSES_MAX; unit-group u = off[e] + i is pass i of pixel pixels[e],
 * off the exclusive prefix sum of counts, and the outputs are indexed by unit-group: sub_out[off[e] + i] (12 f64) is,
 * bit for bit, rt_render_pixels' sub_out of pixel pixels[e] for the seed seeds[i] and the same spp and flags, and
 * rgb_out[off[e] + i] its RGB8. params->seed is ignored. params, flags and the list: rt_render_pixels' rules
 * (RT_FLAG_MIS passes through; RT_FLAG_FP32 and RT_FLAG_MESH_NEAREST are RT_E_INVAL); in addition width * height must
 * be below 2^28 and the unit total sum(counts) at most width * height (RT_E_INVAL, before any device call). The
 * family rule is the pixel list's: the fused megakernel's body runs it (k_render_passes_f64), or, for a mesh scene
 * whose full frame runs a pool kernel, that kernel's passes instance; rt_render_pixels_path answers for
 * a batched render too, and the bits are the same whichever runs.
 * n_pixels = 0 returns RT_OK without a launch. cancel and stats as in rt_render;
 * stats->samples = units * 4 * floor(spp / 4). Every argument check runs without a GPU. */
int rt_render_pixel_passes(const rt_scene* scene, const rt_render_params* params, const uint32_t* pixels,
                           const uint8_t* counts, int64_t n_pixels, const uint64_t* seeds /* host */, int32_t n_seeds,
                           uint8_t* rgb_out /* units * 3, may be NULL */, double* sub_out /* units * 12, may be NULL */,
                           const volatile int32_t* cancel, rt_render_stats* stats);
/* The same with device lists and outputs on params->device (d_sub 16-byte aligned; d_rgb, d_sub nullable), enqueued on
 * `stream`. units: the sum of the counts (rt_accum_plan reports it), n_pixels <= units <= width * height. The list
 * (strictly ascending ids in range, counts in 1 .. n_seeds that add up to units) is the caller's contract. seeds stay
 * on the host. The list is expanded on the device into scratch memory that lives for the call, so the call waits for
 * the render before it returns. */
int rt_render_pixel_passes_device(const rt_scene* scene, const rt_render_params* params, const void* d_pixels,
                                  const void* d_counts, int64_t n_pixels, int64_t units, const uint64_t* seeds,
                                  int32_t n_seeds, void* d_rgb, void* d_sub, void* stream, rt_render_stats* stats);
/* rt_render_pixel_passes with the family chosen by the caller, by rt_render_pixels_with's rules: RT_LIST_AUTO is
 * rt_render_pixel_passes (the scene's pool wherever it has one); an unknown family, or one the scene has no instance
 * of (rt_render_pixels_path's path_out[1] names the one it has), is RT_E_INVAL before any device call. Same bits
 * whichever family runs. rt_accum_add_passes and rt_accum_refine follow RT_LIST_AUTO. */
int rt_render_pixel_passes_with(const rt_scene* scene, const rt_render_params* params, const uint32_t* pixels,
                                const uint8_t* counts, int64_t n_pixels, const uint64_t* seeds /* host */,
                                int32_t n_seeds, int32_t path, uint8_t* rgb_out, double* sub_out,
                                const volatile int32_t* cancel, rt_render_stats* stats);
/* rt_render_pixel_passes_device with the family chosen by the caller, by the same rules. */
int rt_render_pixel_passes_with_device(const rt_scene* scene, const rt_render_params* params, const void* d_pixels,
                                       const void* d_counts, int64_t n_pixels, int64_t units, const uint64_t* seeds,
                                       int32_t n_seeds, int32_t path, void* d_rgb, void* d_sub, void* stream,
                                       rt_render_stats* stats);
/* rt_accum_select plus a pass count per listed pixel: how many passes of n samples per subpixel the pixel should get
 * at once. n >= 1, gain in (0, 1] (the share of the predicted need to hand out), max_passes = C in 1 .. RT_PASSES_MAX,
 * tolerances and K as rt_accum_select, width * height < 2^28; RT_E_INVAL otherwise, before any device call. For a pixel
 * that rt_accum_select(abs_tol, rel_tol, max_n) lists, with its g_p, thr and N_p, in f64 without FMA contraction:
 *   r    = g_p / (thr * thr)                      (IEEE; +inf when thr = 0)
 *   need = (double)N_p * r - (double)N_p
 *   x    = ((double)gain * need) / (double)n
 *   c    = x >= C ? C : max(1, (int)ceil(x))
 *   max_n > 0: c = min(c, (max_n - N_p + n - 1) / n)           (integers; >= 1 because N_p < max_n)
 * A launch never holds more than a frame's worth of units: with H[c] the histogram of the counts, C' is the largest
 * value in 1 .. C with sum_c H[c] min(c, C') <= width * height (C' = 1 always fits), and the final count is
 * min(c, C'). pixels_out: the ids, ascending, identical to rt_accum_select's list; counts_out: their final counts; at
 * most cap of each (cap >= 0; both may be NULL when cap = 0). *n_out: the list's full length; *units_out (nullable):
 * the sum of all final counts; *passes_out (nullable): the largest final count (0 for an empty list). */
int rt_accum_plan(void* accum, float abs_tol, float rel_tol, int32_t max_n, int32_t n, float gain, int32_t max_passes,
                  uint32_t* pixels_out, uint8_t* counts_out, int64_t cap, int64_t* n_out, int64_t* units_out,
                  int64_t* passes_out);
/* The same into device buffers of the accumulator's device, enqueued on `stream`; the call waits for the plan and then
 * writes the three totals on the host. */
int rt_accum_plan_device(void* accum, float abs_tol, float rel_tol, int32_t max_n, int32_t n, float gain,
                         int32_t max_passes, void* d_pixels, void* d_counts, int64_t cap, int64_t* n_out,
                         int64_t* units_out, int64_t* passes_out, void* stream);
/* Renders the listed pixels' passes (rt_render_pixel_passes' rules for params, seeds, the list and the counts; spp >= 4
 * and params->device the accumulator's) into the staging buffer and merges each entry's counts[e] units in pass order
 * with n = floor(spp / 4): per element and pass S += (double)n * m; Q += ((double)n * m) * m, then (K_p, N_p) +=
 * (counts[e], counts[e] * n). The result is, bit for bit, what the loop
 *   for i in 0 .. max(counts) - 1: rt_accum_add_pixels({pixels[e] : counts[e] > i}, seed = seeds[i])
 * gives. Needs K >= 2 as every sparse merge does. A cancelled call merges nothing and returns RT_CANCELLED. */
int rt_accum_add_passes(void* accum, const rt_scene* scene, const rt_render_params* params, const uint64_t* seeds,
                        int32_t n_seeds, const uint32_t* pixels, const uint8_t* counts, int64_t n_pixels,
                        const volatile int32_t* cancel, rt_render_stats* stats);
/* rt_accum_plan(abs_tol, rel_tol, max_n, n = floor(spp / 4), gain, max_passes = n_seeds) followed by
 * rt_accum_add_passes of the planned lists, which stay on the device (as rt_accum_fill's do): only the histogram and
 * the totals are read back. out (nullable) = (pixels, units, passes used: the largest final count). An empty plan
 * launches nothing and returns RT_OK. Every check runs before any device call. */
int rt_accum_refine(void* accum, const rt_scene* scene, const rt_render_params* params, float abs_tol, float rel_tol,
                    int32_t max_n, float gain, const uint64_t* seeds, int32_t n_seeds, const volatile int32_t* cancel,
                    rt_render_stats* stats, int64_t out[3]);

const char* rt_last_error(void);
int rt_abi_version(void);
int rt_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* RT_FFI_H */
