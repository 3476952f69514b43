/*
 * rt_diag.h — diagnostics exported by librtamd.so next to the C ABI of rt_ffi.h (not part of the
 * drop-in surface; used by tests and tools/).
 */
#ifndef RT_DIAG_H
#define RT_DIAG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* Device self-test of the exact-arithmetic shortcuts (path_f64.h: rcp_rn, qdiv, sqrt_rn, div_sqrt)
 * against the IEEE operations on n pseudo-random operands on the current HIP device; writes
 * min(n_out, 5) counts: out[0] = reciprocal mismatches, out[1] = quotient mismatches, out[2] =
 * square-root mismatches (sqrt_rn's fast range [2^-767, 2^1024) against the library sqrt), out[3] =
 * mismatches of the fused normalise div_sqrt(a, x) against a / sqrt(x) (library sqrt, IEEE division)
 * over that range, out[4] = mismatches of div_sqrt, sqrt_rn, rcp_any and V3 / s against the library
 * forms where every fourth wave holds one lane outside the fast ranges (0, subnormal, 2^-800, 2^+-1000,
 * inf, NaN, negative) or at an edge of them (2^900 and its neighbours, around 2^-900 and 2^-767, the largest
 * finite double); two NaNs are equal: a lane's bits do not depend on its wave-mates. Returns 0 or -1. */
int rt_selftest_arith_n(long n, unsigned long long seed, unsigned long long* out, int n_out);
/* The original entry point: out[0] reciprocal and out[1] quotient mismatches only. */
int rt_selftest_arith(long n, unsigned long long seed, unsigned long long out[2]);
/* Device round trips of the pointers every trace call rebuilds (no dereference: any 64-bit pattern is
 * safe): for each of the n addresses p = ptrs[i], a kernel launched with DevScene.ctab = p,
 * DevScene.node_slot = p + 16 and RenderArgs.tail_buf = p + 32 as its first two (kernarg) arguments
 * writes out[6i + k]: k = 0 tables() through the kernarg view, 1 tables() of the by-value argument,
 * 2 the round-4 sign-extending form (wrong whenever bit 31 of p is set: kept to show the check catches
 * it), 3 the kernarg view's ctab, 4 its node_slot, 5 the kernarg RenderArgs' tail_buf. Returns 0 or -1. */
int rt_selftest_tables(const unsigned long long* ptrs, int n, unsigned long long* out);
/* RT_QCHECK builds (-DRT_QCHECK=1): counters of LDS hand-off protocol violations in the megakernels'
 * work queues since the last call (kernels/megakernel_common.h): [0] ring slot overwritten / bad
 * entry, [1] queue over capacity, [2] outstanding-query count below zero, [3] owner/taker state
 * mismatch. Returns 0, 1 when the checks are not compiled in (zeros), -1 on a HIP error. */
int rt_debug_qcheck(unsigned long long out[4]);
/* RT_DEBUG_COUNTERS builds: octree traversal counters since the last call (zeros otherwise):
 * [0] walks [1] past the cull [2] node visits [3] leaves opened [4] triangle tests [5] walk steps;
 * interleaved mesh megakernel: [8] wave iterations [9] lanes in the vertex phase [10] walk-loop
 * wave steps [11] walking lanes summed over those steps. */
int rt_debug_counters(unsigned long long out[16]);
/* RT_DEBUG_COUNTERS builds: lane utilisation per instrumented code region (RT_DBG_REGION) since
 * the last call: out[2i] = wave entries into region i, out[2i+1] = active lanes summed over them
 * (i < 16); RT_DEBUG_TIMERS builds: out[32 + i] = s_memtime ticks of the megakernel's waves in timed
 * region i (RT_DBG_TSTART / RT_DBG_TEND), summed over waves. */
int rt_debug_regions(unsigned long long out[64]);
/* The split tail (kernels/megakernel_common.h plan_tail) of the calling thread's last f64 megakernel
 * render: out[0] = subpixels handed out as sample chunks (0: none split; only when spp / 4 >= 64),
 * out[1] = how many the kernel family wanted before the scratch buffer capped it (out[0] < out[1]: the
 * buffer was too small; the frame is the same, only the end of the launch balances worse), out[2] =
 * samples per chunk. Returns 0. */
int rt_debug_last_split(long long out[3]);
/* RT_DEBUG_TIMERS builds: per wave of the last analytic-scene megakernel launches (k_megakernel_f64), on the
 * constant 100 MHz s_memrealtime clock: out[5w] its start, out[5w + 1] when fewer than half of its lanes
 * last held work (all ones: never), out[5w + 2] its end (zeros: wave w did not run), and for the lane of it
 * that ran out of work last: out[5w + 3] when it took its last unit, out[5w + 4] that unit (ticket); then
 * cleared. For
 * n_waves <= 8192. Returns 0, 1 without the timers (zeros), -1 on a HIP error. */
int rt_debug_wave_times(unsigned long long* out, int n_waves);

/* Batch queries through the query code of one kernel family, one lane per query (tests/test_gpu_queries.py
 * compares every form with the CPU oracle ray by ray). `form` names whose code answers the queries:
 *   RT_DIAG_FUSED        trace_closest<C> / visible<C> (x, y -> div_sqrt -> visible_ray) with C as k_trace_f64
 *                        chooses it: the fused mesh instances of k_megakernel_f64; with RT_FLAG_MESH_NEAREST the
 *                        BVH walks of the nearest-triangle mode.
 *   RT_DIAG_FUSED_G0     the same through the even-F instance that k_megakernel_f64<8, 4> runs for a mesh-free
 *                        compact scene (the round-7 range guards); RT_E_INVAL for a scene with meshes.
 *   RT_DIAG_SPLIT_SLOTS  trace_analytic / visible_analytic, mesh_near_mask (the f32 cull) at the analytic t (or
 *                        infinity) resp. |y - x|, then the slot walk (walk_step<true>) of each near mesh in gen
 *                        order, begun as the pools begin it, merged by consider resp. occluded iff a walk's hit has
 *                        !(t + 0.001 >= |y - x|): k_megakernel_roles_f64 and k_megakernel_mesh_f64's walk pool.
 *   RT_DIAG_SPLIT_KIDS   the same split with the node_kids walk (walk_step<false>) begun with its own f64 cull for
 *                        every mesh of a candidate ray: the wavefront's k_wf_mesh_closest / k_wf_shadow_mesh.
 *   RT_DIAG_SPLIT_FLAT   the same split with flat_query per near mesh: k_megakernel_fpool_f64; RT_E_INVAL unless
 *                        every mesh of the scene is a flat octree (and there are at most two).
 *   RT_DIAG_FUSED_G1     the fused form through the instances k_megakernel_f64<odd, 3> runs for a compact scene with
 *                        meshes: the one-ballot range guards those keep (path_f64.h kCfgGuards1), which k_trace_f64's
 *                        choice of C does not carry; octree walks, or the BVH with RT_FLAG_MESH_NEAREST.
 * The split forms and FUSED_G1 need a compact scene with meshes; only FUSED and FUSED_G1 take a flag (RT_E_INVAL
 * otherwise); flags: 0 or RT_FLAG_MESH_NEAREST (rt_ffi.h). Host arrays. A null pointer (near_mask may be null),
 * n < 0, an unknown form or flag: RT_E_INVAL; then n == 0: RT_OK; then no visible HIP device: RT_E_NODEVICE. */
#define RT_DIAG_FUSED 0
#define RT_DIAG_FUSED_G0 1
#define RT_DIAG_SPLIT_SLOTS 2
#define RT_DIAG_SPLIT_KIDS 3
#define RT_DIAG_SPLIT_FLAT 4
#define RT_DIAG_FUSED_G1 5
struct rt_scene;
/* Scene::trace_ray for n rays (o, d: [n][3]): t[n] (0 for a miss), obj[n] (-1 for a miss), prim[n] (the hit
 * triangle's scene-wide index, -1 unless a mesh was hit), pos / nrm [n][3] through surface<> as k_trace_f64
 * (zeros for a miss). The split forms' near mask comes out of rt_diag_visible only: a mesh culled wrongly here
 * shows as a different hit object. */
int rt_diag_trace(const struct rt_scene* scene, int32_t device, int32_t form, uint32_t flags, int64_t n, const double* o,
                  const double* d, double* t, int32_t* obj, int32_t* prim, double* pos, double* nrm);
/* Scene::mutually_visible for n segments (x, y: [n][3]): vis[n] = 1 visible, 0 occluded; near_mask[n] (may be
 * null): the mask of meshes the split form's cull let through (bit m: mesh m; computed whether or not an
 * analytic object already blocks the segment), 0 for the fused forms. */
int rt_diag_visible(const struct rt_scene* scene, int32_t device, int32_t form, uint32_t flags, int64_t n, const double* x,
                    const double* y, uint8_t* vis, uint32_t* near_mask);

/* Batch path vertices through the integrator of one kernel family, one lane per vertex (tests/test_gpu_vertices.py
 * compares every form with the CPU oracle's orc_vertex vertex by vertex). A lane loads the state a render lane would
 * hold on arrival at the vertex, traces its ray with the form's trace_closest<C>, calls the form's shade_vertex
 * (csrc/device/integrator_f64.h) and stores the state it would carry on. Rows (host arrays):
 *   st[n][19]   ray origin, ray direction, beta, L, bemit, o (3 doubles each), pdf_prev
 *   rng[n][2]   the sample's xoroshiro128++ state
 *   dk[n][2]    depth, kind (0 camera vertex, 1 after a mirror bounce, 2 after a diffuse bounce)
 * st_out / rng_out / dk_out: the same rows after the vertex (bemit and o as the form's Cold holds them; a row whose
 * ray misses is unchanged; the stream's state is stored when Russian roulette passed, as in the render loops);
 * info[n][4]: hit object (-1 miss), the returned continue flag, ShadowDefer::pending and ::meshes (0 for the fused
 * forms). `form` names the instantiation, with the Cfg bits its render kernel takes for this scene and flags:
 *   RT_DIAG_FUSED      shade_vertex<C> with RegCold and no deferral, C as k_trace_f64 chooses it (the mesh code
 *                      compiled in) plus the scene's Phong bit and the MIS flag
 *   RT_DIAG_FUSED_G0   the same through the even-F instance of a mesh-free scene
 *   RT_DIAG_FUSED_G1   the same through the kCfgGuards1 instances of a scene with meshes
 *   RT_DIAG_FUSED_LDS  the fused megakernel's own instantiation (render_f64.hip fused_body): the object table in LDS,
 *                      the one-ballot guards for a scene with meshes, LdsCold on a [6][256] LDS column per thread
 * The deferred-shadow forms trace with the form's split (rt_diag_trace), call shade_vertex with a ShadowDefer as the
 * form's render kernel does, and resolve a pending shadow query the way that kernel family does: the form's walk
 * of each mesh in ShadowDefer::meshes, occluded iff a hit has !(t + 0.001 >= dist); ShadowDefer::c is added to L iff
 * no mesh occludes:
 *   RT_DIAG_SPLIT_SLOTS  the walk pool's instantiation (render_mesh_f64.hip: the object table in LDS, RegCold, the
 *                        shadow ray returned in the ShadowDefer), slot walks
 *   RT_DIAG_SPLIT_ROLES  the roles pool's instantiation (the same with LdsQuerySink: the shadow ray written to LDS
 *                        columns and read back from there), slot walks; rt_diag_vertex only
 *   RT_DIAG_SPLIT_KIDS   k_wf_shade's instantiation (wavefront_f64.hip), node_kids walks of every mesh
 *   RT_DIAG_SPLIT_FLAT   the query pool's instantiation (render_flat_f64.hip: its nospec bit for a scene without
 *                        mirror or Phong objects, LdsCold otherwise, LdsQuerySink), the shadow ray read back from the
 *                        LDS query columns and resolved with flat_query
 * flags: RT_FLAG_MIS, and RT_FLAG_MESH_NEAREST for the fused forms but FUSED_G0 (rt_ffi.h). Compact scenes only; the
 * split forms ask of the scene what they ask in rt_diag_trace. A null pointer, n < 0, an unknown form or flag, a
 * form the scene does not admit: RT_E_INVAL; then n == 0: RT_OK; then no visible HIP device: RT_E_NODEVICE. */
#define RT_DIAG_FUSED_LDS 6
#define RT_DIAG_SPLIT_ROLES 7
int rt_diag_vertex(const struct rt_scene* scene, int32_t device, int32_t form, uint32_t flags, int64_t n, const double* st,
                   const uint64_t* rng, const int32_t* dk, double* st_out, uint64_t* rng_out, int32_t* dk_out,
                   int32_t* info);
/* The device sincos_2pi (csrc/device/path_f64.h: the path's sin and cos of 2 pi u) of n host doubles in [0, 2 pi].
 * A null pointer or n < 0: RT_E_INVAL; then n == 0: RT_OK; then no visible HIP device: RT_E_NODEVICE. */
int rt_diag_sincos(int32_t device, int64_t n, const double* x, double* s, double* c);
#ifdef __cplusplus
}
#endif
#endif /* RT_DIAG_H */
