// Host-visible launchers of the HIP kernels (implemented in *.hip, called by the csrc/api units).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../device/scene_layout.h"

namespace rt {

struct RenderArgs {
    int32_t width, height, x0, y0, tw, th;
    int32_t n_samples;  // spp / 4 per subpixel
    int32_t mis;
    int32_t features;  // Cfg<F> bits: 1 mesh, 2 phong, 4 mis, 8 compact, 16 nearest-triangle meshes (BVH),
                       // 32 no mirror (specular) object (the query-pool kernel's Cfg; the others ignore it)
    int32_t mesh_nodes;  // octree nodes of the largest mesh (megakernel choice)
    int32_t row_step;    // tile row i = screen row y0 + i * row_step
    int32_t tail_cps;    // split tail: chunks per subpixel
    // split tail (megakernels): subpixels [n_whole, nsub) are handed out as chunks of 2^chunk_lg
    // samples; a chunk's lane stores each sample's radiance in tail_buf[sub - n_whole][sample][3]
    // (megakernel_common.h tail_store) and k_tail_sum adds them up in sample order afterwards (the same
    // sequential sum)
    int32_t n_whole, chunk_lg;
    // whole subpixels are handed out in runs of unit_subs consecutive subpixels per ticket (n_wunits
    // tickets): at low spp a ticket per subpixel makes the one global counter's atomics the bottleneck
    int32_t unit_subs, n_wunits;
    uint64_t seed;
    double cx[3], cy[3];  // camera frame (server.rs:330-331), computed on the host
    double inv_n;         // 1.0 / n_samples (server.rs:358)
    double* sub_out;      // optional [pix][4][3]
    uint8_t* rgb_out;     // [pix][3]
    unsigned long long* counters;  // optional [0] = path vertices
    const int32_t* cancel;         // optional device view of the host cancel flag (mapped memory)
    double* tail_buf;              // split-tail sample radiance (see n_whole)
    int32_t f32_brute;             // f32 mode: meshes of <= f32_brute triangles are tested without the BVH
    int32_t all_flat;              // every mesh is a flat octree (DevMesh::flat) and there are <= 2 of them
};

// The split tail the calling thread's last megakernel launch planned (plan_tail): subpixels split into
// chunks, the split the kernel family wanted before the scratch buffer capped it, samples per chunk.
// Thread-local: a render is planned and enqueued on its caller's thread (rt_debug_last_split, rt_diag.h).
struct TailPlan {
    long n_split = 0, want = 0, chunk = 0;
};
extern thread_local TailPlan t_tail_plan;
// Subpixels the analytic and flat-mesh megakernels split per resident lane, x2 (plan_tail's split_x2): one and a
// half per lane, two for frames of up to 4 subpixels per lane (an N = 8 rank share). The tail's chunks must outlast
// the last whole subpixels, and a subpixel can cost 1.35x the average (its paths' lengths): in a share of ~4
// subpixels per lane the last whole ones started at 2/3 of the launch and ended 6 ms after every other wave
// (profiles/r06h_end_probe_waves.log); in the full cornell frame with half a subpixel per lane split, the last
// waves ended 15 ms after the median one, each behind a whole subpixel taken 59 ms before its end
// (profiles/r06ah_end_probe_waves.log). Cornell N = 8 share: 1864.6 (0.5 per lane) -> 1903.4 (1.5,
// profiles/r06u_ab_tail.log) -> 1909.1 (2; 2.5: 1910.7, profiles/r06y_ab_tail_n8.log) Msamples/s; full frames at
// 0.5 -> 1.5 per lane: cornell 1988.3 -> 2003.8 (2: 2001.2, profiles/r06ai_ab_tail_full.log), cubes 1079.5 -> 1085.5,
// N = 2 shares cornell 1963.9 -> 1987.8 and cubes 1067.5 -> 1079.7 (profiles/r06aj_ab_tail_full.log).
// ensure_tail_scratch (api/render.cpp) sizes the split-tail scratch with the same rule.
inline int tail_split_x2(long nsub, long lanes) { return nsub <= 4 * lanes ? 4 : 3; }
// Split-tail scratch bytes per split subpixel (megakernel_common.h plan_tail: the samples after chunk 0).
size_t tail_scratch_per_subpixel(int n_samples);
// tail_buf / tail_cap: scratch for the split tail (bytes); the launcher sizes the tail to fit it.
hipError_t launch_megakernel_f64(const DevScene& sc, const RenderArgs& a, double* sub_buf, uint32_t* next_sub,
                                 double* tail_buf, size_t tail_cap, hipStream_t st);
// Query-pool kernel for flat-octree mesh scenes (render_flat_f64.hip); called by
// launch_megakernel_f64 after the ticket counter is reset.
hipError_t launch_megakernel_flat_f64(const DevScene& sc, const RenderArgs& a, double* sub_buf, uint32_t* next_sub,
                                      double* tail_buf, size_t tail_cap, int refill, hipStream_t st);
// Deep-octree mesh megakernel (render_mesh_f64.hip, walk pool); called by launch_megakernel_f64 after
// the ticket counter is reset; a: the caller's args (features, sizes), planned here.
hipError_t launch_megakernel_mesh_f64(const DevScene& sc, const RenderArgs& a, double* sub_buf, uint32_t* next_sub,
                                      long nsub, int refill, int wmin, double* tail_buf, size_t tail_cap, hipStream_t st);
// Diagnostic symbols of each kernel code object (diag_tu.h): read, add to the outputs, clear.
int diag_read_main(unsigned long long* cnt16, unsigned long long* reg32, unsigned long long* tim16, unsigned long long* q4);
int diag_read_mesh(unsigned long long* cnt16, unsigned long long* reg32, unsigned long long* tim16, unsigned long long* q4);
int diag_read_flat(unsigned long long* cnt16, unsigned long long* reg32, unsigned long long* tim16, unsigned long long* q4);
// f32 perf mode (render_f32.hip): writes the subpixel means to sub_buf like the f64 megakernel.
hipError_t launch_megakernel_f32(const DevScene& sc, const RenderArgs& a, double* sub_buf, uint32_t* next_sub,
                                 hipStream_t st);
hipError_t launch_finalize_f64(const RenderArgs& a, const double* sub_buf, hipStream_t st);
// What a launch's units are, for the fused body and the two pool bodies alike: nothing (kFrame: units are the tile's
// subpixels), a frame pixel per unit-group (kList), or a (pixel, pass) word per unit-group
// (kPasses): pixel | pass << kPassShift (integrator_f64.h), the pass indexing a table of 16 seeds.
constexpr int kFrame = 0, kList = 1, kPasses = 2;
struct UnitList {           // device pointers
    const uint32_t* words;  // n entries: unique pixel ids (list) or pixel | pass << 28 (passes); null: a frame
    long n;
    const uint64_t* seeds;  // 16 seeds: non-null makes it a passes list
    int kind() const { return seeds ? kPasses : words ? kList : kFrame; }
};
// The kernel families with list and passes instances (include/rt_ffi.h RT_LIST_*).
enum : int { kListFused = 1, kListFpool = 2, kListRoles = 3 };
// The pool kernel family launch_megakernel_f64 takes for these args that also has list instances, by its own
// predicates; kListFused: none (analytic scenes, Phong mesh scenes, octrees without slot tables, BVH walks).
inline int list_pool_family(const RenderArgs& a, bool slot_tables) {
    if (a.features & (2 | 16)) return kListFused;
    if (a.all_flat && (a.features & 9) == 9) return kListFpool;
    if ((a.features & 9) == 9 && a.mesh_nodes >= 64 && slot_tables) return kListRoles;
    return kListFused;
}
// Pixel-list render and batched passes (render_f64.hip): the subpixel means of unit-group u
// into sub_buf[u][4][3]: of the frame pixel units.words[u] with a.seed (kList), or of the frame pixel
// units.words[u] & (2^28 - 1) with the seed units.seeds[units.words[u] >> 28] (kPasses: width * height < 2^28,
// hipErrorInvalidValue otherwise); a.tw / th / x0 / y0 / row_step play no part. units.n * 4 <= INT32_MAX and
// non-null words (hipErrorInvalidValue otherwise). next_unit: the ticket counter (reset here).
// family kListFused runs k_render_list_f64 / k_render_passes_f64, the list and passes instances of the fused
// megakernel's body with its Cfg choice (a.features & 15); kListFpool / kListRoles run the list or passes instances of
// the frame's pool kernels (launch_render_units_flat_f64 / launch_render_units_roles_f64, called after the ticket
// counter is reset), which must be list_pool_family's answer for the scene (hipErrorInvalidValue otherwise);
// tail_buf / tail_cap: their split-tail scratch, as launch_megakernel_f64's.
hipError_t launch_render_units_f64(const DevScene& sc, const RenderArgs& a, const UnitList& units, double* sub_buf,
                                   uint32_t* next_unit, int family, double* tail_buf, size_t tail_cap, hipStream_t st);
hipError_t launch_render_units_flat_f64(const DevScene& sc, const RenderArgs& a, const UnitList& units, double* sub_buf,
                                        uint32_t* next_sub, double* tail_buf, size_t tail_cap, hipStream_t st);
hipError_t launch_render_units_roles_f64(const DevScene& sc, const RenderArgs& a, const UnitList& units, double* sub_buf,
                                         uint32_t* next_sub, double* tail_buf, size_t tail_cap, hipStream_t st);
hipError_t launch_trace_f64(const DevScene& sc, long n, const double* o, const double* d, double* t, int32_t* obj,
                            double* pos, double* nrm, bool mesh_nearest, hipStream_t st);

// Batch query diagnostics (include/rt_diag.h rt_diag_trace / rt_diag_visible, kernels/diag_queries.h): n queries,
// one lane each. a / b: the rays' origins and directions (trace: t, obj, prim, pos, nrm out) or the segments'
// endpoints x and y (visible: vis out); near_mask (device, may be null): the split forms' mesh_near_mask.
struct DiagArgs {
    long n;
    const double* a;
    const double* b;
    double* t;
    int32_t* obj;
    int32_t* prim;
    double* pos;
    double* nrm;
    uint8_t* vis;
    uint32_t* near_mask;
};
// Each launcher sits in the translation unit that owns the query code it runs; visible: the segment query
// instead of the ray query.
// render_f64.hip: trace_closest<C> / visible<C> with k_trace_f64's Cfg choice (guards 0), the mesh-free compact
// instance of k_megakernel_f64<8, 4> (1: the round-7 guards), or the compact mesh instances of
// k_megakernel_f64<odd, 3> (2: the one-ballot guards, kCfgGuards1)
hipError_t launch_diag_fused(const DevScene& sc, const DiagArgs& a, bool visible, int guards, bool mesh_nearest,
                             hipStream_t st);
// render_mesh_f64.hip: the roles / walk pools' split (analytic part, mesh_near_mask, slot walks of the near meshes)
hipError_t launch_diag_slots(const DevScene& sc, const DiagArgs& a, bool visible, hipStream_t st);
// wavefront_f64.hip: the wavefront's split (analytic part, mesh_candidate, node_kids walks)
hipError_t launch_diag_kids(const DevScene& sc, const DiagArgs& a, bool visible, hipStream_t st);
// render_flat_f64.hip: the flat query pool's split (analytic part, near mask, flat_query per near mesh)
hipError_t launch_diag_flat(const DevScene& sc, const DiagArgs& a, bool visible, hipStream_t st);


// Batch vertex diagnostics (include/rt_diag.h rt_diag_vertex, kernels/diag_queries.h): n path vertices, one lane
// each, as packed rows (device pointers): st[n][19] = ray origin, ray direction, beta, L, bemit, o, pdf_prev;
// rng[n][2] the stream's state; dk[n][2] = depth, kind; the *_out rows: the state the lane carries on, bemit and o
// as the form's Cold returns them; info[n][4] = hit object, continue flag, and for the deferred forms
// ShadowDefer::pending and ::meshes.
struct DiagVertexArgs {
    long n;
    const double* st;
    const uint64_t* rng;
    const int32_t* dk;
    double* st_out;
    uint64_t* rng_out;
    int32_t* dk_out;
    int32_t* info;
};
// render_f64.hip: trace_closest<C> and shade_vertex<C> (no deferral) for a compact scene with a.features' Phong and
// MIS bits. guards 0: k_trace_f64's C (mesh code compiled in, RegCold); 1: the even-F mesh-free instance; 2: the
// kCfgGuards1 mesh instances; 3: fused_body's own C (the object table in LDS, the one-ballot guards for a mesh
// scene) with LdsCold on a [6][256] column per thread, as fused_body calls it. mesh_nearest: the BVH walks.
hipError_t launch_diag_vertex_fused(const DevScene& sc, const RenderArgs& a, const DiagVertexArgs& v, int guards,
                                    bool mesh_nearest, hipStream_t st);
// The deferred-shadow forms: the form's split trace, shade_vertex with a ShadowDefer as the form's render kernel
// calls it for a.features (hipErrorInvalidValue for features the kernel family has no instance of), then the
// pending shadow query resolved as the family resolves it, defer.c added iff no mesh occludes.
// render_mesh_f64.hip: the slot-walk pools (needs DevScene::node_slot). sink = false: the walk pool's call, the
// shadow ray returned in the ShadowDefer; sink = true: the roles pool's, LdsQuerySink into LDS columns
hipError_t launch_diag_vertex_slots(const DevScene& sc, const RenderArgs& a, const DiagVertexArgs& v, bool sink,
                                    hipStream_t st);
// wavefront_f64.hip: k_wf_shade's instantiation, node_kids walks
hipError_t launch_diag_vertex_kids(const DevScene& sc, const RenderArgs& a, const DiagVertexArgs& v, hipStream_t st);
// render_flat_f64.hip: the query pool's instantiation (its nospec bit, LdsCold, LdsQuerySink), flat_query
hipError_t launch_diag_vertex_flat(const DevScene& sc, const RenderArgs& a, const DiagVertexArgs& v, hipStream_t st);
// render_f64.hip: sincos_2pi (path_f64.h) of n doubles (device pointers).
hipError_t launch_diag_sincos(long n, const double* x, double* s, double* c, hipStream_t st);

}  // namespace rt
