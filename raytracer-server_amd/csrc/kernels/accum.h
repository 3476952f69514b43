// Progressive accumulation: launchers of accum.hip, called by the api units (rt_accum_*).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {

// S += n m, Q += (n m) m over the npix * 12 subpixel means of one pass (first: store without reading S and Q).
// S, Q and m are 16-byte aligned.
hipError_t launch_accum_add(double* S, double* Q, const double* m, long npix, int32_t n, bool first, hipStream_t st);
// sub[pix][4][3] = S / N (nullable) and var[pix][4] f32 (nullable; K >= 2): the delta-method variance of the clamped
// pixel colour (rt_ffi.h rt_accum_resolve).
hipError_t launch_accum_resolve(const double* S, const double* Q, long npix, int64_t N, int64_t K, double* sub,
                                float* var, hipStream_t st);

// Per-pixel counts and sparse merges. cnt[pix][2] = (K_p, N_p): the passes and samples per subpixel
// merged into pixel p.
// cnt[p] = (K, N) for every pixel (add false), or cnt[p] += (K, N) (add true: a full-frame merge of K passes).
hipError_t launch_accum_cnt_fill(uint32_t* cnt, long npix, uint32_t K, uint32_t N, bool add, hipStream_t st);
// The pass m[e][4][3] of the n_list unique pixels list[e] (ids < npix): S[p] += n m, Q[p] += (n m) m with
// launch_accum_add's expression, cnt[p] += (1, n). m 16-byte aligned.
hipError_t launch_accum_add_list(double* S, double* Q, uint32_t* cnt, const uint32_t* list, long n_list, const double* m,
                                 int32_t n, hipStream_t st);
// launch_accum_resolve with N_p and K_p - 1 of cnt (every K_p >= 2 when var is wanted).
hipError_t launch_accum_resolve_cnt(const double* S, const double* Q, const uint32_t* cnt, long npix, double* sub,
                                    float* var, hipStream_t st);
// Selection (rt_ffi.h rt_accum_select): the ids of the active pixels, ascending, by a two-pass compaction. var: the
// resolve's float[pix][4]; cnt: per-pixel counts or null (then every N_p = N); scratch: select_scratch_bytes(npix)
// bytes, 8-byte aligned. At most cap ids go to out; *total (device) is the full count.
size_t select_scratch_bytes(long npix);
hipError_t launch_accum_select(const double* S, const float* var, const uint32_t* cnt, int64_t N, int width, int height,
                               float abs_tol, float rel_tol, int32_t max_n, void* scratch, uint32_t* out, long cap,
                               uint32_t* total, hipStream_t st);
// The hole list of a seeded accumulator (rt_ffi.h rt_accum_holes): the ids of the pixels with
// K_p < 2, and, with period > 0, of those with (col + 3 row) mod period == phase, ascending, by the selection's
// compaction. cnt: the per-pixel counts; scratch: select_scratch_bytes(npix) bytes, 8-byte aligned. At most cap ids go
// to out; *total (device) is the full count, *n_holes (device, 8-byte aligned) the pixels with K_p < 2.
hipError_t launch_accum_holes(const uint32_t* cnt, int width, int height, int32_t period, int32_t phase, void* scratch,
                              uint32_t* out, long cap, uint32_t* total, unsigned long long* n_holes, hipStream_t st);

// Batched passes (rt_ffi.h rt_accum_plan). The most passes one entry may hold: the pass index rides in
// the top 4 bits of a unit word (integrator_f64.h kPassShift).
constexpr int kPassesMax = 16;
// The plan's first two passes: the selection's ballots and scanned block offsets in `scratch` (as launch_accum_select
// leaves them), want[pix] = the pass count each active pixel wants before the frame cap (0: inactive),
// hist[kPassesMax + 1] = how many pixels want each count, *total = the list's length (all device).
hipError_t launch_accum_plan_count(const double* S, const float* var, const uint32_t* cnt, int64_t N, int width,
                                   int height, float abs_tol, float rel_tol, int32_t max_n, int32_t n, float gain,
                                   int32_t max_passes, void* scratch, uint8_t* want, uint32_t* hist, uint32_t* total,
                                   hipStream_t st);
// The plan's last pass: out[at] = the id and counts[at] = min(want, cmax) of the active pixels, ascending, at most cap.
hipError_t launch_accum_plan_write(const void* scratch, const uint8_t* want, long npix, int32_t cmax, uint32_t* out,
                                   uint8_t* counts, long cap, hipStream_t st);
// A list with counts -> off[e] (nullable), the exclusive prefix sum of counts, and units[off[e] + i] =
// list[e] | i << 28 (at most cap words); *total = the unit count. scratch: runs_scratch_bytes(n) bytes.
size_t runs_scratch_bytes(long n);
hipError_t launch_accum_expand(const uint32_t* list, const uint8_t* counts, long n, void* scratch, uint32_t* off,
                               uint32_t* units, long cap, uint32_t* total, hipStream_t st);
// The run merge: entry e's counts[e] units m[off[e] + i][4][3], in pass order, into pixel list[e] with
// launch_accum_add_list's expression; cnt[p] += (counts[e], counts[e] n).
hipError_t launch_accum_add_runs(double* S, double* Q, uint32_t* cnt, const uint32_t* list, const uint8_t* counts,
                                 const uint32_t* off, long n_list, const double* m, int32_t n, hipStream_t st);

}  // namespace rt
