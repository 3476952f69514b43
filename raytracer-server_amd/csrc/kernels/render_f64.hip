// f64 render kernels for gfx950 (CDNA4).
//
//   k_megakernel_f64  — fused, persistent path loop (below); k_finalize_f64 — subpixel means -> RGB8.
//   k_render_list_f64 — the same loop over a list of frame pixels: analytic scenes, and mesh scenes
//                       whose frame kernel has no list instance (Phong mesh scenes, octrees without slot tables) or
//                       whose list is short; launch_render_units_f64 hands the other mesh scenes' lists to the list
//                       instances of the frame's own pool kernels, which give the same bits.
//   k_render_passes_f64 — the same loop over a list of (pixel, pass) units with a seed per pass;
//                       launch_render_units_f64 hands the scenes with pool list instances to the pools' passes
//                       instances.
//   k_trace_f64       — Scene::trace_ray for a batch of rays (parity tests of the intersectors).
//   wavefront kernels — see wavefront_f64.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../device/integrator_f64.h"
#include "kernels.h"
#include "megakernel_common.h"
#include "diag_queries.h"

namespace rt {
using namespace f64;

// Persistent megakernel: a resident grid whose lanes pull subpixels from a global counter. A lane
// walks the spp/4 sample paths of its subpixel vertex by vertex; when a path ends, the next sample
// starts in the same iteration (regeneration); when the subpixel is done its mean goes to
// sub_buf (sequential sum in sample order, server.rs:338-358) and the lane takes the next
// subpixel. Waves idle only in the frame's final tail, not per wave.
// W = minimum waves per SIMD requested from the register allocator.
#ifndef RT_CAM_DEPTH
#define RT_CAM_DEPTH 1  // camera samples buffered ahead per lane (k_megakernel_f64; 2 measured 1% slower)
#endif
constexpr int kCamDepth = RT_CAM_DEPTH;
typedef __attribute__((address_space(3))) double LdsDouble;
typedef __attribute__((address_space(3))) int32_t LdsInt;
typedef __attribute__((address_space(3))) uint64_t LdsU64;

#ifndef RT_MK_MIN_RUN
#define RT_MK_MIN_RUN 32  // samples per ticket at least, while the frame holds more than one run per lane (plan_units;
#endif                     // 1080p at 64 spp: 16 -> 1567.5, 24 / 32 -> 1804-1808, 64 -> 1744.9, 128 -> 1664.9 Msamples/s,
                           // profiles/r06br_ab_min_run_long.log, r06bs_ab_min_run_short.log)

// Diagnostic builds (RT_DEBUG_TIMERS): each wave of k_megakernel_f64 records, on the constant 100 MHz clock
// (s_memrealtime), when it started, when fewer than half of its lanes last held work (-1: never), and when it
// ended (rt_debug_wave_times, tools/end_probe.py --waves): the end phase of a launch, wave by wave.
// Both instance kinds of the body write them: after a k_render_list_f64 launch the records are that launch's.
#if RT_DEBUG_TIMERS
constexpr int kDbgWaves = 8192;
constexpr int kDbgWaveRec = 5;
__device__ unsigned long long g_dbg_wave[kDbgWaveRec * kDbgWaves];
#endif

// The loop's body, shared by its frame instances (L = false: k_megakernel_f64, units are the tile's subpixels) and
// its pixel-list instances (L = true: k_render_list_f64, unit 4 e + j is subpixel j of the frame pixel pixels[e];
// DESIGN.md §13). Everything but the camera sample's SubPixel works on the compact unit id; a list launch plans no
// split tail (nsub == a.n_whole).
// L adds a register with the pixel id of the unit in hand, pix = pixels[id >> 2], loaded where a lane's id enters a
// list entry (load_pix: a new ticket, or a run crossing to (id & 3) == 0), and makes "this unit is whole" a
// compile-time fact at its two uses, so a list instance holds no tail code. Both answer measurements against the
// former copy of this loop (profiles/fused_list_fold_*.log): with pixels[] read at every camera sample
// (unit_subpixel<L>, as the pool kernels do) and the tail tests left to run, the full lists ran 0.6% (cornell) and
// 1.7% (cubes) slower; with the register alone 0.9% and 0.4%. Every read is made by an active lane: it holds a
// ticket < nunits, so its id < n_whole = 4 n_pixels. (unit_of also runs for a lane whose ticket is past the end, or
// -1 after a stop: that id is out of range, but the lane is inactive from then on and load_pix(active) reads nothing.)
// L = kPasses (k_render_passes_f64): the list holds one word per unit-group, a (pixel, pass) pair packed
// as pixel | pass << kPassShift; units[id >> 2] is loaded exactly where a list instance loads pixels[id >> 2], and
// the camera sample draws from seeds[pass] (16 u64 on the device) instead of a.seed. The camera ring only reads ahead
// within one unit, so the seed is a per-unit fact as the pixel is; nothing else in the loop knows about passes. The
// pass rides in the top 4 bits of the pixel's register (frames of width * height < 2^28: the host checks), so the
// instance needs no register beyond the list's; the seed is an 8-byte load beside the camera sample's arithmetic.
// (kFrame / kList / kPasses, kPassShift and kPassPixMask: integrator_f64.h, shared with the pool bodies)
template <int F, int L>
__device__ __forceinline__ void fused_body(double* __restrict__ sub_buf, uint32_t* next_sub, long nsub, int refill,
                                           const uint32_t* __restrict__ pixels,
                                           const uint64_t* __restrict__ seeds = nullptr) {
    // Compact scenes (<= kMaxCompactObjects objects): the object table is copied into LDS, so the
    // shading's per-lane object reads (hit object, light) are ds_reads instead of global loads.
    // the fused mesh instances (F odd) keep the one-ballot guards (path_f64.h kCfgGuards1: they sit at their
    // register cap, and the new guards raised their spill counts)
    // and, with the Phong + MIS mesh-free instance F = 14 (its pixel-list and batched-pass kernels), read the
    // compact tables at each use (kCfgTabUse: the batch windows raised their spill counts)
    using C = Cfg<F | ((F & 8) ? kCfgLdsObj : 0) | ((F & 1) ? kCfgGuards1 | kCfgTabUse : 0) |
                  (F == 14 ? kCfgTabUse : 0)>;
    const DevScene& sc = karg_scene();  // the kernel's first two arguments, read in place (megakernel_common.h)
    const RenderArgs& a = karg_render_args();
    if constexpr (C::ldsobj) lds_objects_fill(sc);
    // Rarely touched per-lane state lives in LDS (one column per thread; VGPRs are the limit at 4
    // waves/SIMD): the subpixel accumulator (once per sample) and the camera-sample buffer — a ring
    // of kCamDepth next samples (camera ray + RNG state) per lane, computed ahead in passes the whole
    // wave runs once >= refill lanes have a free slot (begin_sample for the ~7% of lanes whose path
    // ended each iteration otherwise runs every iteration at that lane utilisation).
    __shared__ double s_acc[3 * 256], s_nbd[kCamDepth * 3 * 256];
    __shared__ uint64_t s_nbr[kCamDepth * 2 * 256];
    __shared__ double s_cold[6 * 256];  // integrator_f64.h LdsCold: o and the pre-bounce throughput of mirror paths
    const LdsCold cold{(LdsDouble*)s_cold + threadIdx.x};
    LdsDouble* acc_l = (LdsDouble*)s_acc + threadIdx.x;  // component k at [k * 256]
    LdsDouble* nbd = (LdsDouble*)s_nbd + threadIdx.x;     // slot q, component k at [(q * 3 + k) * 256]
    LdsU64* nbr = (LdsU64*)s_nbr + threadIdx.x;           // slot q, word k at [(q * 2 + k) * 256]
    RT_DBG_TINIT();
    uint32_t nverts = 0;
    // tickets: whole subpixels, then the split tail's chunks (unit_of)
    const long n_split = nsub - a.n_whole;
    const long nunits = a.n_wunits + n_split * a.tail_cps;
    int id, s;  // subpixel (tile-local, < 2^31: api/common.cpp check_params) and sample of the unit in hand
    const long t0 = wave_ticket(next_sub, true);
    {
        int end_unused;  // the run's end is recomputed when needed (run_end)
        unit_of(a, t0, id, end_unused, s);
    }
    bool active = t0 < nunits;
    [[maybe_unused]] uint32_t pix = 0;
    const auto load_pix = [&](bool want) {
        if constexpr (L) {
            if (want) pix = pixels[id >> 2];
        }
    };
    load_pix(active);
    acc_l[0] = 0.0; acc_l[256] = 0.0; acc_l[512] = 0.0;
    PathState ps;
    bool fresh = true;
    int nbuf = 0, hb = 0;  // buffered camera samples (s + 1 .. s + nbuf) and the ring's head slot
#if RT_DEBUG_TIMERS
    const unsigned long long w_t0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long w_half = ~0ull;
    // per lane: when it took the unit it holds (l_take, l_unit) and when it ran out of work (l_end)
    unsigned long long l_take = w_t0, l_end = w_t0;
    long l_unit = t0;
#endif
    while (__any(active)) {
#if RT_DEBUG_TIMERS
        if (w_half == ~0ull && __popcll(__ballot(active)) < 32) w_half = __builtin_amdgcn_s_memrealtime();
#endif
        RT_DBG_REGION(0);
        RT_DBG_TSTART(t_it);
        bool done = false;
        // (timer 1 of the diagnostic build: the block in which a lane took its next buffered sample at the top of
        // the iteration; it now does so where the last sample ended, below, and the timer reads its own overhead)
        RT_DBG_TSTART(t_fr);
        RT_DBG_TEND(1, t_fr);
        RT_DBG_TSTART(t_rf);
        // camera pass: lanes that start a path now without a buffered sample (sample s), plus lanes
        // with a free ring slot whose next sample (s + nbuf + 1) is in the same unit; run when any
        // lane needs a sample now or >= refill lanes have a free slot
        {
            const bool now = active && fresh;
            const bool need = active && !fresh && nbuf < kCamDepth &&
                              (L ? s + nbuf + 1 < a.n_samples : unit_has(a, id, s, s + nbuf + 1));
            if (__any(now) || (refill > 0 && __popcll(__ballot(need)) >= refill)) {
                if (now || (refill > 0 && need)) {
                    RT_DBG_REGION(3);
                    SubPixel sp;
                    if constexpr (L == kPasses) sp = subpixel_of_pixel(a, pix & kPassPixMask, id);
                    else if constexpr (L) sp = subpixel_of_pixel(a, pix, id);
                    else sp = subpixel_of(a, id);
                    CameraSample nb;
                    if constexpr (L == kPasses)
                        nb = camera_sample_seeded<C::g1>(sc, a, sp, now ? s : s + nbuf + 1, seeds[pix >> kPassShift]);
                    else nb = camera_sample<C::g1>(sc, a, sp, now ? s : s + nbuf + 1);
                    if (now) {
                        begin_path(sc, nb, ps);
                        fresh = false;
                    } else {
                        int slot = hb + nbuf;
                        slot = slot >= kCamDepth ? slot - kCamDepth : slot;
                        const int q = slot * 3 * 256, r = slot * 2 * 256;
                        nbd[q] = nb.d.x; nbd[q + 256] = nb.d.y; nbd[q + 512] = nb.d.z;
                        nbr[r] = nb.r0; nbr[r + 256] = nb.r1;
                        ++nbuf;
                    }
                }
            }
        }
        RT_DBG_TEND(4, t_rf);
        if (active) {
            RT_DBG_REGION(1);
            RT_DBG_TSTART(t_tr);
            HitRec hr = trace_closest<C>(sc, ps.ray);
            RT_DBG_TEND(2, t_tr);
            nverts += hr.obj >= 0;
            RT_DBG_TSTART(t_sh);
            fresh = !shade_vertex<C>(sc, a, ps, hr, nullptr, cold);
            RT_DBG_TEND(3, t_sh);
            RT_DBG_TSTART(t_se);
            if (fresh) {
                RT_DBG_REGION(4);
                if (L || id < a.n_whole) {  // (a list's units are all whole: its instances hold no tail code)
                    V3 acc = v3(acc_l[0], acc_l[256], acc_l[512]);
                    acc = acc + ps.L * a.inv_n;  // server.rs:357-358
                    acc_l[0] = acc.x; acc_l[256] = acc.y; acc_l[512] = acc.z;
                    if (++s == a.n_samples) {
                        double* o = sub_buf + (size_t)id * 3;
                        o[0] = acc.x;
                        o[1] = acc.y;
                        o[2] = acc.z;
                        if (id + 1 < run_end(a, id)) {  // the next subpixel of the run, no ticket
                            ++id;
                            load_pix((id & 3) == 0);
                            s = 0;
                            acc_l[0] = 0.0; acc_l[256] = 0.0; acc_l[512] = 0.0;
                            nbuf = 0;
                            hb = 0;
                        } else {
                            done = true;
                        }
                    }
                } else if (tail_in_place(a, s)) {  // split tail, chunk 0: summed in place, its partial sum to sub_buf
                    V3 acc = v3(acc_l[0], acc_l[256], acc_l[2 * 256]);
                    acc = acc + ps.L * a.inv_n;  // server.rs:357-358
                    acc_l[0] = acc.x; acc_l[256] = acc.y; acc_l[2 * 256] = acc.z;
                    done = !unit_has_next(a, id, s);
                    if (done) {
                        double* o = sub_buf + (size_t)id * 3;
                        o[0] = acc.x;
                        o[1] = acc.y;
                        o[2] = acc.z;
                    }
                    ++s;
                } else {  // split tail, later chunks: each sample's radiance, summed in order by k_tail_sum_f64
                    tail_store(a, id, s, ps.L);
                    done = !unit_has_next(a, id, s);
                    ++s;
                }
                // the next sample of the same unit from the camera buffer, here rather than in a block of its own
                // at the top of the next iteration (same lanes; the camera pass below sees the same ring state:
                // cornell 1024 spp 2000.6 -> 2002.9, C2 MIS 1891.0 -> 1896.6, profiles/r06be_ab_begin_at_end.log)
                if (!done && nbuf > 0) {
                    const int q = hb * 3 * 256, r = hb * 2 * 256;
                    begin_path(sc, CameraSample{v3(nbd[q], nbd[q + 256], nbd[q + 512]), nbr[r], nbr[r + 256]}, ps);
                    fresh = false;
                    hb = hb + 1 == kCamDepth ? 0 : hb + 1;
                    --nbuf;
                }
            }
            RT_DBG_TEND(6, t_se);
        }
        RT_DBG_TSTART(t_bk);
        // cancellation (RenderJob::stop, server.rs:201-203): checked when a lane would start a new
        // subpixel; a set flag stops handing out work, lanes finish the subpixel they hold
        bool stop = false;
        if (a.cancel && __any(done)) stop = __hip_atomic_load(a.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
        const long nt = wave_ticket(next_sub, done && !stop);
        flush_count_if_full(a.counters, nverts, done);
#if RT_DEBUG_TIMERS
        if (done) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (nt < nunits) {
                l_take = now;
                l_unit = nt;
            } else {
                l_end = now;
            }
        }
#endif
        if (done) {
            int end_unused;
            unit_of(a, nt, id, end_unused, s);
            active = !stop && nt < nunits;
            load_pix(active);
            acc_l[0] = 0.0; acc_l[256] = 0.0; acc_l[512] = 0.0;
            fresh = true;
            nbuf = 0;
            hb = 0;
        }
        RT_DBG_TEND(5, t_bk);
        RT_DBG_TEND(0, t_it);
    }
    flush_count(a.counters, nverts);
#if RT_DEBUG_TIMERS
    {
        const unsigned long long w_t1 = __builtin_amdgcn_s_memrealtime();
        const unsigned wid = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        // the lane that ran out of work last: when it took its last unit, and which
        unsigned long long e = l_end, tk = l_take;
        long u = l_unit;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long e2 = __shfl_xor(e, off, 64), tk2 = __shfl_xor(tk, off, 64);
            const long u2 = __shfl_xor(u, off, 64);
            const bool take2 = e2 > e || (e2 == e && u2 > u);
            e = take2 ? e2 : e;
            tk = take2 ? tk2 : tk;
            u = take2 ? u2 : u;
        }
        if ((threadIdx.x & 63) == 0 && wid < (unsigned)kDbgWaves) {
            unsigned long long* r = g_dbg_wave + kDbgWaveRec * wid;
            r[0] = w_t0;
            r[1] = w_half;
            r[2] = w_t1;
            r[3] = tk;
            r[4] = (unsigned long long)u;
        }
    }
#endif
    RT_DBG_TFLUSH();
}

template <int F, int W>
__global__ __launch_bounds__(256, W) void k_megakernel_f64(DevScene sc_g, RenderArgs a_g, double* __restrict__ sub_buf,
                                                          uint32_t* next_sub, long nsub, int refill) {
    fused_body<F, kFrame>(sub_buf, next_sub, nsub, refill, nullptr);
}
// The pixel-list instance: nsub = 4 n_pixels units, sub_buf the compact [n_pixels][4][3] buffer.
template <int F, int W>
__global__ __launch_bounds__(256, W) void k_render_list_f64(DevScene sc_g, RenderArgs a_g, double* __restrict__ sub_buf,
                                                           uint32_t* next_sub, long nsub, int refill,
                                                           const uint32_t* __restrict__ pixels) {
    fused_body<F, kList>(sub_buf, next_sub, nsub, refill, pixels);
}
// The batched-passes instance: nsub = 4 n_units units, units[u] = pixel | pass << 28 (pass < 16),
// seeds[16] on the device, sub_buf the compact [n_units][4][3] buffer. Scheduling is the list instance's.
template <int F, int W>
__global__ __launch_bounds__(256, W) void k_render_passes_f64(DevScene sc_g, RenderArgs a_g, double* __restrict__ sub_buf,
                                                             uint32_t* next_sub, long nsub, int refill,
                                                             const uint32_t* __restrict__ units,
                                                             const uint64_t* __restrict__ seeds) {
    fused_body<F, kPasses>(sub_buf, next_sub, nsub, refill, units, seeds);
}

// Split tail: subpixel n_whole + j's mean, continuing the sequential sum chunk 0 left in sub_buf (its lane
// summed samples [0, c0) in place, megakernel_common.h tail_in_place) over the later chunks' stored sample
// radiance, in sample order, with the same acc + L * inv_n expression as the megakernel's accumulator
// (server.rs:357-358): the bits of one lane summing every sample. A thread per subpixel; tail_buf is
// subpixel-major (tail_store), so the block stages kTailStage samples of its 256 subpixels through LDS: the
// staging loads read each subpixel's 192-byte run with 16-byte lanes side by side (a thread reading its own run
// put every lane of a load on a line of its own: 2.8 GB in 1.0 ms at N = 8,
// profiles/r06af_ktrace_share8_kernel_stats.csv; staged: 0.68 ms, profiles/r06ap_ktrace_share8_kernel_stats.csv,
// the frame's kernel unchanged; a layout with contiguous reads, 0.46 ms, cost the megakernel's stores more, tail_store). LDS rows of kTailRow doubles (an odd count: the threads' 8-byte
// reads spread over the banks).
constexpr int kTailStage = 8, kTailRow = kTailStage * 3 + 1;
__global__ __launch_bounds__(256) void k_tail_sum_f64(RenderArgs a, double* __restrict__ sub_buf, long n_split) {
    __shared__ double stage[256 * kTailRow];
    const int c0 = 1 << a.chunk_lg;
    const int ns = a.n_samples - c0;
    const size_t run = (size_t)ns * 3;  // doubles per subpixel in tail_buf
    for (long base = (long)blockIdx.x * 256; base < n_split; base += (long)gridDim.x * 256) {
        const long j = base + threadIdx.x;
        const int nj = (int)min(256L, n_split - base);  // this block's subpixels
        double* o = sub_buf + (size_t)(a.n_whole + j) * 3;
        V3 acc = j < n_split ? v3(o[0], o[1], o[2]) : v3(0, 0, 0);
        const double* src = a.tail_buf + (size_t)base * run;
        for (int s0 = 0; s0 < ns; s0 += kTailStage) {
            const int nb = min(kTailStage, ns - s0);
            __syncthreads();  // the previous stage's reads are done
            if (nb == kTailStage && (run & 1) == 0) {
                // 12 16-byte pieces per subpixel (runs and stages start 16-byte aligned: run and s0 * 3 even),
                // 12 per thread: all loads issued before the LDS writes (one round trip per stage)
                double2 v[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    const int e = threadIdx.x + 256 * i, q = e / 12, k = e - q * 12;
                    if (q < nj) v[i] = *(const double2*)(src + (size_t)q * run + (size_t)s0 * 3 + 2 * k);
                }
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    const int e = threadIdx.x + 256 * i, q = e / 12, k = e - q * 12;
                    if (q < nj) {
                        stage[q * kTailRow + 2 * k] = v[i].x;
                        stage[q * kTailRow + 2 * k + 1] = v[i].y;
                    }
                }
            } else {
                const int per = nb * 3;
                for (int e = threadIdx.x; e < nj * per; e += 256) {
                    const int q = e / per, k = e - q * per;
                    stage[q * kTailRow + k] = src[(size_t)q * run + (size_t)s0 * 3 + k];
                }
            }
            __syncthreads();
            if (j < n_split) {
                const double* r = stage + threadIdx.x * kTailRow;
                for (int k = 0; k < nb; ++k) acc = acc + v3(r[3 * k], r[3 * k + 1], r[3 * k + 2]) * a.inv_n;
            }
        }
        if (j < n_split) {
            o[0] = acc.x;
            o[1] = acc.y;
            o[2] = acc.z;
        }
    }
}

// 4 subpixel means -> RGB8 (server.rs:360 clamp-then-average, :366-368 gamma, :187-189 `as u8`).
__global__ __launch_bounds__(256) void k_finalize_f64(RenderArgs a, const double* __restrict__ sub_buf) {
    const long npix = (long)a.tw * a.th;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += stride) {
        const double* s = sub_buf + (size_t)p * 12;
        V3 pixel = v3(0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) pixel = pixel + clampv(v3(s[3 * j], s[3 * j + 1], s[3 * j + 2]), 0., 1.) * 0.25;
        V3 c = clampv(pixel, 0., 1.);
        const double g = 1.0 / 2.2;
        V3 gc = v3(pow(c.x, g), pow(c.y, g), pow(c.z, g)) * 255.0 + v3(0.5, 0.5, 0.5);
        a.rgb_out[p * 3 + 0] = as_u8(gc.x);
        a.rgb_out[p * 3 + 1] = as_u8(gc.y);
        a.rgb_out[p * 3 + 2] = as_u8(gc.z);
    }
}

__global__ __launch_bounds__(256) void k_trace_f64(DevScene sc, long n, const double* __restrict__ o,
                                                   const double* __restrict__ d, double* t, int32_t* obj,
                                                   double* pos, double* nrm, int nearest) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r{v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), v3(d[3 * i], d[3 * i + 1], d[3 * i + 2])};
    HitRec h = nearest ? (sc.compact ? trace_closest<Cfg<25>>(sc, r) : trace_closest<Cfg<17>>(sc, r))
                       : (sc.compact ? trace_closest<Cfg<9>>(sc, r) : trace_closest<Cfg<1>>(sc, r));
    obj[i] = h.obj;
    t[i] = h.obj >= 0 ? h.t : 0.0;
    if (h.obj >= 0) {
        V3 p, nn;
        surface<Cfg<1>>(sc, r, h, &p, &nn);
        pos[3 * i] = p.x; pos[3 * i + 1] = p.y; pos[3 * i + 2] = p.z;
        nrm[3 * i] = nn.x; nrm[3 * i + 1] = nn.y; nrm[3 * i + 2] = nn.z;
    }
}

// rt_diag_trace / rt_diag_visible, the fused forms: trace_closest<C> / visible<C> per lane, C as k_trace_f64
// chooses it (cfg 0..3: compact | nearest << 1), cfg 4: the mesh-free compact instance the analytic
// megakernel k_megakernel_f64<8, 4> runs (even F: the round-7 guards, no mesh code compiled in), or cfg 5 / 6:
// the compact mesh instances with the one-ballot guards (kCfgGuards1) that k_megakernel_f64<odd, 3> keeps.
template <class C>
RT_DEV void diag_fused_query(const DevScene& sc, const DiagArgs& a, long i, int vis) {
    if (vis) {
        const V3 x = v3(a.a[3 * i], a.a[3 * i + 1], a.a[3 * i + 2]), y = v3(a.b[3 * i], a.b[3 * i + 1], a.b[3 * i + 2]);
        diag_store_vis(a, i, visible<C>(sc, x, y), 0u);
    } else {
        const Ray r = diag_ray(a, i);
        diag_store_hit(sc, a, i, r, trace_closest<C>(sc, r), 0u);
    }
}
template <int F>
__global__ __launch_bounds__(256) void k_diag_fused(DevScene sc, DiagArgs a, int vis) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    diag_fused_query<Cfg<F>>(sc, a, i, vis);
}
hipError_t launch_diag_fused(const DevScene& sc, const DiagArgs& a, bool visible, int guards, bool mesh_nearest,
                             hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    const int cfg = guards == 1 ? 4 : guards == 2 ? (mesh_nearest ? 6 : 5) : (sc.compact ? 1 : 0) | (mesh_nearest ? 2 : 0);
    const dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
    const int vis = visible ? 1 : 0;
    switch (cfg) {  // one kernel per instance: each holds one copy of the walks
        case 0: hipLaunchKernelGGL(k_diag_fused<1>, grid, block, 0, st, sc, a, vis); break;
        case 1: hipLaunchKernelGGL(k_diag_fused<9>, grid, block, 0, st, sc, a, vis); break;
        case 2: hipLaunchKernelGGL(k_diag_fused<17>, grid, block, 0, st, sc, a, vis); break;
        case 3: hipLaunchKernelGGL(k_diag_fused<25>, grid, block, 0, st, sc, a, vis); break;
        case 4: hipLaunchKernelGGL(k_diag_fused<8>, grid, block, 0, st, sc, a, vis); break;
        case 5: hipLaunchKernelGGL((k_diag_fused<9 | kCfgGuards1 | kCfgTabUse>), grid, block, 0, st, sc, a, vis); break;
        default: hipLaunchKernelGGL((k_diag_fused<25 | kCfgGuards1 | kCfgTabUse>), grid, block, 0, st, sc, a, vis); break;
    }
    return hipGetLastError();
}

// rt_diag_vertex, the fused forms: one path vertex per lane, trace_closest<C> then shade_vertex<C> with no
// deferral (the shadow ray inline), as fused_body's iteration runs them. Cold = RegCold: bemit and o in the
// PathState; Cold = LdsCold: fused_body's own instantiation, on a [6][256] LDS column per thread (the row's bemit
// and o are written there first, and read back from there afterwards). C::ldsobj instances fill the LDS object
// table first, every thread of the block taking part.
template <int F, bool kLdsCold>
__global__ __launch_bounds__(256) void k_diag_vertex_fused(DevScene sc, RenderArgs a, DiagVertexArgs v) {
    using C = Cfg<F>;
    if constexpr (C::ldsobj) lds_objects_fill(sc);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n) return;
    PathState ps = diag_vertex_load(v, i);
    const HitRec hr = trace_closest<C>(sc, ps.ray);
    if constexpr (kLdsCold) {
        __shared__ double s_cold[6 * 256];
        const LdsCold cold{(LdsDouble*)s_cold + threadIdx.x};
        cold.set_o(ps, ps.o);
        cold.set_bemit(ps, ps.bemit);
        const bool cont = shade_vertex<C>(sc, a, ps, hr, nullptr, cold);
        diag_vertex_store(v, i, ps, cold.bemit(ps), cold.o(ps), hr.obj, cont, false, 0u);
    } else {
        const bool cont = shade_vertex<C>(sc, a, ps, hr);
        diag_vertex_store(v, i, ps, ps.bemit, ps.o, hr.obj, cont, false, 0u);
    }
}
// The instance for a compact scene: Phong and MIS from a.features, as the render launchers take them
// (launch_mk_features, launch_megakernel_f64's BVH cases); the mesh, guard and LDS-table bits by `guards`.
hipError_t launch_diag_vertex_fused(const DevScene& sc, const RenderArgs& a, const DiagVertexArgs& v, int guards,
                                    bool mesh_nearest, hipStream_t st) {
    if (v.n <= 0) return hipSuccess;
    if (!sc.compact) return hipErrorInvalidValue;
    const bool mesh = (a.features & 1) != 0;
    if ((guards == 1 && mesh) || (guards == 2 && !mesh) || (mesh_nearest && guards == 1)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((v.n + 255) / 256)), block(256);
    const int pm = a.features & 6;  // Phong, MIS
#define RT_DV_CASE(PM, F, COLD)                                                                       \
    case PM: hipLaunchKernelGGL((k_diag_vertex_fused<(F) | (PM), COLD>), grid, block, 0, st, sc, a, v); break;
#define RT_DV_SWITCH(F, COLD)                                                                         \
    switch (pm) { RT_DV_CASE(0, F, COLD) RT_DV_CASE(2, F, COLD) RT_DV_CASE(4, F, COLD) RT_DV_CASE(6, F, COLD) }
    const int bvh = mesh_nearest ? 16 : 0;
    if (guards == 0) {  // k_trace_f64's choice of C for a compact scene: the mesh code compiled in
        if (bvh) RT_DV_SWITCH(25, false) else RT_DV_SWITCH(9, false)
    } else if (guards == 1) {
        RT_DV_SWITCH(8, false)
    } else if (guards == 2) {
        if (bvh) RT_DV_SWITCH(25 | kCfgGuards1 | kCfgTabUse, false) else RT_DV_SWITCH(9 | kCfgGuards1 | kCfgTabUse, false)
    } else if (!mesh) {  // fused_body's C: F | kCfgLdsObj for a compact scene, | kCfgGuards1 with meshes
        RT_DV_SWITCH(8 | kCfgLdsObj, true)
    } else if (bvh) {
        RT_DV_SWITCH(25 | kCfgLdsObj | kCfgGuards1 | kCfgTabUse, true)
    } else {
        RT_DV_SWITCH(9 | kCfgLdsObj | kCfgGuards1 | kCfgTabUse, true)
    }
#undef RT_DV_SWITCH
#undef RT_DV_CASE
    return hipGetLastError();
}

// rt_diag_sincos: path_f64.h sincos_2pi per lane.
__global__ __launch_bounds__(256) void k_diag_sincos(long n, const double* __restrict__ x, double* __restrict__ s,
                                                     double* __restrict__ c) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double sv, cv;
    sincos_2pi(x[i], &sv, &cv);
    s[i] = sv;
    c[i] = cv;
}
hipError_t launch_diag_sincos(long n, const double* x, double* s, double* c, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_diag_sincos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, x, s, c);
    return hipGetLastError();
}

thread_local TailPlan t_tail_plan;

// The instance of the fused body for (F, W) and unit kind L.
template <int F, int W, int L>
constexpr auto mk_kernel() {
    if constexpr (L == kPasses) return &k_render_passes_f64<F, W>;
    else if constexpr (L == kList) return &k_render_list_f64<F, W>;
    else return &k_megakernel_f64<F, W>;
}

// One launch of the fused body. A frame (L = kFrame) plans its split tail and sums it afterwards; a pixel list or a
// list of passes (nsub = a.n_whole = 4 units.n) is handed out in runs of whole units only, with no split tail.
template <int F, int W, int L>
static void launch_mk(const DevScene& sc, const RenderArgs& a_in, double* sub_buf, uint32_t* next_sub, long nsub,
                      int refill, double* tail_buf, size_t tail_cap, const UnitList& units, hipStream_t st) {
    RenderArgs a = a_in;
    constexpr auto kernel = mk_kernel<F, W, L>();
    const long blocks = resident_blocks(kernel, (nsub + 255) / 256);
    if constexpr (L == kFrame)
        plan_tail(a, nsub, blocks * 256, tail_buf, tail_cap, tail_split_x2(nsub, blocks * 256), 2, 256, RT_MK_MIN_RUN);
    else
        plan_units(a, blocks * 256, 256, RT_MK_MIN_RUN);
    launch_units<L>(kernel, blocks, 256, st, units, sc, a, sub_buf, next_sub, nsub, refill);
    launch_tail_sum_f64(a, sub_buf, nsub - a.n_whole, st);  // (nothing for a list: nsub == a.n_whole)
}

// The analytic / fused-mesh megakernel at its waves/SIMD: 4 for analytic scenes, 3 with meshes (the defaults);
// A/B builds (ab_knobs.h) compile both shapes of every frame instance for RT_MK_WAVES.
template <int F, int L>
static void launch_mk_shape(int waves, const DevScene& sc, const RenderArgs& a, double* sub_buf, uint32_t* next_sub,
                            long nsub, int refill, double* tail_buf, size_t tail_cap, const UnitList& units,
                            hipStream_t st) {
    (void)waves;
    if constexpr (RT_AB_KNOBS != 0 && L == kFrame) {
        if (waves == 3) launch_mk<F, 3, L>(sc, a, sub_buf, next_sub, nsub, refill, tail_buf, tail_cap, units, st);
        else launch_mk<F, RT_MK_W4, L>(sc, a, sub_buf, next_sub, nsub, refill, tail_buf, tail_cap, units, st);
    } else if constexpr ((F & 1) != 0) {
        launch_mk<F, 3, L>(sc, a, sub_buf, next_sub, nsub, refill, tail_buf, tail_cap, units, st);
    } else {
        launch_mk<F, RT_MK_W4, L>(sc, a, sub_buf, next_sub, nsub, refill, tail_buf, tail_cap, units, st);
    }
}

// camera-sample buffer refill threshold (lanes per wave; 0 disables the buffer)
// (24 until round 2; 32-48 measured +0.6-0.9% on cornell, profiles/r02_ab.log)
static int cam_refill() {
    static const int refill = env_int("RT_MK_CAM_REFILL", 40);
    return refill;
}

// The fused instance of a.features & 15, for a frame, a pixel list or a list of passes.
template <int L>
static void launch_mk_features(int waves, const DevScene& sc, const RenderArgs& a, double* sub_buf, uint32_t* next_sub,
                               long nsub, double* tail_buf, size_t tail_cap, const UnitList& units, hipStream_t st) {
    const int refill = cam_refill();
#define RT_MK_CASE(F)                                                                                              \
    case F:                                                                                                        \
        launch_mk_shape<F, L>(waves, sc, a, sub_buf, next_sub, nsub, refill, tail_buf, tail_cap, units, st);       \
        break;
    switch (a.features & 15) {
        RT_MK_CASE(0) RT_MK_CASE(1) RT_MK_CASE(2) RT_MK_CASE(3) RT_MK_CASE(4) RT_MK_CASE(5) RT_MK_CASE(6)
        RT_MK_CASE(7) RT_MK_CASE(8) RT_MK_CASE(9) RT_MK_CASE(10) RT_MK_CASE(11) RT_MK_CASE(12) RT_MK_CASE(13)
        RT_MK_CASE(14) RT_MK_CASE(15)
    }
#undef RT_MK_CASE
}

hipError_t launch_megakernel_f64(const DevScene& sc, const RenderArgs& a_in, double* sub_buf, uint32_t* next_sub,
                                 double* tail_buf, size_t tail_cap, hipStream_t st) {
    RenderArgs a = a_in;
    a.n_whole = (int32_t)((long)a.tw * a.th * 4);  // no split tail unless planned (analytic megakernel)
    a.chunk_lg = 0;
    a.tail_cps = 1;
    const long nsub = (long)a.tw * a.th * 4;
    if (nsub <= 0 || a.n_samples <= 0) return hipSuccess;
    t_tail_plan = TailPlan{};
    hipError_t e = hipMemsetAsync(next_sub, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    // Occupancy (waves/SIMD requested from the register allocator): 4 (128 VGPRs, a few spills)
    // measured fastest for the analytic scenes, 3 (no spills) for the fused mesh kernel
    // (profiles/r01_waves_ab.log); RT_MK_WAVES=3|4 overrides for A/B runs.
    static const int waves_env = env_int("RT_MK_WAVES", 0);
    const int waves = waves_env ? waves_env : ((a.features & 1) ? 3 : 4);
    // Mesh scenes with compact tables and an octree of at least RT_MK_INTERLEAVE nodes: interleaved
    // walks, RT_MK_KSTEPS walk steps per vertex iteration, 2 waves/SIMD (the parked walk state takes
    // 59 KB of LDS per block; 0 selects the fused per-vertex traversal for A/B runs). Shallow octrees (cubes: 9 nodes) walk in a few
    // steps: the fused traversal is faster there (profiles/r01_interleave_ab.log).
    static const int interleave = env_int("RT_MK_INTERLEAVE", 64);
    const int refill = cam_refill();
    static const int wmin = std::max(1, env_int("RT_MK_WALK_MIN", 1));
    static const int bvh_fused = env_int("RT_MK_BVH_FUSED", 0);  // A/B: nearest-triangle mode without interleaving
    // scenes whose meshes are all flat octrees (the cubes): block-synchronous batched mesh queries
    static const int flat = env_int("RT_MK_FLAT", 1);
    if (flat && a.all_flat && (a.features & 25) == 9)
        return launch_megakernel_flat_f64(sc, a, sub_buf, next_sub, tail_buf, tail_cap, refill, st);
    if (interleave && (a.features & 9) == 9 && a.mesh_nodes >= interleave && !((a.features & 16) && bvh_fused)) {
        return launch_megakernel_mesh_f64(sc, a, sub_buf, next_sub, nsub, refill, wmin, tail_buf, tail_cap, st);
    }
    if (a.features & 16) {
        // nearest-triangle meshes (RT_FLAG_MESH_NEAREST) in small or non-compact scenes: BVH
        // traversal inline, 3 waves/SIMD
#define RT_MB_CASE(F)                                                                             \
    case F:                                                                                       \
        launch_mk<F, 3, kFrame>(sc, a, sub_buf, next_sub, nsub, refill, tail_buf, tail_cap, UnitList{}, st); \
        break;
        switch (a.features & 31) {
            RT_MB_CASE(17) RT_MB_CASE(19) RT_MB_CASE(21) RT_MB_CASE(23) RT_MB_CASE(25) RT_MB_CASE(27) RT_MB_CASE(29)
            RT_MB_CASE(31)
        }
#undef RT_MB_CASE
        return hipGetLastError();
    }
    launch_mk_features<kFrame>(waves, sc, a, sub_buf, next_sub, nsub, tail_buf, tail_cap, UnitList{}, st);
    return hipGetLastError();
}

// Pixel-list render and batched passes. family kListFused: the fused body's kList or kPasses
// instance of a.features & 15, with the frame's Cfg choice, mesh instances at 3 waves/SIMD and analytic ones at
// RT_MK_W4, handed out in runs of whole units (plan_units, no split tail); kListFpool / kListRoles: the list or passes
// instances of the scene's pool kernel, planned as its frame is (split tail included). RT_FLAG_FP32 and
// RT_FLAG_MESH_NEAREST are out of scope (check_render_pixels returns RT_E_INVAL).
hipError_t launch_render_units_f64(const DevScene& sc, const RenderArgs& a_in, const UnitList& units, double* sub_buf,
                                   uint32_t* next_unit, int family, double* tail_buf, size_t tail_cap, hipStream_t st) {
    if (units.n <= 0 || a_in.n_samples <= 0) return hipSuccess;
    if (units.n > 0x7fffffffL / 4 || !units.words) return hipErrorInvalidValue;
    if (units.seeds && (long)a_in.width * a_in.height > (long)kPassPixMask) return hipErrorInvalidValue;
    RenderArgs a = a_in;
    a.n_whole = (int32_t)(units.n * 4);  // every unit is a whole subpixel unless a pool launcher plans a split tail
    a.chunk_lg = 0;
    a.tail_cps = 1;
    a.tail_buf = nullptr;
    t_tail_plan = TailPlan{};
    hipError_t e = hipMemsetAsync(next_unit, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    // a mesh scene's pool family (the kernel its full frame runs); a family the scene has no
    // instance of is an error, never a quiet change of kernel
    if (family != kListFused) {
        if (family != list_pool_family(a, sc.node_slot != nullptr)) return hipErrorInvalidValue;
        if (family == kListFpool) return launch_render_units_flat_f64(sc, a, units, sub_buf, next_unit, tail_buf, tail_cap, st);
        return launch_render_units_roles_f64(sc, a, units, sub_buf, next_unit, tail_buf, tail_cap, st);
    }
    if (units.kind() == kPasses) launch_mk_features<kPasses>(0, sc, a, sub_buf, next_unit, a.n_whole, nullptr, 0, units, st);
    else launch_mk_features<kList>(0, sc, a, sub_buf, next_unit, a.n_whole, nullptr, 0, units, st);
    return hipGetLastError();
}

// Scratch bytes one split subpixel needs (plan_tail: the samples after chunk 0, at the default chunk size).
size_t tail_scratch_per_subpixel(int n_samples) {
    RenderArgs a{};
    a.n_samples = n_samples;
    plan_tail(a, 0, 0, nullptr, 0);
    return (size_t)std::max(0, n_samples - (1 << a.chunk_lg)) * 3 * sizeof(double);
}

void launch_tail_sum_f64(const RenderArgs& a, double* sub_buf, long n_split, hipStream_t st) {
    if (n_split <= 0) return;
    const long tb = std::max(1L, std::min(4096L, (n_split + 255) / 256));
    hipLaunchKernelGGL(k_tail_sum_f64, dim3((unsigned)tb), dim3(256), 0, st, a, sub_buf, n_split);
}

hipError_t launch_finalize_f64(const RenderArgs& a, const double* sub_buf, hipStream_t st) {
    const long npix = (long)a.tw * a.th;
    if (npix <= 0) return hipSuccess;
    const long blocks = std::max(1L, std::min(2048L, (npix + 255) / 256));
    hipLaunchKernelGGL(k_finalize_f64, dim3((unsigned)blocks), dim3(256), 0, st, a, sub_buf);
    return hipGetLastError();
}

// Self-test of the exact-arithmetic shortcuts against the IEEE operations they replace: for n
// pseudo-random (a, b) with |b| spread over [2^-900, 2^900] (every exponent, random and extreme
// mantissas), counts rcp_rn(b) != 1.0 / b and qdiv(a, b, rcp_rn(b)) != a / b; and for x spread over
// sqrt_rn's fast range [2^-767, 2^1024) (every exponent, random and extreme mantissas), counts
// sqrt_rn(x) != sqrt(x) (the library sequence with its input scaling and 0/inf fixup). sqrt_rn takes
// its fast path only when the whole wave is in range (a wave vote), so bit equality with the library
// is what makes a lane's result independent of the other lanes of its wave; bad[3] and bad[4] (below) check
// the fused normalise and that property itself, in waves where one lane is outside the fast ranges.
__global__ void k_selftest_arith(long n, uint64_t seed, unsigned long long* bad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng g(seed, (uint32_t)i, (uint32_t)(i >> 32), 7u);
    const uint64_t m = g.next(), m2 = g.next(), sel = g.next(), m3 = g.next(), sel2 = g.next();
    uint64_t mant = m & 0xFFFFFFFFFFFFFull;
    if ((sel & 7) == 0) mant = 0;                              // powers of two
    if ((sel & 7) == 1) mant = 0xFFFFFFFFFFFFFull;             // just below
    if ((sel & 7) == 2) mant = (sel >> 8) & 0xFF;              // just above
    const int ex = -900 + (int)((sel >> 16) % 1801);
    const uint64_t bits = ((uint64_t)(ex + 1023) << 52) | mant | ((sel >> 40) & 1 ? 0x8000000000000000ull : 0);
    const double b = __longlong_as_double((long long)bits);
    const double a = __longlong_as_double((long long)((m2 & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 + (int)((sel >> 48) % 200) - 100) << 52)));
    const double y = rcp_rn(b);
    unsigned long long e = 0;
    if (__double_as_longlong(y) != __double_as_longlong(1.0 / b)) e |= 1;
    if (__double_as_longlong(qdiv(a, b, y)) != __double_as_longlong(a / b)) e |= 2;
    uint64_t sm = m3 & 0xFFFFFFFFFFFFFull;
    if ((sel2 & 7) == 0) sm = 0;
    if ((sel2 & 7) == 1) sm = 0xFFFFFFFFFFFFFull;
    if ((sel2 & 7) == 2) sm = (sel2 >> 8) & 0xFF;
    if ((sel2 & 7) == 3) sm = 0xFFFFFFFFFFFFFull - ((sel2 >> 8) & 0xFF);
    const int sx = -767 + (int)((sel2 >> 16) % 1791);  // [-767, 1023]
    const double x = __longlong_as_double((long long)(((uint64_t)(sx + 1023) << 52) | sm));
    if (__double_as_longlong(sqrt_rn(x)) != __double_as_longlong(sqrt(x))) e |= 4;
    // bad[3]: the fused normalise div_sqrt(v, x) against s = sqrt(x), v / s (library sqrt, IEEE divisions), root
    // and quotients, inside the fast range: once for a vector with its own squared length (largest component
    // 2^h, h in [-383, 510], the others up to 2^-3 of it or +-0, so x lies in [2^-766, 2^1024)), once for the x
    // drawn above (every exponent of [2^-767, 2^1023], extreme mantissas) under a vector within 2^-100 of its root.
    const uint64_t m4 = g.next(), m5 = g.next(), m6 = g.next(), sel3 = g.next();
    const auto comp = [](uint64_t mbits, int ex, uint64_t how) {  // +-(1.m) 2^ex; how & 3 == 3: +-0
        const uint64_t sign = mbits & 0x8000000000000000ull;
        if ((how & 3) == 3) return __longlong_as_double((long long)sign);
        uint64_t mt = mbits & 0xFFFFFFFFFFFFFull;
        if ((how & 12) == 4) mt = 0;
        if ((how & 12) == 8) mt = 0xFFFFFFFFFFFFFull;
        return __longlong_as_double((long long)(sign | ((uint64_t)(ex + 1023) << 52) | mt));
    };
    const auto same = [](double p, double q) {  // equal bits, or both NaN
        return __double_as_longlong(p) == __double_as_longlong(q) || (p != p && q != q);
    };
    const auto same_ds = [&](V3 v, double r) {  // div_sqrt(v, r) against the library forms
        double root;
        const V3 f = div_sqrt(v, r, &root);
        const double s = sqrt(r);
        return same(root, s) && same(f.x, v.x / s) && same(f.y, v.y / s) && same(f.z, v.z / s);
    };
    const int h0 = -383 + (int)((sel3 >> 16) % 894);  // [-383, 510]
    const V3 va = v3(comp(m4, h0, 0), comp(m5, h0 - (int)((sel3 >> 4) & 3), sel3 >> 6),
                     comp(m6, h0 - (int)((sel3 >> 10) & 3), sel3 >> 12));
    const double xa = va.x * va.x + va.y * va.y + va.z * va.z;
    const int hs = sx >> 1;  // the root's exponent (floor)
    const V3 vb = v3(comp(m4, hs - (int)((sel3 >> 32) % 101), sel3 >> 40), comp(m5, hs - (int)((sel3 >> 44) % 101), 0),
                     comp(m6, hs, sel3 >> 52));
    if (!same_ds(va, xa) || !same_ds(vb, x)) e |= 8;
    // bad[4]: the same comparison plus sqrt_rn, rcp_any and V3 / s where a wave is mixed: in every fourth
    // wave one lane (its index rotating) holds an operand outside the fast ranges (0, a subnormal, -0, inf, NaN;
    // 2^-800 or a negative number as radicand; 2^-1000 or 2^1000 as divisor), or one at an edge of the guards'
    // windows: 2^900 (in rcp_safe, outside the high-dword window), the next double above it, the largest double
    // below 2^-900, the largest double below 2^-767 as radicand; inside: 2^-767 and the next double, -2^-900, the
    // largest finite double. Every lane of such a wave must still give the library's bits: that is what makes a
    // lane's result independent of its wave-mates. Both guard forms are checked (G1: the fused mesh instances').
    const long wv = i >> 6;
    double xp = x, bp = b;
    if ((wv & 3) == 3 && (int)(i & 63) == (int)((wv >> 2) & 63)) {
        const uint64_t sub = (m4 & 0xFFFFFFFFFFFFFull) | 1ull;  // a subnormal
        switch ((int)((wv >> 2) % 15)) {
        case 0: xp = 0.0; bp = 0.0; break;
        case 1: xp = __longlong_as_double((long long)sub); bp = xp; break;
        case 2: xp = 0x1p-800; bp = -0.0; break;
        case 3: xp = INFINITY; bp = INFINITY; break;
        case 4: xp = __longlong_as_double(0x7FF8000000000000ll); bp = xp; break;
        case 5: xp = -x; bp = -INFINITY; break;
        case 6: xp = -0.0; bp = -__longlong_as_double((long long)sub); break;
        case 7: bp = 0x1p-1000; break;
        case 8: bp = -0x1p1000; break;
        case 9: bp = 0x1p900; xp = 0x1p-767; break;
        case 10: bp = 0x1.0000000000001p900; xp = 0x1.fffffffffffffp-768; break;
        case 11: bp = -0x1.fffffffffffffp-901; xp = 0x1.fffffffffffffp1023; break;
        case 12: bp = -0x1p-900; xp = 0x1.0000000000001p-767; break;
        case 13: bp = 0x1.fffffffffffffp1023; xp = -0x1.fffffffffffffp-768; break;
        default: bp = 0x1.fffffffffffffp899; xp = 0x1p-768; break;
        }
    }
    bool ok = same_ds(vb, xp) && same(sqrt_rn(xp), sqrt(xp)) && same(rcp_any(bp), 1.0 / bp);
    ok = ok && same(sqrt_rn<true>(xp), sqrt(xp)) && same(rcp_any<true>(bp), 1.0 / bp);
    // numerators within 2^+-100 like a (the quotient neither overflows nor underflows), one of them +-0 at times
    const V3 nv = v3(a, comp(m5, (int)((sel3 >> 20) % 200) - 100, 0), comp(m6, (int)((sel3 >> 28) % 200) - 100, sel3 >> 12));
    const V3 qv = nv / bp;
    ok = ok && same(qv.x, nv.x / bp) && same(qv.y, nv.y / bp) && same(qv.z, nv.z / bp);
    double r1;
    // (G1 divides by an in-range root of an out-of-range radicand through qdiv: nv keeps that quotient in range too)
    const V3 q1 = vdiv<true>(nv, bp), d1 = div_sqrt<true>(nv, xp, &r1);
    const double s1 = sqrt(xp);
    ok = ok && same(q1.x, nv.x / bp) && same(q1.y, nv.y / bp) && same(q1.z, nv.z / bp);
    ok = ok && same(r1, s1) && same(d1.x, nv.x / s1) && same(d1.y, nv.y / s1) && same(d1.z, nv.z / s1);
    if (!ok) e |= 16;
    if (e & 1) atomicAdd(&bad[0], 1ull);
    if (e & 2) atomicAdd(&bad[1], 1ull);
    if (e & 4) atomicAdd(&bad[2], 1ull);
    if (e & 8) atomicAdd(&bad[3], 1ull);
    if (e & 16) atomicAdd(&bad[4], 1ull);
}

// Diagnostic builds: the wave records of the last k_megakernel_f64 launches (start, half-idle, end per wave, on
// the 100 MHz s_memrealtime clock; zeros for waves that did not run), then cleared; 1 (zeros) without timers.
extern "C" int rt_debug_wave_times(unsigned long long* out, int n_waves) {
    if (!out || n_waves <= 0) return -1;
    for (long i = 0; i < 5L * n_waves; ++i) out[i] = 0;
#if RT_DEBUG_TIMERS
    const int n = std::min(n_waves, kDbgWaves);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg_wave), kDbgWaveRec * sizeof(unsigned long long) * n) != hipSuccess) return -1;
    static unsigned long long zeros[kDbgWaveRec * kDbgWaves];
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_wave), zeros, sizeof zeros) != hipSuccess) return -1;
    return 0;
#else
    return 1;
#endif
}

// The split tail of the calling thread's last megakernel launch (kernels.h TailPlan).
extern "C" int rt_debug_last_split(long long out[3]) {
    if (!out) return -1;
    out[0] = t_tail_plan.n_split;
    out[1] = t_tail_plan.want;
    out[2] = t_tail_plan.chunk;
    return 0;
}

// n_out: the caller's output count (at most 5 are written: reciprocal, quotient, square root, fused normalise,
// mixed waves)
extern "C" int rt_selftest_arith_n(long n, unsigned long long seed, unsigned long long* out, int n_out) {
    constexpr int kCounts = 5;
    unsigned long long* d = nullptr;
    if (n <= 0 || !out || n_out <= 0 || hipMalloc(&d, kCounts * sizeof(unsigned long long)) != hipSuccess) return -1;
    int rc = 0;
    unsigned long long h[kCounts] = {0, 0, 0, 0, 0};
    if (hipMemset(d, 0, kCounts * sizeof(unsigned long long)) != hipSuccess) rc = -1;
    if (!rc) {
        hipLaunchKernelGGL(k_selftest_arith, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, seed, d);
        if (hipGetLastError() != hipSuccess || hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    }
    (void)hipFree(d);
    for (int i = 0; i < n_out && i < kCounts; ++i) out[i] = h[i];
    return rc;
}
// The original two-output entry point (reciprocal, quotient), kept for callers built against it.
extern "C" int rt_selftest_arith(long n, unsigned long long seed, unsigned long long out[2]) {
    return rt_selftest_arith_n(n, seed, out, 2);
}

// Pointer round trips of the per-call views every trace call goes through (scene.rs:272-289 reads the
// scene's tables): the compact-table pointer rebuilt from two readfirstlane halves (tables()), the scene
// and render arguments read in place in the kernarg segment (karg_scene / karg_render_args at offsets 0
// and 248, the megakernels' own parameter order). out[0] tables() through the kernarg view, [1] tables()
// of the by-value argument, [2] the round-4 sign-extending form (tables_form<true>), [3] the kernarg
// view's raw ctab, [4] its node_slot, [5] karg_render_args().tail_buf. The pointers are never
// dereferenced, so fabricated addresses are safe.
__global__ __launch_bounds__(64) void k_selftest_tables(DevScene sc_g, RenderArgs a_g, unsigned long long* out) {
    const DevScene& sc = karg_scene();
    const RenderArgs& a = karg_render_args();
    const uint64_t v[6] = {(uint64_t)(uintptr_t)tables(sc), (uint64_t)(uintptr_t)tables(sc_g),
                           (uint64_t)(uintptr_t)tables_form<true>(sc), (uint64_t)(uintptr_t)sc.ctab,
                           (uint64_t)(uintptr_t)sc.node_slot, (uint64_t)(uintptr_t)a.tail_buf};
    (void)a_g;
    if (threadIdx.x < 6) out[threadIdx.x] = v[threadIdx.x];
}

extern "C" int rt_selftest_tables(const unsigned long long* ptrs, int n, unsigned long long* out) {
    if (!ptrs || !out || n <= 0) return -1;
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, 6 * sizeof(unsigned long long)) != hipSuccess) return -1;
    int rc = 0;
    for (int i = 0; i < n && !rc; ++i) {
        DevScene sc{};
        RenderArgs a{};
        sc.ctab = (const CompactTab*)(uintptr_t)ptrs[i];
        sc.node_slot = (const KidSlot*)(uintptr_t)(ptrs[i] + 16);
        a.tail_buf = (double*)(uintptr_t)(ptrs[i] + 32);
        hipLaunchKernelGGL(k_selftest_tables, dim3(1), dim3(64), 0, 0, sc, a, d);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out + 6 * (size_t)i, d, 6 * sizeof(unsigned long long),
                                                         hipMemcpyDeviceToHost) != hipSuccess)
            rc = -1;
    }
    (void)hipFree(d);
    return rc;
}

#define RT_DIAG_TU_FN diag_read_main
#include "diag_tu.h"

// Diagnostic builds: the counters of every kernel code object, summed, then cleared (zeros otherwise);
// a null output leaves that set alone.
static int diag_all(unsigned long long* cnt16, unsigned long long* reg32, unsigned long long* tim16, unsigned long long* q4) {
    for (int i = 0; i < 16; ++i) {
        if (cnt16) cnt16[i] = 0;
        if (tim16) tim16[i] = 0;
    }
    for (int i = 0; i < 32 && reg32; ++i) reg32[i] = 0;
    for (int i = 0; i < 4 && q4; ++i) q4[i] = 0;
    if (diag_read_main(cnt16, reg32, tim16, q4) || diag_read_mesh(cnt16, reg32, tim16, q4) ||
        diag_read_flat(cnt16, reg32, tim16, q4))
        return -1;
    return 0;
}

// RT_QCHECK builds: read and clear the LDS hand-off protocol counters (megakernel_common.h);
// returns 1 (and zeros) when the checks are not compiled in.
extern "C" int rt_debug_qcheck(unsigned long long out[4]) {
#if RT_QCHECK
    return diag_all(nullptr, nullptr, nullptr, out);
#else
    for (int i = 0; i < 4; ++i) out[i] = 0;
    return 1;
#endif
}

// Diagnostic builds: read and clear the region counters and timers (all zeros otherwise).
extern "C" int rt_debug_regions(unsigned long long out[64]) {
    for (int i = 48; i < 64; ++i) out[i] = 0;
    return diag_all(nullptr, out, out + 32, nullptr);
}

// Diagnostic builds: read and clear the traversal counters (all zeros otherwise).
extern "C" int rt_debug_counters(unsigned long long out[16]) {
    return diag_all(out, nullptr, nullptr, nullptr);
}

hipError_t launch_trace_f64(const DevScene& sc, long n, const double* o, const double* d, double* t, int32_t* obj,
                            double* pos, double* nrm, bool mesh_nearest, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_trace_f64, dim3((unsigned)blocks), dim3(256), 0, st, sc, n, o, d, t, obj, pos, nrm,
                       mesh_nearest ? 1 : 0);
    return hipGetLastError();
}

}  // namespace rt
