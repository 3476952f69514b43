// Progressive accumulation for gfx950.
//
//   k_accum_add     — merges one pass's subpixel means into the two f64 sums S = sum n m, Q = sum n m^2.
//   k_accum_resolve — the accumulated subpixel means S / N and the variance of the clamped pixel colour.
// Both stream: every access is a 16-byte load or store of consecutive lanes. Compiled without FMA contraction (the
// Makefile's -ffp-contract=off), so tests/accum_ref.py restates them bit for bit.
// Rendering to an error target (restated by tests/adapt_ref.py):
//   k_accum_cnt_fill, k_accum_add_list, k_accum_resolve_cnt — per-pixel counts (K_p, N_p) and sparse merges.
//   k_select_count / k_select_scan / k_select_write — the pixels whose estimated error is above a target, ascending.
// Batched passes (restated by tests/batch_ref.py):
//   k_plan_count / k_plan_write — the selection plus a pass count per pixel; k_runs_count / k_runs_write — the
//   list's expansion into (pixel, pass) units; k_accum_add_runs — the run merge.
// Filling the holes of a reprojection (restated by tests/fill_ref.py):
//   k_holes_count — the pixels without two passes, and a refresh pattern; feeds k_select_scan / k_select_write.
#include <hip/hip_runtime.h>

#include "accum.h"

namespace rt {

// One lane per pair of elements (a pixel's 12 doubles are 6 pairs; npix * 6 pairs in all).
template <bool kFirst>
__global__ __launch_bounds__(256) void k_accum_add(double2* __restrict__ S, double2* __restrict__ Q,
                                                   const double2* __restrict__ m, long npairs, double n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    const double2 v = m[i];
    const double ax = n * v.x, ay = n * v.y;
    double2 s = make_double2(ax, ay), q = make_double2(ax * v.x, ay * v.y);
    if (!kFirst) {
        const double2 s0 = S[i], q0 = Q[i];
        s = make_double2(s0.x + s.x, s0.y + s.y);
        q = make_double2(q0.x + q.x, q0.y + q.y);
    }
    S[i] = s;
    Q[i] = q;
}

// Pixel p's resolve with N samples per subpixel and K1 = K - 1 (unused when var is null).
__device__ __forceinline__ void resolve_pixel(const double2* __restrict__ S, const double2* __restrict__ Q, long p,
                                              double N, double K1, double2* __restrict__ sub,
                                              float4* __restrict__ var) {
    double m[12];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double2 s = S[(size_t)p * 6 + k];
        m[2 * k] = s.x / N;
        m[2 * k + 1] = s.y / N;
    }
    if (sub) {
#pragma unroll
        for (int k = 0; k < 6; ++k) sub[(size_t)p * 6 + k] = make_double2(m[2 * k], m[2 * k + 1]);
    }
    if (var) {
        double vs[12];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double2 q = Q[(size_t)p * 6 + k];
            const double dx = q.x / N - m[2 * k] * m[2 * k], dy = q.y / N - m[2 * k + 1] * m[2 * k + 1];
            vs[2 * k] = (dx > 0. ? dx : 0.) / K1;
            vs[2 * k + 1] = (dy > 0. ? dy : 0.) / K1;
        }
        double v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double a = 0.;
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // the clamp passes a subpixel's scatter on only inside (0, 1)
                const double mj = m[3 * j + c];
                a = a + ((mj > 0. && mj < 1.) ? vs[3 * j + c] : 0.);
            }
            v[c] = a / 16.;
        }
        var[p] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)((v[0] + v[1]) + v[2]));
    }
}

// One lane per pixel, one K and N for the frame.
__global__ __launch_bounds__(256) void k_accum_resolve(const double2* __restrict__ S, const double2* __restrict__ Q,
                                                       long npix, double N, double K1, double2* __restrict__ sub,
                                                       float4* __restrict__ var) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    resolve_pixel(S, Q, p, N, K1, sub, var);
}

// The same with the pixel's own counts: N_p and K_p - 1.
__global__ __launch_bounds__(256) void k_accum_resolve_cnt(const double2* __restrict__ S, const double2* __restrict__ Q,
                                                           const uint2* __restrict__ cnt, long npix,
                                                           double2* __restrict__ sub, float4* __restrict__ var) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const uint2 c = cnt[p];
    resolve_pixel(S, Q, p, (double)c.y, (double)c.x - 1.0, sub, var);
}

// Per-pixel counts and sparse merges ---------------------------------------------------------

// cnt[p] = (K, N), or cnt[p] += (K, N). One lane per pixel.
template <bool kAdd>
__global__ __launch_bounds__(256) void k_accum_cnt_fill(uint2* __restrict__ cnt, long npix, uint32_t K, uint32_t N) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    uint2 c = make_uint2(K, N);
    if (kAdd) {
        const uint2 c0 = cnt[p];
        c = make_uint2(c0.x + K, c0.y + N);
    }
    cnt[p] = c;
}

// One lane per (list entry, pair of elements): k_accum_add<false>'s expression at the entry's pixel. The list is
// unique, so no two lanes touch one element; the lane of pair 0 counts the pass.
__global__ __launch_bounds__(256) void k_accum_add_list(double2* __restrict__ S, double2* __restrict__ Q,
                                                        uint2* __restrict__ cnt, const uint32_t* __restrict__ list,
                                                        const double2* __restrict__ m, long npairs, double n,
                                                        uint32_t n_u) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    const long e = i / 6;
    const int k = (int)(i - e * 6);
    const uint32_t p = list[e];
    const size_t at = (size_t)p * 6 + k;
    const double2 v = m[i];
    const double ax = n * v.x, ay = n * v.y;
    const double2 s0 = S[at], q0 = Q[at];
    S[at] = make_double2(s0.x + ax, s0.y + ay);
    Q[at] = make_double2(q0.x + ax * v.x, q0.y + ay * v.y);
    if (k == 0) {
        const uint2 c = cnt[p];
        cnt[p] = make_uint2(c.x + 1u, c.y + n_u);
    }
}

// Selection: is pixel p active? (rt_ffi.h rt_accum_select; tests/adapt_ref.py restates it operation by operation)
// g_out, thr_out, n_out: the error estimate, the target and N_p the answer was made from (the plan's inputs).
__device__ __forceinline__ bool select_terms(const double2* __restrict__ S, const float4* __restrict__ var,
                                             const uint2* __restrict__ cnt, double N, int width, int height,
                                             double abs_tol, double rel_tol, int32_t max_n, long p, double& g_out,
                                             double& thr_out, int64_t& n_out) {
    const int row = (int)(p / width), col = (int)(p - (long)row * width);
    double num = 0., den = 0.;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int r = row + dy, c = col + dx;
            if (r < 0 || r >= height || c < 0 || c >= width) continue;
            const double kk = (dx == 0 ? 0.5 : 0.25) * (dy == 0 ? 0.5 : 0.25);
            num = num + kk * (double)var[(long)r * width + c].w;
            den = den + kk;
        }
    }
    const double g = num / den;
    uint32_t n_p = 0;
    double Np = N;
    if (cnt) {
        n_p = cnt[p].y;
        Np = (double)n_p;
    }
    double m[12];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double2 s = S[(size_t)p * 6 + k];
        m[2 * k] = s.x / Np;
        m[2 * k + 1] = s.y / Np;
    }
    double c3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a = 0.;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double mj = m[3 * j + c];
            a = a + (mj < 0. ? 0. : (mj > 1. ? 1. : mj)) * 0.25;
        }
        c3[c] = a;
    }
    const double y = (c3[0] + c3[1]) + c3[2];
    const double thr = (rel_tol * y) / 3.0 + abs_tol;
    const bool under = max_n <= 0 || (cnt ? (int64_t)n_p : (int64_t)N) < (int64_t)max_n;
    g_out = g;
    thr_out = thr;
    n_out = cnt ? (int64_t)n_p : (int64_t)N;
    return g > thr * thr && under;
}
__device__ __forceinline__ bool select_active(const double2* __restrict__ S, const float4* __restrict__ var,
                                              const uint2* __restrict__ cnt, double N, int width, int height,
                                              double abs_tol, double rel_tol, int32_t max_n, long p) {
    double g, thr;
    int64_t n_p;
    return select_terms(S, var, cnt, N, width, height, abs_tol, rel_tol, max_n, p, g, thr, n_p);
}

// Pass 1: each wave's ballot of active pixels (masks[wave], 64 pixels per wave) and each block's count.
__global__ __launch_bounds__(256) void k_select_count(const double2* __restrict__ S, const float4* __restrict__ var,
                                                      const uint2* __restrict__ cnt, double N, int width, int height,
                                                      double abs_tol, double rel_tol, int32_t max_n,
                                                      unsigned long long* __restrict__ masks,
                                                      uint32_t* __restrict__ block_count) {
    __shared__ uint32_t s_n[4];
    const long npix = (long)width * height;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const bool act = p < npix && select_active(S, var, cnt, N, width, height, abs_tol, rel_tol, max_n, p);
    const unsigned long long mk = __ballot(act);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        masks[(size_t)blockIdx.x * 4 + wave] = mk;
        s_n[wave] = (uint32_t)__popcll(mk);
    }
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
}

// Pass 1 of the hole list of a seeded accumulator (tests/fill_ref.py restates it): pixel p is listed
// iff K_p < 2, or period > 0 and (col + 3 row) mod period == phase. Ballots and block counts as k_select_count stores
// them, for k_select_scan and k_select_write. *n_holes counts the pixels with K_p < 2: one vector atomic per block on
// an integer (order-free); the list's order never depends on it.
__global__ __launch_bounds__(256) void k_holes_count(const uint2* __restrict__ cnt, int width, long npix, int32_t period,
                                                     int32_t phase, unsigned long long* __restrict__ masks,
                                                     uint32_t* __restrict__ block_count,
                                                     unsigned long long* __restrict__ n_holes) {
    __shared__ uint32_t s_n[4], s_h[4];
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    bool hole = false, act = false;
    if (p < npix) {
        hole = cnt[p].x < 2u;
        act = hole;
        if (period > 0) {  // npix fits an int32 (rt_accum_create), so 32-bit divisions do
            const uint32_t row = (uint32_t)p / (uint32_t)width, col = (uint32_t)p - row * (uint32_t)width;
            act = act || (int32_t)(((uint64_t)col + 3ull * (uint64_t)row) % (uint64_t)(uint32_t)period) == phase;
        }
    }
    const unsigned long long mk = __ballot(act), mh = __ballot(hole);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        masks[(size_t)blockIdx.x * 4 + wave] = mk;
        s_n[wave] = (uint32_t)__popcll(mk);
        s_h[wave] = (uint32_t)__popcll(mh);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_count[blockIdx.x] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
        const uint32_t h = (s_h[0] + s_h[1]) + (s_h[2] + s_h[3]);
        if (h != 0u) atomicAdd(n_holes, (unsigned long long)h);
    }
}

// Pass 2 (one block of 1024 threads): the exclusive scan of the block counts, in place; *total = their sum. Each thread
// sums a contiguous segment, the 1024 segment sums are scanned in LDS, then each thread writes its segment's offsets.
__global__ __launch_bounds__(1024) void k_select_scan(uint32_t* __restrict__ block_count, long nblocks,
                                                      uint32_t* __restrict__ total) {
    __shared__ uint32_t s_sum[1024];
    const long per = (nblocks + 1023) / 1024;
    const long b0 = min((long)threadIdx.x * per, nblocks), b1 = min(b0 + per, nblocks);
    uint32_t sum = 0;
    for (long b = b0; b < b1; ++b) sum += block_count[b];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele, inclusive
        const uint32_t add = threadIdx.x >= (unsigned)off ? s_sum[threadIdx.x - off] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = s_sum[threadIdx.x] - sum;  // exclusive
    for (long b = b0; b < b1; ++b) {
        const uint32_t c = block_count[b];
        block_count[b] = run;
        run += c;
    }
    if (threadIdx.x == 1023) *total = s_sum[1023];
}

// Pass 3: ballot-prefix writes, ascending: block offset + the block's earlier waves + the lanes below.
__global__ __launch_bounds__(256) void k_select_write(const unsigned long long* __restrict__ masks,
                                                      const uint32_t* __restrict__ block_off, long npix,
                                                      uint32_t* __restrict__ out, long cap) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long* mb = masks + (size_t)blockIdx.x * 4;
    long at = block_off[blockIdx.x];
    for (int w = 0; w < wave; ++w) at += __popcll(mb[w]);
    const unsigned long long mk = mb[wave];
    if (!((mk >> lane) & 1ull) || p >= npix) return;
    at += __popcll(lane ? (mk & ((~0ull) >> (64 - lane))) : 0ull);
    if (at < cap) out[at] = (uint32_t)p;
}

// Batched passes (restated by tests/batch_ref.py) -----------------------------------------------

// Pass 1 of the plan: k_select_count's ballots and block counts, plus each active pixel's wanted pass count
//   r = g / (thr thr);  need = N_p r - N_p;  x = (gain need) / n;  c = x >= C ? C : max(1, ceil(x));
//   max_n > 0: c = min(c, (max_n - N_p + n - 1) / n)
// in want[p] (0: inactive), and the histogram hist[c] of the wanted counts (integer atomics: order-free).
__global__ __launch_bounds__(256) void k_plan_count(const double2* __restrict__ S, const float4* __restrict__ var,
                                                    const uint2* __restrict__ cnt, double N, int width, int height,
                                                    double abs_tol, double rel_tol, int32_t max_n, int32_t n, double gain,
                                                    int32_t C, unsigned long long* __restrict__ masks,
                                                    uint32_t* __restrict__ block_count, uint8_t* __restrict__ want,
                                                    uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_n[4], s_h[kPassesMax + 1];
    if (threadIdx.x <= kPassesMax) s_h[threadIdx.x] = 0u;
    __syncthreads();
    const long npix = (long)width * height;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    bool act = false;
    int c = 0;
    if (p < npix) {
        double g, thr;
        int64_t n_p;
        act = select_terms(S, var, cnt, N, width, height, abs_tol, rel_tol, max_n, p, g, thr, n_p);
        if (act) {
            const double Np = (double)n_p;
            const double r = g / (thr * thr);
            const double need = Np * r - Np;
            const double x = (gain * need) / (double)n;
            c = x >= (double)C ? C : (x > 1.0 ? (int)ceil(x) : 1);
            if (max_n > 0) {
                const int64_t room = ((int64_t)max_n - n_p + (int64_t)n - 1) / (int64_t)n;
                c = (int64_t)c < room ? c : (int)room;
            }
            atomicAdd(&s_h[c], 1u);
        }
        want[p] = (uint8_t)c;
    }
    const unsigned long long mk = __ballot(act);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        masks[(size_t)blockIdx.x * 4 + wave] = mk;
        s_n[wave] = (uint32_t)__popcll(mk);
    }
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
    if (threadIdx.x <= kPassesMax && s_h[threadIdx.x] != 0u) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
}

// Pass 3 of the plan: k_select_write's positions; the id and min(want, cmax) of each active pixel.
__global__ __launch_bounds__(256) void k_plan_write(const unsigned long long* __restrict__ masks,
                                                    const uint32_t* __restrict__ block_off,
                                                    const uint8_t* __restrict__ want, long npix, int32_t cmax,
                                                    uint32_t* __restrict__ out, uint8_t* __restrict__ counts, long cap) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long* mb = masks + (size_t)blockIdx.x * 4;
    long at = block_off[blockIdx.x];
    for (int w = 0; w < wave; ++w) at += __popcll(mb[w]);
    const unsigned long long mk = mb[wave];
    if (!((mk >> lane) & 1ull) || p >= npix) return;
    at += __popcll(lane ? (mk & ((~0ull) >> (64 - lane))) : 0ull);
    if (at < cap) {
        const int c = want[p];
        out[at] = (uint32_t)p;
        counts[at] = (uint8_t)(c < cmax ? c : cmax);
    }
}

// The expansion of a list with counts into units, pass 1: each block's sum of its 256 entries' counts.
__global__ __launch_bounds__(256) void k_runs_count(const uint8_t* __restrict__ counts, long n,
                                                    uint32_t* __restrict__ block_count) {
    __shared__ uint32_t s_n[4];
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    uint32_t v = e < n ? counts[e] : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
}
// Pass 3 (pass 2 is k_select_scan): off[e] = the exclusive prefix sum of the counts, and entry e's units
// units[off[e] + i] = list[e] | i << 28, i < counts[e]; nothing is written at or past cap units.
__global__ __launch_bounds__(256) void k_runs_write(const uint32_t* __restrict__ list, const uint8_t* __restrict__ counts,
                                                    long n, const uint32_t* __restrict__ block_off,
                                                    uint32_t* __restrict__ off, uint32_t* __restrict__ units, long cap) {
    __shared__ uint32_t s_sum[256];
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = e < n ? counts[e] : 0u;
    s_sum[threadIdx.x] = c;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // Hillis-Steele, inclusive
        const uint32_t add = threadIdx.x >= (unsigned)d ? s_sum[threadIdx.x - d] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += add;
        __syncthreads();
    }
    if (e >= n) return;
    const long o = (long)block_off[blockIdx.x] + (s_sum[threadIdx.x] - c);
    if (off) off[e] = (uint32_t)o;
    const uint32_t p = list[e];
    for (uint32_t i = 0; i < c; ++i)
        if (o + i < cap) units[o + i] = p | (i << 28);
}

// The run merge: one lane per (list entry, pair of elements); the entry's counts[e] consecutive units of m, from
// off[e], are merged in pass order with k_accum_add_list's expression: the bits of counts[e] successive sparse merges.
__global__ __launch_bounds__(256) void k_accum_add_runs(double2* __restrict__ S, double2* __restrict__ Q,
                                                        uint2* __restrict__ cnt, const uint32_t* __restrict__ list,
                                                        const uint8_t* __restrict__ counts,
                                                        const uint32_t* __restrict__ off, const double2* __restrict__ m,
                                                        long npairs, double n, uint32_t n_u) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    const long e = i / 6;
    const int k = (int)(i - e * 6);
    const uint32_t p = list[e], c = counts[e];
    const size_t at = (size_t)p * 6 + k;
    const double2* mu = m + (size_t)off[e] * 6 + k;
    double2 s = S[at], q = Q[at];
    for (uint32_t j = 0; j < c; ++j) {
        const double2 v = mu[(size_t)j * 6];
        const double ax = n * v.x, ay = n * v.y;
        s = make_double2(s.x + ax, s.y + ay);
        q = make_double2(q.x + ax * v.x, q.y + ay * v.y);
    }
    S[at] = s;
    Q[at] = q;
    if (k == 0) {
        const uint2 c0 = cnt[p];
        cnt[p] = make_uint2(c0.x + c, c0.y + c * n_u);
    }
}

static long select_blocks(long npix) { return (npix + 255) / 256; }

hipError_t launch_accum_plan_count(const double* S, const float* var, const uint32_t* cnt, int64_t N, int width,
                                   int height, float abs_tol, float rel_tol, int32_t max_n, int32_t n, float gain,
                                   int32_t max_passes, void* scratch, uint8_t* want, uint32_t* hist, uint32_t* total,
                                   hipStream_t st) {
    const long npix = (long)width * height;
    if (npix <= 0 || n < 1 || max_passes < 1 || max_passes > kPassesMax) return hipErrorInvalidValue;
    const long nb = select_blocks(npix);
    unsigned long long* masks = (unsigned long long*)scratch;
    uint32_t* counts = (uint32_t*)(masks + (size_t)nb * 4);
    hipError_t e = hipMemsetAsync(hist, 0, (kPassesMax + 1) * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_count, dim3((unsigned)nb), dim3(256), 0, st, reinterpret_cast<const double2*>(S),
                       reinterpret_cast<const float4*>(var), reinterpret_cast<const uint2*>(cnt), (double)N, width,
                       height, (double)abs_tol, (double)rel_tol, max_n, n, (double)gain, max_passes, masks, counts, want,
                       hist);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, st, counts, nb, total);
    return hipGetLastError();
}

hipError_t launch_accum_plan_write(const void* scratch, const uint8_t* want, long npix, int32_t cmax, uint32_t* out,
                                   uint8_t* counts, long cap, hipStream_t st) {
    if (npix <= 0 || cap <= 0) return hipSuccess;
    const long nb = select_blocks(npix);
    const unsigned long long* masks = (const unsigned long long*)scratch;
    const uint32_t* block_off = (const uint32_t*)(masks + (size_t)nb * 4);
    hipLaunchKernelGGL(k_plan_write, dim3((unsigned)nb), dim3(256), 0, st, masks, block_off, want, npix, cmax, out, counts,
                       cap);
    return hipGetLastError();
}

size_t runs_scratch_bytes(long n) { return ((size_t)select_blocks(n) + 2) * sizeof(uint32_t); }

hipError_t launch_accum_expand(const uint32_t* list, const uint8_t* counts, long n, void* scratch, uint32_t* off,
                               uint32_t* units, long cap, uint32_t* total, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const long nb = select_blocks(n);
    uint32_t* block_count = (uint32_t*)scratch;
    hipLaunchKernelGGL(k_runs_count, dim3((unsigned)nb), dim3(256), 0, st, counts, n, block_count);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, st, block_count, nb, total);
    hipLaunchKernelGGL(k_runs_write, dim3((unsigned)nb), dim3(256), 0, st, list, counts, n, block_count, off, units, cap);
    return hipGetLastError();
}

hipError_t launch_accum_add_runs(double* S, double* Q, uint32_t* cnt, const uint32_t* list, const uint8_t* counts,
                                 const uint32_t* off, long n_list, const double* m, int32_t n, hipStream_t st) {
    const long npairs = n_list * 6;
    if (npairs <= 0) return hipSuccess;
    const long blocks = (npairs + 255) / 256;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_accum_add_runs, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<double2*>(S),
                       reinterpret_cast<double2*>(Q), reinterpret_cast<uint2*>(cnt), list, counts, off,
                       reinterpret_cast<const double2*>(m), npairs, (double)n, (uint32_t)n);
    return hipGetLastError();
}

size_t select_scratch_bytes(long npix) {
    const size_t nb = (size_t)select_blocks(npix);
    return nb * 4 * sizeof(unsigned long long) + (nb + 2) * sizeof(uint32_t);  // masks | block counts
}

hipError_t launch_accum_select(const double* S, const float* var, const uint32_t* cnt, int64_t N, int width, int height,
                               float abs_tol, float rel_tol, int32_t max_n, void* scratch, uint32_t* out, long cap,
                               uint32_t* total, hipStream_t st) {
    const long npix = (long)width * height;
    if (npix <= 0) return hipErrorInvalidValue;
    const long nb = select_blocks(npix);
    unsigned long long* masks = (unsigned long long*)scratch;
    uint32_t* counts = (uint32_t*)(masks + (size_t)nb * 4);
    hipLaunchKernelGGL(k_select_count, dim3((unsigned)nb), dim3(256), 0, st, reinterpret_cast<const double2*>(S),
                       reinterpret_cast<const float4*>(var), reinterpret_cast<const uint2*>(cnt), (double)N, width,
                       height, (double)abs_tol, (double)rel_tol, max_n, masks, counts);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, st, counts, nb, total);
    if (cap > 0 && out)
        hipLaunchKernelGGL(k_select_write, dim3((unsigned)nb), dim3(256), 0, st, masks, counts, npix, out, cap);
    return hipGetLastError();
}

hipError_t launch_accum_holes(const uint32_t* cnt, int width, int height, int32_t period, int32_t phase, void* scratch,
                              uint32_t* out, long cap, uint32_t* total, unsigned long long* n_holes, hipStream_t st) {
    const long npix = (long)width * height;
    if (npix <= 0 || !cnt || !scratch || !total || !n_holes || period < 0 || phase < 0 || phase >= (period > 1 ? period : 1))
        return hipErrorInvalidValue;
    const long nb = select_blocks(npix);
    unsigned long long* masks = (unsigned long long*)scratch;
    uint32_t* counts = (uint32_t*)(masks + (size_t)nb * 4);
    hipError_t e = hipMemsetAsync(n_holes, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_holes_count, dim3((unsigned)nb), dim3(256), 0, st, reinterpret_cast<const uint2*>(cnt), width,
                       npix, period, phase, masks, counts, n_holes);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, st, counts, nb, total);
    if (cap > 0 && out)
        hipLaunchKernelGGL(k_select_write, dim3((unsigned)nb), dim3(256), 0, st, masks, counts, npix, out, cap);
    return hipGetLastError();
}

hipError_t launch_accum_cnt_fill(uint32_t* cnt, long npix, uint32_t K, uint32_t N, bool add, hipStream_t st) {
    if (npix <= 0) return hipSuccess;
    const long blocks = (npix + 255) / 256;
    if (add)
        hipLaunchKernelGGL(k_accum_cnt_fill<true>, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<uint2*>(cnt),
                           npix, K, N);
    else
        hipLaunchKernelGGL(k_accum_cnt_fill<false>, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<uint2*>(cnt),
                           npix, K, N);
    return hipGetLastError();
}

hipError_t launch_accum_add_list(double* S, double* Q, uint32_t* cnt, const uint32_t* list, long n_list, const double* m,
                                 int32_t n, hipStream_t st) {
    const long npairs = n_list * 6;
    if (npairs <= 0) return hipSuccess;
    const long blocks = (npairs + 255) / 256;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_accum_add_list, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<double2*>(S),
                       reinterpret_cast<double2*>(Q), reinterpret_cast<uint2*>(cnt), list,
                       reinterpret_cast<const double2*>(m), npairs, (double)n, (uint32_t)n);
    return hipGetLastError();
}

hipError_t launch_accum_add(double* S, double* Q, const double* m, long npix, int32_t n, bool first, hipStream_t st) {
    const long npairs = npix * 6;
    if (npairs <= 0) return hipSuccess;
    const long blocks = (npairs + 255) / 256;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    double2* s2 = reinterpret_cast<double2*>(S);
    double2* q2 = reinterpret_cast<double2*>(Q);
    const double2* m2 = reinterpret_cast<const double2*>(m);
    if (first)
        hipLaunchKernelGGL(k_accum_add<true>, dim3((unsigned)blocks), dim3(256), 0, st, s2, q2, m2, npairs, (double)n);
    else
        hipLaunchKernelGGL(k_accum_add<false>, dim3((unsigned)blocks), dim3(256), 0, st, s2, q2, m2, npairs, (double)n);
    return hipGetLastError();
}

hipError_t launch_accum_resolve(const double* S, const double* Q, long npix, int64_t N, int64_t K, double* sub,
                                float* var, hipStream_t st) {
    if (npix <= 0 || (!sub && !var)) return hipSuccess;
    const long blocks = (npix + 255) / 256;
    hipLaunchKernelGGL(k_accum_resolve, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const double2*>(S),
                       reinterpret_cast<const double2*>(Q), npix, (double)N, (double)(K - 1),
                       reinterpret_cast<double2*>(sub), reinterpret_cast<float4*>(var));
    return hipGetLastError();
}

hipError_t launch_accum_resolve_cnt(const double* S, const double* Q, const uint32_t* cnt, long npix, double* sub,
                                    float* var, hipStream_t st) {
    if (npix <= 0 || (!sub && !var)) return hipSuccess;
    const long blocks = (npix + 255) / 256;
    hipLaunchKernelGGL(k_accum_resolve_cnt, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const double2*>(S),
                       reinterpret_cast<const double2*>(Q), reinterpret_cast<const uint2*>(cnt), npix,
                       reinterpret_cast<double2*>(sub), reinterpret_cast<float4*>(var));
    return hipGetLastError();
}

}  // namespace rt
