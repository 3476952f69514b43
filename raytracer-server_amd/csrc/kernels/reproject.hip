// Accumulator reprojection across camera moves for gfx950.
//
//   k_reproject_f64 — seeds accumulator dst (the new view) from accumulator src (the old view): per dst subpixel the
//                     tent-centre camera ray's first hit is projected into the src frame, validated by
//                     mutually_visible from the hit point to the src camera, and the nearest src subpixel's sums are
//                     rescaled to the history length the pixel inherits.
// The definition is in include/rt_ffi.h (rt_accum_reproject), operation by operation; tests/reproject_ref.py restates
// it. Compiled without FMA contraction (the Makefile's -ffp-contract=off), so numpy gives the same bits.
#include <hip/hip_runtime.h>

#include "../device/integrator_f64.h"
#include "reproject.h"

namespace rt {
using namespace f64;

// One lane per dst subpixel, in rt_render's subpixel order (subpixel_of): lanes 4 p .. 4 p + 3 are dst pixel p, so a
// pixel's quad sits in one wave and its AND / min go through __shfl_xor. Every lane of a wave reaches the shuffles
// (the subpixel count is a multiple of 4, blocks of 256). F: the Cfg choice of k_trace_f64 / k_features_f64.
template <int F>
__global__ __launch_bounds__(256) void k_reproject_f64(DevScene sc, ReprojArgs ra) {
    using C = Cfg<F>;
    const long nsub = (long)ra.width * ra.height * 4;
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = p < nsub;
    bool ok = live;
    size_t src_at = 0;       // the source subpixel's first double: (q * 4 + j') * 3
    uint32_t Kq = 0, Nq = 0;  // the source pixel's counts
    if (live) {
        RenderArgs a{};
        a.width = ra.width;
        a.height = ra.height;
        a.tw = ra.width;
        a.th = ra.height;
        a.row_step = 1;
        const SubPixel sp = subpixel_of(a, p);
        const double w = (double)ra.width, h = (double)ra.height;
        // step 1: the dst view's tent-centre ray (u1 = u2 = 0.5) and its first hit
        const Ray r = camera_ray(sc, ld3(ra.cx), ld3(ra.cy), w, h, sp.col, sp.yref, sp.sx, sp.sy, 0.5, 0.5);
        const HitRec hr = trace_closest<C>(sc, r);
        // step 2: only a diffuse surface's outgoing radiance is the same from both cameras
        ok = hr.obj >= 0 && sc.objects[hr.obj].brdf == BRDF_DIFFUSE;
        V3 x = v3(0, 0, 0), n = v3(0, 0, 0);
        const V3 pos_s = ld3(ra.pos_s);
        if (ok) {
            surface<Cfg<1>>(sc, r, hr, &x, &n);
            // steps 3, 4: the hit point in the src frame; the comparisons are written so that NaN fails them, and
            // nothing is converted to an integer before they pass
            const V3 v = x - pos_s;
            const double al = dot(v, ld3(ra.A)), be = dot(v, ld3(ra.B)), ga = dot(v, ld3(ra.C));
            ok = ga > 0.;
            const double fx = (al / ga + 0.5) * w, fy = (be / ga + 0.5) * h;
            ok = ok && fx >= 0. && fx < w && fy >= 0. && fy < h;
            if (ok) {
                const double fcol = floor(fx), fyr = floor(fy);
                const int col = (int)fcol, yref = (int)fyr;
                const int sx = (int)floor((fx - fcol) * 2.), sy = (int)floor((fy - fyr) * 2.);
                const int row = ra.height - 1 - yref;
                // col in [0, w), yref in [0, h), sx, sy in {0, 1} by the comparisons above; checked again as
                // integers so that no gather can leave the buffers
                ok = col >= 0 && col < ra.width && row >= 0 && row < ra.height && (sx | sy) >= 0 && (sx | sy) <= 1;
                const size_t q = (size_t)row * (size_t)ra.width + (size_t)col;
                src_at = (q * 4 + (size_t)(2 * sy + sx)) * 3;
                if (ok) {
                    if (ra.cnt_src) {
                        const uint2 c = reinterpret_cast<const uint2*>(ra.cnt_src)[q];
                        Kq = c.x;
                        Nq = c.y;
                    } else {
                        Kq = ra.K_src;
                        Nq = ra.N_src;
                    }
                    ok = Nq > 0u;  // (every N_q >= 2 after src's two full-frame passes)
                }
            }
            // step 5: the src camera is on the side of the surface the dst camera sees
            if (ok) ok = dot(n, pos_s - x) > 0.;
            // step 6: Scene::mutually_visible from the hit point to the src camera; only lanes still valid ask
            if (ok) ok = visible<C>(sc, x, pos_s);
        }
    }
    // the quad: valid iff all four are; N_p and K_p from the four source pixels
    const int ok_i = ok ? 1 : 0;
    const int ok2 = ok_i & __shfl_xor(ok_i, 1);
    const bool valid = (ok2 & __shfl_xor(ok2, 2)) != 0;
    uint32_t n_min = ok ? Nq : 0xFFFFFFFFu;
    n_min = min(n_min, (uint32_t)__shfl_xor((int)n_min, 1));
    n_min = min(n_min, (uint32_t)__shfl_xor((int)n_min, 2));
    const uint32_t Np = valid ? min((uint32_t)ra.max_n, n_min) : 0u;
    // ceil(K_q N_p / N_q) in 64-bit integers
    uint32_t k_j = 0xFFFFFFFFu;
    if (valid) k_j = (uint32_t)(((uint64_t)Kq * (uint64_t)Np + (uint64_t)Nq - 1ull) / (uint64_t)Nq);
    k_j = min(k_j, (uint32_t)__shfl_xor((int)k_j, 1));
    k_j = min(k_j, (uint32_t)__shfl_xor((int)k_j, 2));
    const uint32_t Kp = valid ? max(2u, k_j) : 0u;
    if (live) {
        double s[3] = {0., 0., 0.}, q[3] = {0., 0., 0.};
        if (valid) {
            const double np_d = (double)Np, nq_d = (double)Nq;
#pragma unroll
            for (int c = 0; c < 3; ++c) {  // dividing first keeps the subpixel mean and Q / N - m m
                s[c] = np_d * (ra.S_src[src_at + c] / nq_d);
                q[c] = np_d * (ra.Q_src[src_at + c] / nq_d);
            }
        }
        // the quad's 96-byte S and Q rows: four lanes, 24 consecutive bytes each
        double* so = ra.S_dst + (size_t)p * 3;
        double* qo = ra.Q_dst + (size_t)p * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            so[c] = s[c];
            qo[c] = q[c];
        }
        if ((p & 3) == 0) reinterpret_cast<uint2*>(ra.cnt_dst)[p >> 2] = make_uint2(Kp, Np);
    }
    // valid pixels: one count per quad, a ballot per wave, one vector atomic per wave (an integer: order-free)
    const unsigned long long mk = __ballot(live && valid && (p & 3) == 0);
    if ((threadIdx.x & 63) == 0 && mk != 0ull) atomicAdd(ra.n_valid, (unsigned long long)__popcll(mk));
}

hipError_t launch_reproject_f64(const DevScene& sc, const ReprojArgs& a, hipStream_t st) {
    const long nsub = (long)a.width * a.height * 4;
    if (nsub <= 0) return hipSuccess;
    if (a.max_n < 1 || !a.S_src || !a.Q_src || !a.S_dst || !a.Q_dst || !a.cnt_dst || !a.n_valid)
        return hipErrorInvalidValue;
    const long blocks = (nsub + 255) / 256;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    const int cfg = (sc.compact ? 1 : 0) | (a.nearest ? 2 : 0);
    switch (cfg) {  // one kernel per instance: each holds one copy of the walks
        case 0: hipLaunchKernelGGL(k_reproject_f64<1>, grid, block, 0, st, sc, a); break;
        case 1: hipLaunchKernelGGL(k_reproject_f64<9>, grid, block, 0, st, sc, a); break;
        case 2: hipLaunchKernelGGL(k_reproject_f64<17>, grid, block, 0, st, sc, a); break;
        default: hipLaunchKernelGGL(k_reproject_f64<25>, grid, block, 0, st, sc, a); break;
    }
    return hipGetLastError();
}

}  // namespace rt
