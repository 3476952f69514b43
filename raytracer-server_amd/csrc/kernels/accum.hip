// Progressive accumulation for gfx950.
//
//   k_accum_add     — merges one pass's subpixel means into the two f64 sums S = sum n m, Q = sum n m^2.
//   k_accum_resolve — the accumulated subpixel means S / N and the variance of the clamped pixel colour.
// Both stream: every access is a 16-byte load or store of consecutive lanes. Compiled without FMA contraction (the
// Makefile's -ffp-contract=off), so tests/accum_ref.py restates them bit for bit.
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

// One lane per pixel. K1 = K - 1 (unused when var is null).
__global__ __launch_bounds__(256) void k_accum_resolve(const double2* __restrict__ S, const double2* __restrict__ Q,
                                                       long npix, double N, double K1, double2* __restrict__ sub,
                                                       float4* __restrict__ var) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
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

}  // namespace rt
