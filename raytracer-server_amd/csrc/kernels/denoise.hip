// Denoised previews for gfx950.
//
//   k_features_f64 — first-hit feature buffers: the four tent-centre camera rays of a pixel (one lane per
//                    subpixel) through trace_closest / surface, reduced per pixel to 8 floats.
//   k_atrous_*     — edge-avoiding a-trous wavelet filter over the subpixel means, guided by the features.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../device/integrator_f64.h"
#include "denoise.h"

namespace rt {
using namespace f64;

// (s0 + s1) + (s2 + s3) over the four consecutive lanes of a pixel, in every lane of the quad.
RT_DEV double quad_sum(double v) {
    const double a = v + __shfl_xor(v, 1);  // even lane: s_e + s_o, odd lane: s_o + s_e (the same bits)
    return a + __shfl_xor(a, 2);
}

// One lane per subpixel, in rt_render's subpixel order (subpixel_of): lanes 4 p .. 4 p + 3 are tile pixel p.
// Every lane of a wave reaches the reduction (the tile's subpixel count is a multiple of 4, blocks of 256).
__global__ __launch_bounds__(256) void k_features_f64(DevScene sc, FeatArgs fa, float* __restrict__ feat) {
    const long nsub = (long)fa.tw * fa.th * 4;
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = p < nsub;
    V3 n = v3(0, 0, 0), alb = v3(0, 0, 0);
    double t = 0.0, hit = 0.0;
    if (live) {
        RenderArgs a{};
        a.width = fa.width;
        a.height = fa.height;
        a.x0 = fa.x0;
        a.y0 = fa.y0;
        a.tw = fa.tw;
        a.th = fa.th;
        a.row_step = fa.row_step;
        const SubPixel sp = subpixel_of(a, p);
        // u1 = u2 = 0.5: the tent filter's centre (r = 1, so the offset is 1 - sqrt(1) = 0)
        const Ray r = camera_ray(sc, ld3(fa.cx), ld3(fa.cy), (double)fa.width, (double)fa.height, sp.col, sp.yref,
                                 sp.sx, sp.sy, 0.5, 0.5);
        // the Cfg choice of k_trace_f64
        const HitRec h = fa.nearest ? (sc.compact ? trace_closest<Cfg<25>>(sc, r) : trace_closest<Cfg<17>>(sc, r))
                                    : (sc.compact ? trace_closest<Cfg<9>>(sc, r) : trace_closest<Cfg<1>>(sc, r));
        if (h.obj >= 0) {
            V3 pos;
            surface<Cfg<1>>(sc, r, h, &pos, &n);
            const DevObject& o = sc.objects[h.obj];
            const V3 base = o.brdf == BRDF_PHONG ? ld3(o.color_d) * o.ph_kd + ld3(o.color_s) * o.ph_ks : ld3(o.k);
            alb = clampv(base + ld3(o.emitted), 0., 1.);
            t = h.t;
            hit = 1.0;
        }
    }
    const double hits = quad_sum(hit);
    const double sn[3] = {quad_sum(n.x), quad_sum(n.y), quad_sum(n.z)};
    const double st = quad_sum(t);
    const double sa[3] = {quad_sum(alb.x), quad_sum(alb.y), quad_sum(alb.z)};
    if (live && (p & 3) == 0) {
        // means over the rays that hit (the sums are 0 when none did)
        const double d = hits > 0. ? hits : 1.0;
        float4* o = reinterpret_cast<float4*>(feat + (size_t)(p >> 2) * kFeatFloats);
        o[0] = make_float4((float)(sn[0] / d), (float)(sn[1] / d), (float)(sn[2] / d), (float)(st / d));
        o[1] = make_float4((float)(sa[0] / d), (float)(sa[1] / d), (float)(sa[2] / d), (float)(hits * 0.25));
    }
}

hipError_t launch_features_f64(const DevScene& sc, const FeatArgs& a, float* feat, hipStream_t st) {
    const long nsub = (long)a.tw * a.th * 4;
    if (nsub <= 0) return hipSuccess;
    const long blocks = (nsub + 255) / 256;
    hipLaunchKernelGGL(k_features_f64, dim3((unsigned)blocks), dim3(256), 0, st, sc, a, feat);
    return hipGetLastError();
}

// c0 = sum_j clamp(sub_j, 0, 1) * 0.25 in f64 (k_finalize_f64's sum, server.rs:360), rounded to f32.
__global__ __launch_bounds__(256) void k_atrous_init(const double2* __restrict__ sub, float4* __restrict__ c0,
                                                     long npix) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const double2* s = sub + (size_t)p * 6;  // 12 doubles: [4][3]
    double v[12];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double2 d = s[k];
        v[2 * k] = d.x;
        v[2 * k + 1] = d.y;
    }
    V3 pixel = v3(0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) pixel = pixel + clampv(v3(v[3 * j], v[3 * j + 1], v[3 * j + 2]), 0., 1.) * 0.25;
    c0[p] = make_float4((float)pixel.x, (float)pixel.y, (float)pixel.z, 0.f);
}

// One level. A block takes a 16 x 16 patch of one sub-lattice and stages the 20 x 20 patch with its halo in LDS as
// three planes of 16-byte entries (colour + validity, feat[0..3], feat[4..7]); each global access is a 16-byte load
// or store, each LDS read a ds_read_b128.
// Row pitch: a ds_read_b128 is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, ... (lanes of two patch
// rows), one 256-byte bank row (sixteen 16-byte slots) per group and cycle. Lane (ty, tx) reads entry
// (ty + dy) * pitch + tx + dx, so a group's slots are {0-3, 12-15} and pitch + {4-11} (mod 16, plus a common
// offset): distinct only when pitch = 0 (mod 16). The 20 entries of a row therefore sit in a pitch of 32.
constexpr int kPatch = 16, kHalo = 2, kStage = kPatch + 2 * kHalo, kPitch = 32;

__global__ __launch_bounds__(256) void k_atrous_level(AtrousArgs a, const float4* __restrict__ cin,
                                                      const float4* __restrict__ feat, float4* __restrict__ cout) {
    __shared__ float4 s_c[kStage * kPitch];
    __shared__ float4 s_f0[kStage * kPitch];
    __shared__ float4 s_f1[kStage * kPitch];
    unsigned b = blockIdx.x;
    const int tile_x = (int)(b % (unsigned)a.tiles_x);
    b /= (unsigned)a.tiles_x;
    const int la = (int)(b % (unsigned)a.nlx);
    b /= (unsigned)a.nlx;
    const int tile_y = (int)(b % (unsigned)a.tiles_y);
    const int lb = (int)(b / (unsigned)a.tiles_y);
    const int s = a.step;
    // this sub-lattice: pixels (la + s u, lb + s v), u < wl, v < hl
    const int wl = (a.width - la + s - 1) / s, hl = (a.height - lb + s - 1) / s;
    const int u0 = tile_x * kPatch, v0 = tile_y * kPatch;
    if (u0 >= wl || v0 >= hl) return;  // uniform: a smaller sub-lattice has fewer patches

    for (int e = threadIdx.x; e < kStage * kStage; e += 256) {
        const int ly = e / kStage, lx = e - ly * kStage;
        const int u = u0 - kHalo + lx, v = v0 - kHalo + ly;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f), f0 = c, f1 = c;  // a tap outside the image: weight 0 (c.w)
        if (u >= 0 && v >= 0 && u < wl && v < hl) {
            const size_t pix = (size_t)(lb + (long)s * v) * (size_t)a.width + (size_t)(la + (long)s * u);
            c = cin[pix];
            c.w = 1.f;
            f0 = feat[2 * pix];
            f1 = feat[2 * pix + 1];
        }
        s_c[ly * kPitch + lx] = c;
        s_f0[ly * kPitch + lx] = f0;
        s_f1[ly * kPitch + lx] = f1;
    }
    __syncthreads();

    const int tx = threadIdx.x & (kPatch - 1), ty = threadIdx.x >> 4;
    if (u0 + tx >= wl || v0 + ty >= hl) return;
    const int ctr = (ty + kHalo) * kPitch + tx + kHalo;
    const float4 cp = s_c[ctr], p0 = s_f0[ctr], p1 = s_f1[ctr];
    const float hw[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
            const int q = (ty + dy) * kPitch + tx + dx;
            const float4 cq = s_c[q], q0 = s_f0[q], q1 = s_f1[q];
            const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
            const float nx = p0.x - q0.x, ny = p0.y - q0.y, nz = p0.z - q0.z;
            const float rz = (p0.w - q0.w) / (p0.w + q0.w + 1e-20f);
            const float ax = p1.x - q1.x, ay = p1.y - q1.y, az = p1.z - q1.z, ak = p1.w - q1.w;
            const float E = (dr * dr + dg * dg + db * db) * a.inv_c + (nx * nx + ny * ny + nz * nz) * a.inv_n +
                            rz * rz * a.inv_z + (ax * ax + ay * ay + az * az + ak * ak) * a.inv_a;
            const float w = hw[dx] * hw[dy] * expf(-E) * cq.w;
            sw += w;
            sr += w * cq.x;
            sg += w * cq.y;
            sb += w * cq.z;
        }
    }
    const size_t pix = (size_t)(lb + (long)s * (v0 + ty)) * (size_t)a.width + (size_t)(la + (long)s * (u0 + tx));
    cout[pix] = make_float4(sr / sw, sg / sw, sb / sw, 0.f);  // the centre tap has E = 0: sw >= 9/64
}

// Linear colour out, and RGB8 through k_finalize_f64's arithmetic (server.rs:366-368 gamma, :187-189 `as u8`).
__global__ __launch_bounds__(256) void k_atrous_out(const float4* __restrict__ c, long npix, uint8_t* __restrict__ rgb,
                                                    float* __restrict__ lin) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const float4 v = c[p];
    if (lin) {
        lin[p * 3 + 0] = v.x;
        lin[p * 3 + 1] = v.y;
        lin[p * 3 + 2] = v.z;
    }
    if (rgb) {
        const V3 cc = clampv(v3((double)v.x, (double)v.y, (double)v.z), 0., 1.);
        const double g = 1.0 / 2.2;
        const V3 gc = v3(pow(cc.x, g), pow(cc.y, g), pow(cc.z, g)) * 255.0 + v3(0.5, 0.5, 0.5);
        rgb[p * 3 + 0] = as_u8(gc.x);
        rgb[p * 3 + 1] = as_u8(gc.y);
        rgb[p * 3 + 2] = as_u8(gc.z);
    }
}

// The variance-guided filter -----------------------------------------------------------------
// The colour entries carry the pixel's variance in their fourth component (global scratch and LDS alike), so the
// scratch stays at 32 bytes per pixel and a tap's colour and variance come with one ds_read_b128.

// c0 as k_atrous_init; v0 = max(var[p][3], 0) (a negative or NaN input counts as 0: negative marks a tap outside the
// image in the level kernel's stage).
__global__ __launch_bounds__(256) void k_atrous_init_var(const double2* __restrict__ sub, const float4* __restrict__ var,
                                                         float4* __restrict__ c0, long npix) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const double2* s = sub + (size_t)p * 6;  // 12 doubles: [4][3]
    double v[12];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double2 d = s[k];
        v[2 * k] = d.x;
        v[2 * k + 1] = d.y;
    }
    V3 pixel = v3(0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) pixel = pixel + clampv(v3(v[3 * j], v[3 * j + 1], v[3 * j + 2]), 0., 1.) * 0.25;
    const float v0 = var[p].w;
    c0[p] = make_float4((float)pixel.x, (float)pixel.y, (float)pixel.z, v0 > 0.f ? v0 : 0.f);
}

// One level: k_atrous_level's patch, stage, planes, pitch and tap order. The colour plane's fourth component is the
// variance, -1 for a tap outside the image (weight 0). g_p, the 3 x 3 tent of the variance at the level's step, reads
// the stage at the centre +- 1: inside the halo of 2. a.inv_c is sigma_c^2 here (0: no colour term).
__global__ __launch_bounds__(256) void k_atrous_level_var(AtrousArgs a, const float4* __restrict__ cin,
                                                          const float4* __restrict__ feat, float4* __restrict__ cout) {
    __shared__ float4 s_c[kStage * kPitch];
    __shared__ float4 s_f0[kStage * kPitch];
    __shared__ float4 s_f1[kStage * kPitch];
    unsigned b = blockIdx.x;
    const int tile_x = (int)(b % (unsigned)a.tiles_x);
    b /= (unsigned)a.tiles_x;
    const int la = (int)(b % (unsigned)a.nlx);
    b /= (unsigned)a.nlx;
    const int tile_y = (int)(b % (unsigned)a.tiles_y);
    const int lb = (int)(b / (unsigned)a.tiles_y);
    const int s = a.step;
    const int wl = (a.width - la + s - 1) / s, hl = (a.height - lb + s - 1) / s;
    const int u0 = tile_x * kPatch, v0 = tile_y * kPatch;
    if (u0 >= wl || v0 >= hl) return;  // uniform: a smaller sub-lattice has fewer patches

    for (int e = threadIdx.x; e < kStage * kStage; e += 256) {
        const int ly = e / kStage, lx = e - ly * kStage;
        const int u = u0 - kHalo + lx, v = v0 - kHalo + ly;
        float4 c = make_float4(0.f, 0.f, 0.f, -1.f), f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
        if (u >= 0 && v >= 0 && u < wl && v < hl) {
            const size_t pix = (size_t)(lb + (long)s * v) * (size_t)a.width + (size_t)(la + (long)s * u);
            c = cin[pix];  // c.w >= 0 (k_atrous_init_var; a level's output is a ratio of non-negative sums)
            f0 = feat[2 * pix];
            f1 = feat[2 * pix + 1];
        }
        s_c[ly * kPitch + lx] = c;
        s_f0[ly * kPitch + lx] = f0;
        s_f1[ly * kPitch + lx] = f1;
    }
    __syncthreads();

    const int tx = threadIdx.x & (kPatch - 1), ty = threadIdx.x >> 4;
    if (u0 + tx >= wl || v0 + ty >= hl) return;
    const int ctr = (ty + kHalo) * kPitch + tx + kHalo;
    const float4 cp = s_c[ctr], p0 = s_f0[ctr], p1 = s_f1[ctr];
    const float hw[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
    const float kw[3] = {1.f / 4.f, 1.f / 2.f, 1.f / 4.f};
    float gs = 0.f, gw = 0.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float vq = s_c[ctr + (dy - 1) * kPitch + dx - 1].w;
            const float k = vq >= 0.f ? kw[dx] * kw[dy] : 0.f;
            gs += k * vq;
            gw += k;
        }
    }
    // the level's one reciprocal: the centre tap is inside, so gw >= 1/4
    const float inv_c = a.inv_c > 0.f ? 1.f / (a.inv_c * (gs / gw) + 1e-10f) : 0.f;
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
    // one row of taps at a time (the rows are not unrolled): five taps' entries in flight keep the kernel at
    // k_atrous_level's occupancy; unrolled over all 25 the compiler holds 174 VGPRs (2 waves per SIMD)
#pragma unroll 1
    for (int dy = 0; dy < 5; ++dy) {
        const float hy = (dy == 0 || dy == 4) ? 1.f / 16.f : dy == 2 ? 3.f / 8.f : 1.f / 4.f;  // hw[dy]
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
            const int q = (ty + dy) * kPitch + tx + dx;
            const float4 cq = s_c[q], q0 = s_f0[q], q1 = s_f1[q];
            const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
            const float nx = p0.x - q0.x, ny = p0.y - q0.y, nz = p0.z - q0.z;
            const float rz = (p0.w - q0.w) / (p0.w + q0.w + 1e-20f);
            const float ax = p1.x - q1.x, ay = p1.y - q1.y, az = p1.z - q1.z, ak = p1.w - q1.w;
            const float E = (dr * dr + dg * dg + db * db) * inv_c + (nx * nx + ny * ny + nz * nz) * a.inv_n +
                            rz * rz * a.inv_z + (ax * ax + ay * ay + az * az + ak * ak) * a.inv_a;
            const float w = cq.w >= 0.f ? hw[dx] * hy * expf(-E) : 0.f;
            sw += w;
            sr += w * cq.x;
            sg += w * cq.y;
            sb += w * cq.z;
            sv += (w * w) * cq.w;
        }
    }
    const size_t pix = (size_t)(lb + (long)s * (v0 + ty)) * (size_t)a.width + (size_t)(la + (long)s * (u0 + tx));
    cout[pix] = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));  // the centre tap has E = 0: sw >= 9/64
}

// The filtered variance out (the colour and RGB8 go through k_atrous_out).
__global__ __launch_bounds__(256) void k_atrous_var_out(const float4* __restrict__ c, long npix, float* __restrict__ vout) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < npix) vout[p] = c[p].w;
}

size_t atrous_scratch_bytes(long npix) { return (size_t)std::max(npix, 0L) * 2 * sizeof(float4); }

// 1 / sigma^2, finite (a zero difference times it stays 0, as 0 / sigma^2 is); sigma <= 0 drops the term
static float inv_sq(double sigma) { return sigma > 0. ? (float)std::min(1.0 / (sigma * sigma), 3.0e38) : 0.f; }

hipError_t launch_atrous(int width, int height, const double* sub, const float* feat, int levels, float sigma_c,
                         float sigma_n, float sigma_z, float sigma_a, void* scratch, uint8_t* rgb, float* lin,
                         hipStream_t st) {
    const long npix = (long)width * height;
    if (npix <= 0) return hipSuccess;
    float4* buf[2] = {static_cast<float4*>(scratch), static_cast<float4*>(scratch) + npix};
    const unsigned pblocks = (unsigned)((npix + 255) / 256);
    hipLaunchKernelGGL(k_atrous_init, dim3(pblocks), dim3(256), 0, st, reinterpret_cast<const double2*>(sub), buf[0],
                       npix);
    int cur = 0;
    for (int i = 0; i < levels; ++i) {
        AtrousArgs a{};
        a.width = width;
        a.height = height;
        a.step = 1 << i;
        a.nlx = std::min(a.step, width);
        a.nly = std::min(a.step, height);
        a.tiles_x = ((width + a.step - 1) / a.step + kPatch - 1) / kPatch;
        a.tiles_y = ((height + a.step - 1) / a.step + kPatch - 1) / kPatch;
        a.inv_c = inv_sq((double)sigma_c / (double)a.step);
        a.inv_n = inv_sq(sigma_n);
        a.inv_z = inv_sq(sigma_z);
        a.inv_a = inv_sq(sigma_a);
        const long blocks = (long)a.tiles_x * a.nlx * a.tiles_y * a.nly;
        if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_atrous_level, dim3((unsigned)blocks), dim3(256), 0, st, a, buf[cur],
                           reinterpret_cast<const float4*>(feat), buf[cur ^ 1]);
        cur ^= 1;
    }
    if (rgb || lin) hipLaunchKernelGGL(k_atrous_out, dim3(pblocks), dim3(256), 0, st, buf[cur], npix, rgb, lin);
    return hipGetLastError();
}

hipError_t launch_atrous_var(int width, int height, const double* sub, const float* feat, const float* var,
                             int levels, float sigma_c, float sigma_n, float sigma_z, float sigma_a, void* scratch,
                             uint8_t* rgb, float* lin, float* vout, hipStream_t st) {
    const long npix = (long)width * height;
    if (npix <= 0) return hipSuccess;
    float4* buf[2] = {static_cast<float4*>(scratch), static_cast<float4*>(scratch) + npix};
    const unsigned pblocks = (unsigned)((npix + 255) / 256);
    hipLaunchKernelGGL(k_atrous_init_var, dim3(pblocks), dim3(256), 0, st, reinterpret_cast<const double2*>(sub),
                       reinterpret_cast<const float4*>(var), buf[0], npix);
    int cur = 0;
    for (int i = 0; i < levels; ++i) {
        AtrousArgs a{};
        a.width = width;
        a.height = height;
        a.step = 1 << i;
        a.nlx = std::min(a.step, width);
        a.nly = std::min(a.step, height);
        a.tiles_x = ((width + a.step - 1) / a.step + kPatch - 1) / kPatch;
        a.tiles_y = ((height + a.step - 1) / a.step + kPatch - 1) / kPatch;
        // sigma_c^2, finite and not flushed to 0 (a tiny sigma_c still means "colour term on")
        a.inv_c = sigma_c > 0.f ? (float)std::min(std::max((double)sigma_c * (double)sigma_c, 1.2e-38), 3.0e38) : 0.f;
        a.inv_n = inv_sq(sigma_n);
        a.inv_z = inv_sq(sigma_z);
        a.inv_a = inv_sq(sigma_a);
        const long blocks = (long)a.tiles_x * a.nlx * a.tiles_y * a.nly;
        if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_atrous_level_var, dim3((unsigned)blocks), dim3(256), 0, st, a, buf[cur],
                           reinterpret_cast<const float4*>(feat), buf[cur ^ 1]);
        cur ^= 1;
    }
    if (rgb || lin) hipLaunchKernelGGL(k_atrous_out, dim3(pblocks), dim3(256), 0, st, buf[cur], npix, rgb, lin);
    if (vout) hipLaunchKernelGGL(k_atrous_var_out, dim3(pblocks), dim3(256), 0, st, buf[cur], npix, vout);
    return hipGetLastError();
}

}  // namespace rt
