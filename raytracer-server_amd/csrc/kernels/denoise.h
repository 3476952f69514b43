// Denoised previews: first-hit feature buffers and the edge-avoiding a-trous filter.
// Launchers of denoise.hip, called by api/denoise.cpp (rt_render_features*, rt_denoise*).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../device/scene_layout.h"

namespace rt {

// k_features_f64: the tile of rt_render_params and the camera frame (server.rs:330-331, host-computed).
struct FeatArgs {
    int32_t width, height, x0, y0, tw, th;
    int32_t row_step;  // tile row i = screen row y0 + i * row_step
    int32_t nearest;   // RT_FLAG_MESH_NEAREST
    double cx[3], cy[3];
};

// One level of the filter. The level's step s = 2^i splits the image into min(s, width) x min(s, height)
// sub-lattices {(la + s u, lb + s v)}; a block filters a 16 x 16 patch of one of them.
struct AtrousArgs {
    int32_t width, height, step;
    int32_t nlx, nly;          // sub-lattices per axis
    int32_t tiles_x, tiles_y;  // 16 x 16 patches per sub-lattice (of the largest one; the others skip the excess)
    float inv_c, inv_n, inv_z, inv_a;  // 1 / sigma^2 of each term of E (colour: 1 / (sigma_c 2^-i)^2); 0 drops the term
};

constexpr int kFeatFloats = 8;  // feat[pix][8]: mean normal, mean t, mean albedo, coverage

// feat[tw * th][8] on the device.
hipError_t launch_features_f64(const DevScene& sc, const FeatArgs& a, float* feat, hipStream_t st);
// Scratch floats of launch_atrous (two colour images of float4 per pixel).
size_t atrous_scratch_bytes(long npix);
// The filter on device buffers: sub[pix][4][3] f64, feat[pix][8] f32 -> lin[pix][3] f32 (nullable) and
// rgb[pix][3] u8 (nullable; levels = 0 callers make the RGB8 with launch_finalize_f64 instead).
// sigma <= 0 drops its term. scratch: atrous_scratch_bytes(width * height) bytes, 16-byte aligned.
hipError_t launch_atrous(int width, int height, const double* sub, const float* feat, int levels, float sigma_c,
                         float sigma_n, float sigma_z, float sigma_a, void* scratch, uint8_t* rgb, float* lin,
                         hipStream_t st);

// The variance-guided filter (rt_denoise_var*): launch_atrous with var[pix][4] f32 (only [3] is read)
// scaling the colour term, and the filtered variance vout[pix] f32 (nullable). The same scratch: the variance rides
// in the colour entries' fourth component. AtrousArgs::inv_c carries sigma_c^2 here (0 drops the colour term).
hipError_t launch_atrous_var(int width, int height, const double* sub, const float* feat, const float* var,
                             int levels, float sigma_c, float sigma_n, float sigma_z, float sigma_a, void* scratch,
                             uint8_t* rgb, float* lin, float* vout, hipStream_t st);

}  // namespace rt
