// Progressive accumulation: launchers of accum.hip, called by rt_api.cpp (rt_accum_*).
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

}  // namespace rt
