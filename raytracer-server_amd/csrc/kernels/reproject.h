// Accumulator reprojection across camera moves: the launcher of reproject.hip, called by
// api/accum.cpp (rt_accum_reproject). The definition, operation by operation, is in include/rt_ffi.h;
// tests/reproject_ref.py restates it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../device/scene_layout.h"

namespace rt {

// k_reproject_f64's own argument block (DevScene and RenderArgs keep their layouts). The DevScene passed beside it
// carries the dst view's camera.
struct ReprojArgs {
    int32_t width, height;
    int32_t nearest;       // RT_FLAG_MESH_NEAREST on a scene with meshes
    int32_t max_n;         // >= 1
    double cx[3], cy[3];   // the dst view's camera frame at width x height
    double pos_s[3];       // the src view's camera position
    double A[3], B[3], C[3];  // rows of the inverse of the src frame (cx_s | cy_s | dir_s), host-computed
    const double* S_src;   // [pix][4][3]
    const double* Q_src;
    const uint32_t* cnt_src;  // [pix][2] = (K_q, N_q), or null: every source pixel holds (K_src, N_src)
    uint32_t K_src, N_src;
    double* S_dst;
    double* Q_dst;
    uint32_t* cnt_dst;     // [pix][2], every entry written
    unsigned long long* n_valid;  // device counter, zeroed by the caller
};

hipError_t launch_reproject_f64(const DevScene& sc, const ReprojArgs& a, hipStream_t st);

}  // namespace rt
