// C ABI (include/rt_ffi.h): denoised previews — first-hit feature buffers, the à-trous filter and its
// variance-guided form.
#include <cmath>

#include "../kernels/denoise.h"
#include "api_common.hpp"

using namespace rt::api;

namespace {

int check_features(const char* who, const rt_scene* scene, const rt_render_params* p, const void* out) {
    if (!scene || !p || !out) return fail(RT_E_INVAL, std::string(who) + ": null argument");
    return check_params(p);
}

int check_denoise(const char* who, int32_t width, int32_t height, const void* sub, const void* feat, int32_t levels,
                  const float sigma[4], const void* rgb_out) {
    if (!sub || !feat || !rgb_out) return fail(RT_E_INVAL, std::string(who) + ": null argument");
    if (width < 1 || height < 1) return fail(RT_E_INVAL, std::string(who) + ": width/height must be positive");
    if ((int64_t)width * height > (int64_t)INT32_MAX) return fail(RT_E_INVAL, std::string(who) + ": image too large");
    if (levels < 0 || levels > 8) return fail(RT_E_INVAL, std::string(who) + ": levels must be in 0..8");
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(sigma[i])) return fail(RT_E_INVAL, std::string(who) + ": sigma must be finite");
    return RT_OK;
}

// The checks that open the four filter entry points (rt_denoise*: `var` is checked by the two that take one), and
// the device selected.
int denoise_begin(const char* who, int32_t device, int32_t width, int32_t height, const void* sub, const void* feat,
                  int32_t levels, const float sigma[4], const void* rgb_out) {
    int rc = check_denoise(who, width, height, sub, feat, levels, sigma, rgb_out);
    if (rc == RT_OK) rc = need_device(who, device);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    return RT_OK;
}

// Enqueues the filter on `st` and waits for it, so its scratch is idle again when the call returns. With d_var
// (rt_denoise_var*) the variance-guided filter runs, and d_vout may ask for the filtered variance.
int denoise_run(const char* who, int32_t device, int32_t width, int32_t height, const double* d_sub,
                const float* d_feat, const float* d_var, int32_t levels, const float sigma[4], uint8_t* d_rgb,
                float* d_lin, float* d_vout, hipStream_t st) {
    const long npix = (long)width * height;
    hipError_t e = hipSuccess;
    if (levels == 0) {
        // the pass-through: the RGB8 is rt_render's own; only a linear or a variance output still needs the filter
        e = finalize_rgb(width, height, d_sub, d_rgb, st);
        if (e == hipSuccess && !d_lin && !d_vout) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
        if (!d_lin && !d_vout) return RT_OK;
    }
    const size_t bytes = rt::atrous_scratch_bytes(npix);
    void* scratch = scratch_take(device, bytes, &e);
    if (!scratch) return oom_or_hip(e, std::string(who) + " scratch");
    uint8_t* rgb = levels == 0 ? nullptr : d_rgb;
    e = d_var ? rt::launch_atrous_var(width, height, d_sub, d_feat, d_var, levels, sigma[0], sigma[1], sigma[2],
                                      sigma[3], scratch, rgb, d_lin, d_vout, st)
              : rt::launch_atrous(width, height, d_sub, d_feat, levels, sigma[0], sigma[1], sigma[2], sigma[3], scratch,
                                  rgb, d_lin, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    scratch_give(device, scratch, bytes);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return RT_OK;
}

// The host form of the filter (rt_denoise, and with `var` rt_denoise_var): uploads into one block, runs the filter on
// a stream of the call's own, and copies back the outputs asked for. Arguments checked by denoise_begin.
int denoise_host(const char* who, int32_t device, int32_t width, int32_t height, const double* sub, const float* feat,
                 const float* var, int32_t levels, const float sigma[4], uint8_t* rgb_out, float* lin_out,
                 float* var_out) {
    const size_t npix = (size_t)width * height;
    const size_t b_sub = npix * 12 * sizeof(double), b_feat = npix * rt::kFeatFloats * sizeof(float);
    const size_t b_var = npix * 4 * sizeof(float), b_lin = npix * 3 * sizeof(float), b_vout = npix * sizeof(float);
    DeviceBlock buf;
    const size_t at_sub = buf.part(b_sub), at_feat = buf.part(b_feat), at_var = buf.part(var ? b_var : 0);
    const size_t at_lin = buf.part(lin_out ? b_lin : 0), at_vout = buf.part(var_out ? b_vout : 0), at_rgb = buf.part(npix * 3);
    hipError_t e = buf.alloc();
    if (e != hipSuccess) return oom_or_hip(e, std::string(who) + " buffers");
    double* d_sub = buf.at<double>(at_sub);
    float* d_feat = buf.at<float>(at_feat);
    float* d_var = var ? buf.at<float>(at_var) : nullptr;
    float* d_lin = lin_out ? buf.at<float>(at_lin) : nullptr;
    float* d_vout = var_out ? buf.at<float>(at_vout) : nullptr;
    uint8_t* d_rgb = buf.at<uint8_t>(at_rgb);
    CallStream cs;
    e = cs.init();
    if (e == hipSuccess) e = hipMemcpyAsync(d_sub, sub, b_sub, hipMemcpyHostToDevice, cs.st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_feat, feat, b_feat, hipMemcpyHostToDevice, cs.st);
    if (e == hipSuccess && var) e = hipMemcpyAsync(d_var, var, b_var, hipMemcpyHostToDevice, cs.st);
    if (e == hipSuccess) {
        const int rc = denoise_run(who, device, width, height, d_sub, d_feat, d_var, levels, sigma, d_rgb, d_lin, d_vout, cs.st);
        if (rc != RT_OK) return rc;
        e = hipMemcpyAsync(rgb_out, d_rgb, npix * 3, hipMemcpyDeviceToHost, cs.st);
    }
    if (e == hipSuccess && lin_out) e = hipMemcpyAsync(lin_out, d_lin, b_lin, hipMemcpyDeviceToHost, cs.st);
    if (e == hipSuccess && var_out) e = hipMemcpyAsync(var_out, d_vout, b_vout, hipMemcpyDeviceToHost, cs.st);
    if (e == hipSuccess) e = cs.close();
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return RT_OK;
}

}  // namespace

namespace rt::api {

int features_enqueue(rt_scene* s, const rt_render_params* p, float* d_feat, hipStream_t st) {
    HIP_TRY(hipSetDevice(p->device));
    rt::DevScene ds;
    const int rc = upload(s, p->device, &ds);
    if (rc != RT_OK) return rc;
    rt::FeatArgs a{};
    a.width = p->width;
    a.height = p->height;
    a.x0 = p->x0;
    a.y0 = p->y0;
    a.tw = p->tile_w;
    a.th = p->tile_h;
    a.row_step = p->row_step > 1 ? p->row_step : 1;
    a.nearest = (p->flags & RT_FLAG_MESH_NEAREST) && !s->host.meshes.empty();
    rt::host::camera_frame(s->cam_dir, s->cam_right, s->cam_fov, p->width, p->height, a.cx, a.cy);
    HIP_TRY(rt::launch_features_f64(ds, a, d_feat, st));
    return RT_OK;
}

}  // namespace rt::api

extern "C" {

int rt_render_features_device(const rt_scene* scene, const rt_render_params* params, void* d_feat, void* stream) {
    int rc = check_features("rt_render_features_device", scene, params, d_feat);
    if (rc == RT_OK) rc = need_device("rt_render_features_device", params->device);
    if (rc != RT_OK) return rc;
    return features_enqueue(const_cast<rt_scene*>(scene), params, (float*)d_feat, (hipStream_t)stream);
}

int rt_render_features(const rt_scene* scene, const rt_render_params* p, float* feat_out) {
    int rc = check_features("rt_render_features", scene, p, feat_out);
    if (rc == RT_OK) rc = need_device("rt_render_features", p->device);
    if (rc != RT_OK) return rc;
    const size_t bytes = (size_t)p->tile_w * p->tile_h * rt::kFeatFloats * sizeof(float);
    if (bytes == 0) return RT_OK;
    HIP_TRY(hipSetDevice(p->device));
    DeviceBlock buf;
    buf.part(bytes);
    hipError_t e = buf.alloc();
    if (e != hipSuccess) return oom_or_hip(e, "rt_render_features buffer");
    float* d_feat = buf.at<float>(0);
    rc = features_enqueue(const_cast<rt_scene*>(scene), p, d_feat, nullptr);
    e = hipStreamSynchronize(nullptr);  // also after a failed enqueue: what it did enqueue is drained
    if (rc != RT_OK) return rc;
    if (e == hipSuccess) e = hipMemcpy(feat_out, d_feat, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_render_features: ") + hipGetErrorString(e));
    return RT_OK;
}

int rt_denoise_device(int32_t device, int32_t width, int32_t height, const double* sub, const float* feat,
                      int32_t levels, float sigma_c, float sigma_n, float sigma_z, float sigma_a, uint8_t* rgb_out,
                      float* lin_out, void* stream) {
    const float sigma[4] = {sigma_c, sigma_n, sigma_z, sigma_a};
    const int rc = denoise_begin("rt_denoise_device", device, width, height, sub, feat, levels, sigma, rgb_out);
    if (rc != RT_OK) return rc;
    return denoise_run("rt_denoise_device", device, width, height, sub, feat, nullptr, levels, sigma, rgb_out, lin_out,
                       nullptr, (hipStream_t)stream);
}

int rt_denoise(int32_t device, int32_t width, int32_t height, const double* sub, const float* feat, int32_t levels,
               float sigma_c, float sigma_n, float sigma_z, float sigma_a, uint8_t* rgb_out, float* lin_out) {
    const float sigma[4] = {sigma_c, sigma_n, sigma_z, sigma_a};
    const int rc = denoise_begin("rt_denoise", device, width, height, sub, feat, levels, sigma, rgb_out);
    if (rc != RT_OK) return rc;
    return denoise_host("rt_denoise", device, width, height, sub, feat, nullptr, levels, sigma, rgb_out, lin_out, nullptr);
}

int rt_denoise_var_device(int32_t device, int32_t width, int32_t height, const double* sub, const float* feat,
                          const float* var, int32_t levels, float sigma_c, float sigma_n, float sigma_z,
                          float sigma_a, uint8_t* rgb_out, float* lin_out, float* var_out, void* stream) {
    const float sigma[4] = {sigma_c, sigma_n, sigma_z, sigma_a};
    if (!var) return fail(RT_E_INVAL, "rt_denoise_var_device: null argument");
    const int rc = denoise_begin("rt_denoise_var_device", device, width, height, sub, feat, levels, sigma, rgb_out);
    if (rc != RT_OK) return rc;
    return denoise_run("rt_denoise_var_device", device, width, height, sub, feat, var, levels, sigma, rgb_out, lin_out,
                       var_out, (hipStream_t)stream);
}

int rt_denoise_var(int32_t device, int32_t width, int32_t height, const double* sub, const float* feat,
                   const float* var, int32_t levels, float sigma_c, float sigma_n, float sigma_z, float sigma_a,
                   uint8_t* rgb_out, float* lin_out, float* var_out) {
    const float sigma[4] = {sigma_c, sigma_n, sigma_z, sigma_a};
    if (!var) return fail(RT_E_INVAL, "rt_denoise_var: null argument");
    const int rc = denoise_begin("rt_denoise_var", device, width, height, sub, feat, levels, sigma, rgb_out);
    if (rc != RT_OK) return rc;
    return denoise_host("rt_denoise_var", device, width, height, sub, feat, var, levels, sigma, rgb_out, lin_out, var_out);
}

}  // extern "C"
