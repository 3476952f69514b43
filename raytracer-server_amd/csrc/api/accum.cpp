// C ABI (include/rt_ffi.h): the accumulator — its buffers, full-frame merges, the resolve, the
// per-pixel counts — and its reprojection across camera moves.
#include "../kernels/reproject.h"
#include "accum_state.hpp"

using namespace rt::api;

namespace rt::api {

int accum_ready(const char* who, rt_accum* a, bool stage, bool adapt) {
    const int rc = need_device(who, a->device);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(a->device));
    hipError_t e = hipSuccess;
    if (!a->S) {
        e = hipMalloc((void**)&a->S, 2 * a->sub_bytes());
        if (e == hipSuccess) a->Q = a->S + a->npix() * 12;
        else a->S = nullptr;
    }
    if (e == hipSuccess && stage && !a->stage) {
        e = hipMalloc((void**)&a->stage, a->stage_bytes());
        if (e != hipSuccess) a->stage = nullptr;
    }
    if (e != hipSuccess) return oom_or_hip(e, "rt_accum buffers");
    if (adapt && !a->adapt) {
        e = hipMalloc((void**)&a->adapt, a->adapt_bytes());
        if (e != hipSuccess) {
            a->adapt = nullptr;
            return oom_or_hip(e, "rt_accum error-target buffers");
        }
    }
    return RT_OK;
}

int batch_ready(const char* who, rt_accum* a) {
    const int rc = accum_ready(who, a, true, true);
    if (rc != RT_OK) return rc;
    if (!a->batch) {
        const hipError_t e = hipMalloc((void**)&a->batch, a->batch_bytes());
        if (e != hipSuccess) {
            a->batch = nullptr;
            return oom_or_hip(e, "rt_accum batch buffers");
        }
    }
    return RT_OK;
}

int accum_merge(rt_accum* a, const double* d_sub, int32_t n, hipStream_t st) {
    hipError_t e = rt::launch_accum_add(a->S, a->Q, d_sub, (long)a->npix(), n, a->K == 0 && !a->seeded, st);
    if (e == hipSuccess && a->sparse) e = rt::launch_accum_cnt_fill(a->cnt(), (long)a->npix(), 1u, (uint32_t)n, true, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_accum merge: ") + hipGetErrorString(e));
    a->K += 1;
    a->N += n;
    return RT_OK;
}

int accum_merge_list(rt_accum* a, const uint32_t* d_pixels, int64_t n_pixels, const double* d_sub, int32_t n,
                     hipStream_t st, const uint8_t* d_counts, const uint32_t* d_off) {
    hipError_t e = hipSuccess;
    if (!a->sparse) e = rt::launch_accum_cnt_fill(a->cnt(), (long)a->npix(), (uint32_t)a->K, (uint32_t)a->N, false, st);
    if (e == hipSuccess)
        e = d_counts ? rt::launch_accum_add_runs(a->S, a->Q, a->cnt(), d_pixels, d_counts, d_off, (long)n_pixels, d_sub, n, st)
                     : rt::launch_accum_add_list(a->S, a->Q, a->cnt(), d_pixels, (long)n_pixels, d_sub, n, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess)
        return fail(RT_E_HIP, std::string(d_counts ? "rt_accum run merge: " : "rt_accum sparse merge: ") + hipGetErrorString(e));
    a->sparse = true;
    return RT_OK;
}

hipError_t accum_resolve_enqueue(rt_accum* a, double* d_sub, float* d_var, uint8_t* d_rgb, hipStream_t st) {
    hipError_t e = a->sparse ? rt::launch_accum_resolve_cnt(a->S, a->Q, a->cnt(), (long)a->npix(), d_sub, d_var, st)
                             : rt::launch_accum_resolve(a->S, a->Q, (long)a->npix(), a->N, a->K, d_sub, d_var, st);
    if (e == hipSuccess && d_rgb) e = finalize_rgb(a->width, a->height, d_sub, d_rgb, st);
    return e;
}

int check_accum_add(const rt_accum* a, const rt_scene* scene, const rt_render_params* p) {
    if (!a || !scene || !p) return fail(RT_E_INVAL, "rt_accum_add: null argument");
    if (p->width != a->width || p->height != a->height || p->x0 != 0 || p->y0 != 0 || p->tile_w != a->width ||
        p->tile_h != a->height)
        return fail(RT_E_INVAL, "rt_accum_add: params must be the accumulator's whole frame");
    if (p->row_step < 0 || p->row_step > 1) return fail(RT_E_INVAL, "rt_accum_add: row_step must be 0 or 1");
    if (p->spp < 4) return fail(RT_E_INVAL, "rt_accum_add: spp must be >= 4");
    if (p->device != a->device) return fail(RT_E_INVAL, "rt_accum_add: params->device is not the accumulator's device");
    return check_params(p);
}

int check_accum_sub(const char* who, const rt_accum* a, const void* sub, int32_t n) {
    if (!a || !sub) return fail(RT_E_INVAL, std::string(who) + ": null argument");
    if (n < 1) return fail(RT_E_INVAL, std::string(who) + ": n must be >= 1");
    return RT_OK;
}

int check_accum_resolve(const char* who, const rt_accum* a, const void* var) {
    if (!a) return fail(RT_E_INVAL, std::string(who) + ": null argument");
    if (a->covered) return RT_OK;  // every K_p >= 2 (rt_accum_fill)
    if (a->K < 1) return fail(RT_E_INVAL, std::string(who) + ": no pass accumulated");
    if (var && a->K < 2) return fail(RT_E_INVAL, std::string(who) + ": the variance needs at least two passes");
    return RT_OK;
}

int check_sparse(const char* who, const rt_accum* a, const void* pixels, int64_t n_pixels, bool host_list) {
    const std::string w(who);
    if (!a) return fail(RT_E_INVAL, w + ": null argument");
    if (n_pixels < 0 || n_pixels > (int64_t)a->npix()) return fail(RT_E_INVAL, w + ": n_pixels must be in 0 .. width * height");
    if (n_pixels > 0 && !pixels) return fail(RT_E_INVAL, w + ": null pixel list");
    if (host_list) {
        const int rc = check_pixel_list(who, (const uint32_t*)pixels, n_pixels, (int64_t)a->npix());
        if (rc != RT_OK) return rc;
    }
    if (a->K < 2 && !a->covered) return fail(RT_E_INVAL, w + ": a sparse pass needs two full-frame passes first");
    return RT_OK;
}

}  // namespace rt::api

extern "C" {

int rt_accum_create(int32_t device, int32_t width, int32_t height, void** out) {
    if (!out) return fail(RT_E_INVAL, "rt_accum_create: null argument");
    *out = nullptr;
    if (device < 0) return fail(RT_E_INVAL, "rt_accum_create: device ordinal must be >= 0");
    if (width < 1 || height < 1) return fail(RT_E_INVAL, "rt_accum_create: width/height must be positive");
    if ((int64_t)width * height > (int64_t)INT32_MAX) return fail(RT_E_INVAL, "rt_accum_create: image too large");
    rt_accum* a = new rt_accum;
    a->device = device;
    a->width = width;
    a->height = height;
    *out = a;
    return RT_OK;
}

void rt_accum_destroy(void* accum) {
    rt_accum* a = (rt_accum*)accum;
    if (!a) return;
    if (a->S || a->stage || a->adapt || a->batch) {
        (void)hipSetDevice(a->device);
        if (a->S) (void)hipFree(a->S);
        if (a->stage) (void)hipFree(a->stage);
        if (a->adapt) (void)hipFree(a->adapt);
        if (a->batch) (void)hipFree(a->batch);
    }
    delete a;
}

int rt_accum_reset(void* accum) {
    rt_accum* a = (rt_accum*)accum;
    if (!a) return fail(RT_E_INVAL, "rt_accum_reset: null argument");
    a->K = 0;  // the next pass stores without reading
    a->N = 0;
    a->sparse = false;  // the per-pixel counts are forgotten with the passes
    a->seeded = false;  // and so is reprojected history
    a->covered = false;
    return RT_OK;
}

int rt_accum_info(const void* accum, int64_t info[4]) {
    const rt_accum* a = (const rt_accum*)accum;
    if (!a || !info) return fail(RT_E_INVAL, "rt_accum_info: null argument");
    info[0] = a->K;
    info[1] = a->N;
    info[2] = a->width;
    info[3] = a->height;
    return RT_OK;
}

int rt_accum_add(void* accum, const rt_scene* scene, const rt_render_params* p, const volatile int32_t* cancel,
                 rt_render_stats* stats) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_accum_add(a, scene, p);
    if (rc == RT_OK) rc = accum_ready("rt_accum_add", a, true, false);
    if (rc != RT_OK) return rc;
    RenderCall call;
    rc = call.init("rt_accum_add", cancel, stats);
    if (rc != RT_OK) return rc;
    rc = render_enqueue(const_cast<rt_scene*>(scene), p, a->stage_rgb(), a->stage_sub(), call.cs.st, call.mirror.dev,
                        cancel, &call.ps);
    rc = call.finish("rt_accum_add", rc);
    if (rc != RT_OK) return rc;  // failed, or cancelled: S, Q, K and N untouched
    return accum_merge(a, a->stage_sub(), p->spp / 4, call.cs.st);
}

int rt_accum_add_sub(void* accum, const double* sub, int32_t n) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_accum_sub("rt_accum_add_sub", a, sub, n);
    if (rc == RT_OK) rc = accum_ready("rt_accum_add_sub", a, true, false);
    if (rc != RT_OK) return rc;
    CallStream cs;
    HIP_TRY(cs.init());
    HIP_TRY(hipMemcpyAsync(a->stage_sub(), sub, a->sub_bytes(), hipMemcpyHostToDevice, cs.st));
    return accum_merge(a, a->stage_sub(), n, cs.st);
}

int rt_accum_add_sub_device(void* accum, const void* d_sub, int32_t n, void* stream) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_accum_sub("rt_accum_add_sub_device", a, d_sub, n);
    if (rc == RT_OK) rc = accum_ready("rt_accum_add_sub_device", a, false, false);
    if (rc != RT_OK) return rc;
    return accum_merge(a, (const double*)d_sub, n, (hipStream_t)stream);
}

int rt_accum_resolve_device(void* accum, void* d_sub, void* d_var, void* d_rgb, void* stream) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_accum_resolve("rt_accum_resolve_device", a, d_var);
    const bool stage = d_rgb && !d_sub;
    if (rc == RT_OK) rc = accum_ready("rt_accum_resolve_device", a, stage, false);
    if (rc != RT_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = accum_resolve_enqueue(a, stage ? a->stage_sub() : (double*)d_sub, (float*)d_var, (uint8_t*)d_rgb, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_accum_resolve_device: ") + hipGetErrorString(e));
    return RT_OK;
}

int rt_accum_resolve(void* accum, double* sub_out, float* var_out, uint8_t* rgb_out) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_accum_resolve("rt_accum_resolve", a, var_out);
    if (rc == RT_OK) rc = accum_ready("rt_accum_resolve", a, true, false);
    if (rc != RT_OK) return rc;
    CallStream cs;
    HIP_TRY(cs.init());
    hipStream_t st = cs.st;
    const bool want_sub = sub_out || rgb_out;
    hipError_t e = accum_resolve_enqueue(a, want_sub ? a->stage_sub() : nullptr, var_out ? a->stage_var() : nullptr,
                                         rgb_out ? a->stage_rgb() : nullptr, st);
    if (e == hipSuccess && sub_out) e = hipMemcpyAsync(sub_out, a->stage_sub(), a->sub_bytes(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && var_out)
        e = hipMemcpyAsync(var_out, a->stage_var(), a->npix() * 4 * sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && rgb_out) e = hipMemcpyAsync(rgb_out, a->stage_rgb(), a->npix() * 3, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_accum_resolve: ") + hipGetErrorString(e));
    return RT_OK;
}

int rt_accum_counts(void* accum, uint32_t* k_out, uint32_t* n_out) {
    rt_accum* a = (rt_accum*)accum;
    if (!a) return fail(RT_E_INVAL, "rt_accum_counts: null argument");
    const size_t npix = a->npix();
    if (!a->sparse) {  // one K and N for the frame: no device call
        for (size_t i = 0; i < npix; ++i) {
            if (k_out) k_out[i] = (uint32_t)a->K;
            if (n_out) n_out[i] = (uint32_t)a->N;
        }
        return RT_OK;
    }
    int rc = need_device("rt_accum_counts", a->device);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(a->device));
    std::vector<uint32_t> both(npix * 2);
    HIP_TRY(hipMemcpy(both.data(), a->cnt(), npix * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npix; ++i) {
        if (k_out) k_out[i] = both[2 * i];
        if (n_out) n_out[i] = both[2 * i + 1];
    }
    return RT_OK;
}

// Accumulator reprojection across camera moves ---------------------------------------------

int rt_accum_reproject(void* dst, void* src, const rt_scene* dst_view, const rt_scene* src_view, uint32_t flags,
                       int32_t max_n, int64_t* n_valid) {
    rt_accum* d = (rt_accum*)dst;
    const rt_accum* s = (const rt_accum*)src;
    if (!d || !s || !dst_view || !src_view) return fail(RT_E_INVAL, "rt_accum_reproject: null argument");
    if (d == s) return fail(RT_E_INVAL, "rt_accum_reproject: dst and src must be two accumulators");
    if (d->width != s->width || d->height != s->height || d->device != s->device)
        return fail(RT_E_INVAL, "rt_accum_reproject: dst and src differ in size or device");
    if (dst_view->root != src_view->root) return fail(RT_E_INVAL, "rt_accum_reproject: the two views do not share a base");
    if (max_n < 1) return fail(RT_E_INVAL, "rt_accum_reproject: max_n must be >= 1");
    if (flags & ~RT_FLAG_MESH_NEAREST) return fail(RT_E_INVAL, "rt_accum_reproject: unknown flag");
    if (s->K < 2 && !s->covered)
        return fail(RT_E_INVAL, "rt_accum_reproject: src needs at least two full-frame passes");
    int rc = accum_ready("rt_accum_reproject", d, false, true);
    if (rc != RT_OK) return rc;
    rt::DevScene ds;
    rc = upload(const_cast<rt_scene*>(dst_view), d->device, &ds);  // the dst view's camera rides in ds
    if (rc != RT_OK) return rc;
    rt::ReprojArgs a{};
    a.width = d->width;
    a.height = d->height;
    a.nearest = (flags & RT_FLAG_MESH_NEAREST) && !dst_view->host.meshes.empty();
    a.max_n = max_n;
    rt::host::camera_frame(dst_view->cam_dir, dst_view->cam_right, dst_view->cam_fov, d->width, d->height, a.cx, a.cy);
    {
        // the inverse of (cx_s | cy_s | dir_s) by cofactors (rt_ffi.h): cross(a, b) = (a_y b_z - a_z b_y, a_z b_x -
        // a_x b_z, a_x b_y - a_y b_x), dot = (a_x b_x + a_y b_y) + a_z b_z, no FMA contraction
        double cxs[3], cys[3];
        const double* dir = src_view->cam_dir;
        rt::host::camera_frame(dir, src_view->cam_right, src_view->cam_fov, d->width, d->height, cxs, cys);
        auto cross = [](const double* u, const double* v, double* o) {
            o[0] = u[1] * v[2] - u[2] * v[1];
            o[1] = u[2] * v[0] - u[0] * v[2];
            o[2] = u[0] * v[1] - u[1] * v[0];
        };
        double yd[3], dx[3], xy[3];
        cross(cys, dir, yd);
        cross(dir, cxs, dx);
        cross(cxs, cys, xy);
        const double D = cxs[0] * yd[0] + cxs[1] * yd[1] + cxs[2] * yd[2];
        for (int k = 0; k < 3; ++k) {
            a.A[k] = yd[k] / D;
            a.B[k] = dx[k] / D;
            a.C[k] = xy[k] / D;
            a.pos_s[k] = src_view->cam_pos[k];
        }
    }
    a.S_src = s->S;
    a.Q_src = s->Q;
    a.cnt_src = s->sparse ? s->cnt() : nullptr;
    a.K_src = (uint32_t)s->K;
    a.N_src = (uint32_t)s->N;
    a.S_dst = d->S;
    a.Q_dst = d->Q;
    a.cnt_dst = d->cnt();
    a.n_valid = (unsigned long long*)d->adapt_total();
    // dst is reset first: whatever happens below, it never keeps half of an earlier history
    d->K = 0;
    d->N = 0;
    d->sparse = false;
    d->seeded = false;
    d->covered = false;
    CallStream cs;
    HIP_TRY(cs.init());
    unsigned long long count = 0;
    hipError_t e = hipMemsetAsync(a.n_valid, 0, sizeof(unsigned long long), cs.st);
    if (e == hipSuccess) e = rt::launch_reproject_f64(ds, a, cs.st);
    if (e == hipSuccess) e = hipMemcpyAsync(&count, a.n_valid, sizeof count, hipMemcpyDeviceToHost, cs.st);
    const hipError_t es = hipStreamSynchronize(cs.st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_accum_reproject: ") + hipGetErrorString(e));
    d->sparse = true;  // the per-pixel counts are live
    d->seeded = true;  // the next merge adds
    if (n_valid) *n_valid = (int64_t)count;
    return RT_OK;
}

}  // extern "C"
