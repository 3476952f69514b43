// C ABI (include/rt_ffi.h): rendering to a per-pixel error target — pixel-list renders and their
// kernel families, sparse merges, the selection — and the holes of a reprojection and their fill
// (DESIGN.md §15).
#include <algorithm>
#include <cstring>
#include <functional>

#include "accum_state.hpp"

using namespace rt::api;

namespace {

// The kernel family of a pixel-list render. The pool family a scene has under its flags is the one its
// full frame runs (kernels.h list_pool_family), decided from the host-side packed scene as check_diag decides its
// forms; `path` asks for a family or leaves the choice to the length rule.
static_assert(RT_LIST_FUSED == rt::kListFused && RT_LIST_FPOOL == rt::kListFpool && RT_LIST_ROLES == rt::kListRoles,
              "kernels.h mirrors rt_ffi.h's family ids");
int list_pool_of(const rt_scene* s, const rt_render_params* p) {
    return rt::list_pool_family(make_render_args(s, p), !s->packed.slots.empty());
}
// The automatic choice: the scene's pool at every list length. On the cubes and the unicorn the pool kernels were never
// slower than k_render_list_f64 for lists from every pixel of a 1920x1080 frame down to one pixel (DESIGN.md §16's
// table), so no length threshold exists; scene, flags and length decide alone, so the answer needs no device.
int list_auto_family(int pool, int64_t /*n_pixels*/) { return pool; }

int check_select(const char* who, const rt_accum* a, float abs_tol, float rel_tol, int64_t cap, const void* out,
                 const int64_t* n_out) {
    const std::string w(who);
    if (!a || !n_out) return fail(RT_E_INVAL, w + ": null argument");
    if (!(abs_tol >= 0.f) || !(rel_tol >= 0.f)) return fail(RT_E_INVAL, w + ": tolerances must be >= 0 and not NaN");
    if (cap < 0 || (cap > 0 && !out)) return fail(RT_E_INVAL, w + ": bad output buffer");
    if (a->K < 2 && !a->covered) return fail(RT_E_INVAL, w + ": the selection needs at least two passes");
    return RT_OK;
}

// The end of a compaction into a pixel list (select_run, holes_run), enqueued on `st` with outcome e: waits, and
// reads the list's full length from adapt_total and, where asked, the 8-byte count the kernel left at d_extra.
int list_counts(const char* who, rt_accum* a, hipError_t e, hipStream_t st, int64_t* n_out,
                const unsigned long long* d_extra = nullptr, int64_t* extra_out = nullptr) {
    uint32_t total = 0;
    unsigned long long extra = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&total, a->adapt_total(), sizeof total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && extra_out) e = hipMemcpyAsync(&extra, d_extra, sizeof extra, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    *n_out = (int64_t)total;
    if (extra_out) *extra_out = (int64_t)extra;
    return RT_OK;
}

// The host form of a compaction (rt_accum_select, rt_accum_holes): run(d_list, cap, st) compacts into the
// accumulator's own list buffer on a stream of the call's and leaves the full length in *n_out; the first
// min(*n_out, cap) ids go back to the caller.
int list_to_host(rt_accum* a, uint32_t* pixels_out, int64_t cap, const int64_t* n_out,
                 const std::function<int(uint32_t*, int64_t, hipStream_t)>& run) {
    CallStream cs;
    HIP_TRY(cs.init());
    const int64_t dcap = std::min<int64_t>(cap, (int64_t)a->npix());  // the list buffer holds every pixel
    const int rc = run(a->adapt_list(), dcap, cs.st);
    if (rc != RT_OK) return rc;
    const int64_t n = std::min(*n_out, dcap);
    if (n > 0) HIP_TRY(hipMemcpy(pixels_out, a->adapt_list(), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

// Resolves the variance into the staging area, selects into d_out (device, cap ids) on `st`, waits, and reads the count.
int select_run(rt_accum* a, float abs_tol, float rel_tol, int32_t max_n, uint32_t* d_out, int64_t cap, int64_t* n_out,
               hipStream_t st) {
    hipError_t e = accum_resolve_enqueue(a, nullptr, a->stage_var(), nullptr, st);
    if (e == hipSuccess)
        e = rt::launch_accum_select(a->S, a->stage_var(), a->sparse ? a->cnt() : nullptr, a->N, a->width, a->height,
                                    abs_tol, rel_tol, max_n, a->adapt_scratch(), d_out, (long)cap, a->adapt_total(), st);
    return list_counts("rt_accum_select", a, e, st, n_out);
}

// Filling the holes of a reprojection -------------------------------------------------------

// The arguments of a hole list that need no device; the seeded state is asked for last, so that every other check
// can be reached without a GPU.
int check_holes(const char* who, const rt_accum* a, int32_t period, int32_t phase) {
    const std::string w(who);
    if (period < 0) return fail(RT_E_INVAL, w + ": period must be >= 0");
    if (phase < 0 || phase >= std::max(period, 1)) return fail(RT_E_INVAL, w + ": phase must be in 0 .. max(period, 1) - 1");
    if (!a->seeded) return fail(RT_E_INVAL, w + ": the accumulator is not seeded by rt_accum_reproject");
    return RT_OK;
}

// Lists the holes into d_out (device, cap ids) on `st`, waits, and reads the two counts.
int holes_run(rt_accum* a, int32_t period, int32_t phase, uint32_t* d_out, int64_t cap, int64_t* n_out, int64_t* n_holes,
              hipStream_t st) {
    unsigned long long* d_holes = (unsigned long long*)(a->adapt_total() + 2);
    hipError_t e = rt::launch_accum_holes(a->cnt(), a->width, a->height, period, phase, a->adapt_scratch(), d_out, (long)cap,
                                          a->adapt_total(), d_holes, st);
    return list_counts("rt_accum_holes", a, e, st, n_out, d_holes, n_holes);
}

int check_holes_call(const char* who, const rt_accum* a, int32_t period, int32_t phase, int64_t cap, const void* out,
                     const int64_t* n_out) {
    const std::string w(who);
    if (!a || !n_out) return fail(RT_E_INVAL, w + ": null argument");
    if (cap < 0 || (cap > 0 && !out)) return fail(RT_E_INVAL, w + ": bad output buffer");
    return check_holes(who, a, period, phase);
}

}  // namespace

namespace rt::api {

int check_render_pixels(const char* who, const rt_scene* scene, const rt_render_params* p, const void* pixels,
                        int64_t n_pixels) {
    const std::string w(who);
    if (!scene || !p) return fail(RT_E_INVAL, w + ": null argument");
    const int rc = check_params(p);
    if (rc != RT_OK) return rc;
    if (p->x0 != 0 || p->y0 != 0 || p->tile_w != p->width || p->tile_h != p->height)
        return fail(RT_E_INVAL, w + ": params must be the whole frame");
    if (p->row_step > 1) return fail(RT_E_INVAL, w + ": row_step must be 0 or 1");
    if (p->flags & (RT_FLAG_FP32 | RT_FLAG_MESH_NEAREST))
        return fail(RT_E_INVAL, w + ": RT_FLAG_FP32 and RT_FLAG_MESH_NEAREST are not supported by the pixel-list render");
    if (n_pixels < 0 || n_pixels > (int64_t)p->width * p->height)
        return fail(RT_E_INVAL, w + ": n_pixels must be in 0 .. width * height");
    if (n_pixels > (int64_t)INT32_MAX / 4) return fail(RT_E_INVAL, w + ": n_pixels * 4 must fit an int32");
    if (n_pixels > 0 && !pixels) return fail(RT_E_INVAL, w + ": null pixel list");
    return RT_OK;
}

int check_pixel_list(const char* who, const uint32_t* pixels, int64_t n_pixels, int64_t npix) {
    for (int64_t e = 0; e < n_pixels; ++e) {
        if ((int64_t)pixels[e] >= npix)
            return fail(RT_E_INVAL, std::string(who) + ": pixel id " + std::to_string(pixels[e]) + " outside the frame");
        if (e > 0 && pixels[e] <= pixels[e - 1])
            return fail(RT_E_INVAL, std::string(who) + ": the pixel list must be strictly ascending");
    }
    return RT_OK;
}

int list_family_of(const char* who, const rt_scene* s, const rt_render_params* p, int64_t n_pixels, int32_t path,
                   int* family) {
    if (path < RT_LIST_AUTO || path > RT_LIST_ROLES) return fail(RT_E_INVAL, std::string(who) + ": unknown kernel family");
    const int pool = list_pool_of(s, p);
    if (path == RT_LIST_AUTO) *family = list_auto_family(pool, n_pixels);
    else if (path == RT_LIST_FUSED || path == pool) *family = path;
    else return fail(RT_E_INVAL, std::string(who) + ": the scene has no pixel-list instance of this kernel family");
    return RT_OK;
}

int render_units_enqueue(rt_scene* s, const rt_render_params* p, const rt::UnitList& units, uint8_t* d_rgb, double* d_sub,
                         hipStream_t st, const int32_t* dcancel, PendingStats* ps, int32_t path, const char* what) {
    const int64_t n = units.n;  // unit-groups: entries of the compact buffer
    int family = RT_LIST_FUSED;
    int rc = list_family_of(what, s, p, n, path, &family);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    rt::DevScene ds;
    rc = upload(s, p->device, &ds);
    if (rc != RT_OK) return rc;
    rt::RenderArgs a = make_render_args(s, p);
    a.x0 = 0;
    a.y0 = 0;
    a.row_step = 1;
    a.tw = (int32_t)n;  // k_finalize_f64's view of the compact buffer
    a.th = 1;
    if (units.seeds) a.seed = 0;  // unused: every unit draws from its pass's seed
    a.rgb_out = d_rgb;
    a.cancel = dcancel;
    if (ps) {
        const hipError_t e = ps->init(ps->out);
        if (e != hipSuccess) return fail(RT_E_HIP, std::string("stats: ") + hipGetErrorString(e));
        ps->samples = n * 4 * (int64_t)a.n_samples;
        HIP_TRY(hipEventRecord(ps->e0, st));
    }
    hipError_t te;
    std::unique_ptr<rt::Workspace> ws = take_workspace(s, p->device, st, &te);
    if (!ws) return fail(RT_E_HIP, std::string("workspace: ") + hipGetErrorString(te));
    hipError_t e = ws->ensure_counters();
    double* sub = d_sub;
    if (e == hipSuccess && !sub) {
        e = ws->ensure_sub((size_t)n);
        sub = ws->sub_buf;
    }
    a.sub_out = sub;
    if (e == hipSuccess && ps) e = hipMemsetAsync(ws->counters, 0, 8 * sizeof(unsigned long long), st);
    if (e == hipSuccess && a.n_samples <= 0) e = hipMemsetAsync(sub, 0, (size_t)n * 12 * sizeof(double), st);
    if (e == hipSuccess) {
        a.counters = ps ? ws->counters : nullptr;
        // the pool kernels split their last units into chunks of samples: the frame's scratch rule, for this many unit-groups
        if (family != RT_LIST_FUSED) ensure_tail_scratch(ws.get(), a, (size_t)n);
        e = rt::launch_render_units_f64(ds, a, units, sub, (uint32_t*)(ws->counters + 4), family, ws->tail_buf,
                                        ws->tail_cap, st);
    }
    if (e == hipSuccess && d_rgb) e = rt::launch_finalize_f64(a, sub, st);
    if (e == hipSuccess && ps) e = hipEventRecord(ps->e1, st);
    if (e == hipSuccess && ps) e = hipMemcpyAsync(ps->count, ws->counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    give_workspace(s, std::move(ws), st);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return RT_OK;
}

}  // namespace rt::api

extern "C" {

int rt_render_pixels_with_device(const rt_scene* scene, const rt_render_params* params, const void* d_pixels,
                                 int64_t n_pixels, int32_t path, void* d_rgb, void* d_sub, void* stream,
                                 rt_render_stats* stats) {
    int rc = check_render_pixels("rt_render_pixels_device", scene, params, d_pixels, n_pixels);
    int family;
    if (rc == RT_OK) rc = list_family_of("rt_render_pixels_device", scene, params, n_pixels, path, &family);
    if (rc != RT_OK) return rc;
    if (n_pixels == 0) return empty_list(stats);
    rc = need_device("rt_render_pixels_device", params->device);
    if (rc != RT_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    PendingStats ps;
    ps.out = stats;
    rc = render_units_enqueue(const_cast<rt_scene*>(scene), params, {(const uint32_t*)d_pixels, n_pixels, nullptr},
                              (uint8_t*)d_rgb, (double*)d_sub, st, nullptr, stats ? &ps : nullptr, path, kListRender);
    return stats_sync(rc, st, stats ? &ps : nullptr);
}

int rt_render_pixels_device(const rt_scene* scene, const rt_render_params* params, const void* d_pixels,
                            int64_t n_pixels, void* d_rgb, void* d_sub, void* stream, rt_render_stats* stats) {
    return rt_render_pixels_with_device(scene, params, d_pixels, n_pixels, RT_LIST_AUTO, d_rgb, d_sub, stream, stats);
}

int rt_render_pixels_with(const rt_scene* scene, const rt_render_params* p, const uint32_t* pixels, int64_t n_pixels,
                          int32_t path, uint8_t* rgb_out, double* sub_out, const volatile int32_t* cancel,
                          rt_render_stats* stats) {
    int rc = check_render_pixels("rt_render_pixels", scene, p, pixels, n_pixels);
    if (rc == RT_OK) rc = check_pixel_list("rt_render_pixels", pixels, n_pixels, (int64_t)p->width * p->height);
    int family;
    if (rc == RT_OK) rc = list_family_of("rt_render_pixels", scene, p, n_pixels, path, &family);
    if (rc != RT_OK) return rc;
    if (n_pixels == 0) return empty_list(stats);
    rc = need_device("rt_render_pixels", p->device);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    const size_t n = (size_t)n_pixels, b_sub = n * 12 * sizeof(double);
    RenderCall call;
    const size_t at_sub = call.mem.part(b_sub), at_pix = call.mem.part(n * sizeof(uint32_t)), at_rgb = call.mem.part(n * 3);
    rc = call.init("rt_render_pixels", cancel, stats);
    if (rc != RT_OK) return rc;
    double* d_sub = call.mem.at<double>(at_sub);
    uint32_t* d_pix = call.mem.at<uint32_t>(at_pix);
    uint8_t* d_rgb = call.mem.at<uint8_t>(at_rgb);
    const hipError_t e = hipMemcpyAsync(d_pix, pixels, n * sizeof(uint32_t), hipMemcpyHostToDevice, call.cs.st);
    if (e != hipSuccess) return oom_or_hip(e, "rt_render_pixels");
    rc = render_units_enqueue(const_cast<rt_scene*>(scene), p, {d_pix, n_pixels, nullptr}, rgb_out ? d_rgb : nullptr, d_sub,
                              call.cs.st, call.mirror.dev, &call.ps, path, kListRender);
    return call.finish("rt_render_pixels", rc, {{rgb_out, d_rgb, n * 3}, {sub_out, d_sub, b_sub}});
}

int rt_render_pixels(const rt_scene* scene, const rt_render_params* p, const uint32_t* pixels, int64_t n_pixels,
                     uint8_t* rgb_out, double* sub_out, const volatile int32_t* cancel, rt_render_stats* stats) {
    return rt_render_pixels_with(scene, p, pixels, n_pixels, RT_LIST_AUTO, rgb_out, sub_out, cancel, stats);
}

int rt_render_pixels_path(const rt_scene* scene, const rt_render_params* p, int64_t n_pixels, int32_t path_out[2]) {
    if (!path_out) return fail(RT_E_INVAL, "rt_render_pixels_path: null argument");
    // (the list itself plays no part: a non-null stand-in passes check_render_pixels' null-list rule)
    const int rc = check_render_pixels("rt_render_pixels_path", scene, p, path_out, n_pixels);
    if (rc != RT_OK) return rc;
    path_out[1] = list_pool_of(scene, p);
    path_out[0] = list_auto_family(path_out[1], n_pixels);
    return RT_OK;
}

int rt_accum_add_pixels(void* accum, const rt_scene* scene, const rt_render_params* p, const uint32_t* pixels,
                        int64_t n_pixels, const volatile int32_t* cancel, rt_render_stats* stats) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_accum_add(a, scene, p);
    if (rc == RT_OK) rc = check_render_pixels("rt_accum_add_pixels", scene, p, pixels, n_pixels);
    if (rc == RT_OK) rc = check_sparse("rt_accum_add_pixels", a, pixels, n_pixels, true);
    if (rc != RT_OK) return rc;
    if (n_pixels == 0) return empty_list(stats);
    rc = accum_ready("rt_accum_add_pixels", a, true, true);
    if (rc != RT_OK) return rc;
    RenderCall call;
    rc = call.init("rt_accum_add_pixels", cancel, stats);
    if (rc != RT_OK) return rc;
    hipStream_t st = call.cs.st;
    const hipError_t e = hipMemcpyAsync(a->adapt_list(), pixels, (size_t)n_pixels * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return oom_or_hip(e, "rt_accum_add_pixels");
    rc = render_units_enqueue(const_cast<rt_scene*>(scene), p, {a->adapt_list(), n_pixels, nullptr}, nullptr, a->stage_sub(),
                              st, call.mirror.dev, &call.ps, RT_LIST_AUTO, kListRender);
    rc = call.finish("rt_accum_add_pixels", rc);
    if (rc != RT_OK) return rc;  // failed, or cancelled: nothing merged
    return accum_merge_list(a, a->adapt_list(), n_pixels, a->stage_sub(), p->spp / 4, st);
}

int rt_accum_add_sub_pixels(void* accum, const uint32_t* pixels, int64_t n_pixels, const double* sub, int32_t n) {
    rt_accum* a = (rt_accum*)accum;
    int rc = RT_OK;
    if (n < 1) rc = fail(RT_E_INVAL, "rt_accum_add_sub_pixels: n must be >= 1");
    if (rc == RT_OK && n_pixels > 0 && !sub) rc = fail(RT_E_INVAL, "rt_accum_add_sub_pixels: null argument");
    if (rc == RT_OK) rc = check_sparse("rt_accum_add_sub_pixels", a, pixels, n_pixels, true);
    if (rc != RT_OK || n_pixels == 0) return rc;
    rc = accum_ready("rt_accum_add_sub_pixels", a, true, true);
    if (rc != RT_OK) return rc;
    CallStream cs;
    HIP_TRY(cs.init());
    HIP_TRY(hipMemcpyAsync(a->adapt_list(), pixels, (size_t)n_pixels * sizeof(uint32_t), hipMemcpyHostToDevice, cs.st));
    HIP_TRY(hipMemcpyAsync(a->stage_sub(), sub, (size_t)n_pixels * 12 * sizeof(double), hipMemcpyHostToDevice, cs.st));
    return accum_merge_list(a, a->adapt_list(), n_pixels, a->stage_sub(), n, cs.st);
}

int rt_accum_add_sub_pixels_device(void* accum, const void* d_pixels, int64_t n_pixels, const void* d_sub, int32_t n,
                                   void* stream) {
    rt_accum* a = (rt_accum*)accum;
    int rc = RT_OK;
    if (n < 1) rc = fail(RT_E_INVAL, "rt_accum_add_sub_pixels_device: n must be >= 1");
    if (rc == RT_OK && n_pixels > 0 && !d_sub) rc = fail(RT_E_INVAL, "rt_accum_add_sub_pixels_device: null argument");
    if (rc == RT_OK) rc = check_sparse("rt_accum_add_sub_pixels_device", a, d_pixels, n_pixels, false);
    if (rc != RT_OK || n_pixels == 0) return rc;
    rc = accum_ready("rt_accum_add_sub_pixels_device", a, false, true);
    if (rc != RT_OK) return rc;
    return accum_merge_list(a, (const uint32_t*)d_pixels, n_pixels, (const double*)d_sub, n, (hipStream_t)stream);
}

int rt_accum_select_device(void* accum, float abs_tol, float rel_tol, int32_t max_n, void* d_pixels, int64_t cap,
                           int64_t* n_out, void* stream) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_select("rt_accum_select_device", a, abs_tol, rel_tol, cap, d_pixels, n_out);
    if (rc == RT_OK) rc = accum_ready("rt_accum_select_device", a, true, true);
    if (rc != RT_OK) return rc;
    return select_run(a, abs_tol, rel_tol, max_n, (uint32_t*)d_pixels, cap, n_out, (hipStream_t)stream);
}

int rt_accum_select(void* accum, float abs_tol, float rel_tol, int32_t max_n, uint32_t* pixels_out, int64_t cap,
                    int64_t* n_out) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_select("rt_accum_select", a, abs_tol, rel_tol, cap, pixels_out, n_out);
    if (rc == RT_OK) rc = accum_ready("rt_accum_select", a, true, true);
    if (rc != RT_OK) return rc;
    return list_to_host(a, pixels_out, cap, n_out, [&](uint32_t* d_list, int64_t dcap, hipStream_t st) {
        return select_run(a, abs_tol, rel_tol, max_n, d_list, dcap, n_out, st);
    });
}

int rt_accum_holes_device(void* accum, int32_t period, int32_t phase, void* d_pixels, int64_t cap, int64_t* n_out,
                          int64_t* n_holes, void* stream) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_holes_call("rt_accum_holes_device", a, period, phase, cap, d_pixels, n_out);
    if (rc == RT_OK) rc = accum_ready("rt_accum_holes_device", a, false, true);
    if (rc != RT_OK) return rc;
    return holes_run(a, period, phase, (uint32_t*)d_pixels, cap, n_out, n_holes, (hipStream_t)stream);
}

int rt_accum_holes(void* accum, int32_t period, int32_t phase, uint32_t* pixels_out, int64_t cap, int64_t* n_out,
                   int64_t* n_holes) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_holes_call("rt_accum_holes", a, period, phase, cap, pixels_out, n_out);
    if (rc == RT_OK) rc = accum_ready("rt_accum_holes", a, false, true);
    if (rc != RT_OK) return rc;
    return list_to_host(a, pixels_out, cap, n_out, [&](uint32_t* d_list, int64_t dcap, hipStream_t st) {
        return holes_run(a, period, phase, d_list, dcap, n_out, n_holes, st);
    });
}

int rt_accum_fill(void* accum, const rt_scene* scene, const rt_render_params* p, uint64_t seed2, int32_t period,
                  int32_t phase, const volatile int32_t* cancel, rt_render_stats* stats, int64_t fill_out[2]) {
    rt_accum* a = (rt_accum*)accum;
    int rc = check_accum_add(a, scene, p);
    if (rc == RT_OK) rc = check_render_pixels("rt_accum_fill", scene, p, nullptr, 0);
    if (rc == RT_OK) rc = check_holes("rt_accum_fill", a, period, phase);
    if (rc == RT_OK) rc = accum_ready("rt_accum_fill", a, true, true);
    if (rc != RT_OK) return rc;
    rt_render_stats sum, one;  // each pass's stats go to `one`
    std::memset(&sum, 0, sizeof sum);
    RenderCall call;
    rc = call.init("rt_accum_fill", cancel, &one);
    if (rc != RT_OK) return rc;
    hipStream_t st = call.cs.st;
    int64_t lens[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        // pass 1: the holes and the refresh pattern; pass 2: what still lacks a second pass. The list stays on the
        // device; only its length comes back.
        int64_t n_list = 0;
        rc = holes_run(a, pass == 0 ? period : 0, pass == 0 ? phase : 0, a->adapt_list(), (int64_t)a->npix(), &n_list,
                       nullptr, st);
        if (rc != RT_OK) return rc;
        lens[pass] = n_list;
        if (n_list == 0) continue;  // an empty list launches nothing
        if (n_list > (int64_t)INT32_MAX / 4) return fail(RT_E_INVAL, "rt_accum_fill: the list's length * 4 must fit an int32");
        rt_render_params pp = *p;
        if (pass == 1) pp.seed = seed2;
        rc = render_units_enqueue(const_cast<rt_scene*>(scene), &pp, {a->adapt_list(), n_list, nullptr}, nullptr,
                                  a->stage_sub(), st, call.mirror.dev, &call.ps, RT_LIST_AUTO, kListRender);
        rc = call.finish("rt_accum_fill", rc);
        if (rc < 0) return rc;
        if (rc != RT_OK) break;  // cancelled: this pass merges nothing and the accumulator stays uncovered
        rc = accum_merge_list(a, a->adapt_list(), n_list, a->stage_sub(), p->spp / 4, st);
        if (rc != RT_OK) return rc;
        sum.samples += one.samples;
        sum.vertices += one.vertices;
        sum.iterations += one.iterations;
        sum.device_ms += one.device_ms;
        for (int k = 0; k < 8; ++k) {
            sum.kernel_ms[k] += one.kernel_ms[k];
            sum.kernel_launches[k] += one.kernel_launches[k];
        }
    }
    if (stats) *stats = sum;
    if (fill_out) {
        fill_out[0] = lens[0];
        fill_out[1] = lens[1];
    }
    if (rc == RT_OK) a->covered = true;  // every K_p >= 2
    return rc;
}

}  // extern "C"
