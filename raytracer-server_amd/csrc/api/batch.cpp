// C ABI (include/rt_ffi.h): batched passes — several error-target passes per pixel in one launch —
// and the plan that chooses them.
#include <algorithm>

#include "accum_state.hpp"

using namespace rt::api;

namespace {

static_assert(RT_PASSES_MAX == rt::kPassesMax, "accum.h mirrors rt_ffi.h's RT_PASSES_MAX");
// a unit word holds the pixel id below the pass index (integrator_f64.h kPassShift)
constexpr int64_t kPassFramePixels = (int64_t)1 << 28;

// The arguments of a batched render that need no device: check_render_pixels' rules, a frame whose pixel ids leave
// the top 4 bits of a word free, and 1 .. RT_PASSES_MAX seeds.
int check_passes(const char* who, const rt_scene* scene, const rt_render_params* p, const void* pixels,
                 const void* counts, int64_t n_pixels, const uint64_t* seeds, int32_t n_seeds) {
    const std::string w(who);
    int rc = check_render_pixels(who, scene, p, pixels, n_pixels);
    if (rc != RT_OK) return rc;
    if (n_pixels > 0 && !counts) return fail(RT_E_INVAL, w + ": null count list");
    if (!seeds) return fail(RT_E_INVAL, w + ": null seeds");
    if (n_seeds < 1 || n_seeds > RT_PASSES_MAX) return fail(RT_E_INVAL, w + ": n_seeds must be in 1 .. 16");
    if ((int64_t)p->width * p->height >= kPassFramePixels)
        return fail(RT_E_INVAL, w + ": width * height must be below 2^28 for a batched render");
    return RT_OK;
}

// Host counts: each in 1 .. n_seeds, and no more than a frame's worth of units in all.
int check_pass_counts(const char* who, const uint8_t* counts, int64_t n_pixels, int32_t n_seeds, int64_t npix,
                      int64_t* units_out) {
    int64_t units = 0;
    for (int64_t e = 0; e < n_pixels; ++e) {
        if (counts[e] < 1 || (int32_t)counts[e] > n_seeds)
            return fail(RT_E_INVAL, std::string(who) + ": every count must be in 1 .. n_seeds");
        units += counts[e];
    }
    if (units > npix) return fail(RT_E_INVAL, std::string(who) + ": more than width * height units");
    *units_out = units;
    return RT_OK;
}

// n_seeds host seeds -> 16 device words on `st` (h16: storage that outlives the work on `st`).
hipError_t seeds_upload(uint64_t* d_seeds, const uint64_t* seeds, int32_t n_seeds, uint64_t* h16, hipStream_t st) {
    for (int i = 0; i < RT_PASSES_MAX; ++i) h16[i] = i < n_seeds ? seeds[i] : 0;
    return hipMemcpyAsync(d_seeds, h16, RT_PASSES_MAX * sizeof(uint64_t), hipMemcpyHostToDevice, st);
}

int check_plan(const char* who, const rt_accum* a, float abs_tol, float rel_tol, int32_t n, float gain,
               int32_t max_passes) {
    const std::string w(who);
    if (!a) return fail(RT_E_INVAL, w + ": null argument");
    if (!(abs_tol >= 0.f) || !(rel_tol >= 0.f)) return fail(RT_E_INVAL, w + ": tolerances must be >= 0 and not NaN");
    if (n < 1) return fail(RT_E_INVAL, w + ": n must be >= 1");
    if (!(gain > 0.f) || !(gain <= 1.f)) return fail(RT_E_INVAL, w + ": gain must be in (0, 1]");
    if (max_passes < 1 || max_passes > RT_PASSES_MAX) return fail(RT_E_INVAL, w + ": max_passes must be in 1 .. 16");
    if ((int64_t)a->npix() >= kPassFramePixels) return fail(RT_E_INVAL, w + ": width * height must be below 2^28");
    return RT_OK;
}
// (asked for last, so that every other check can be reached without a GPU)
int check_plan_passes(const char* who, const rt_accum* a) {
    if (a->K < 2 && !a->covered) return fail(RT_E_INVAL, std::string(who) + ": the plan needs at least two passes");
    return RT_OK;
}

// What opens rt_accum_plan and rt_accum_plan_device: the plan's arguments, the outputs (have_outs: both lists are
// there), the two passes (asked for last, check_plan_passes), then the batch buffers.
int plan_begin(const char* who, rt_accum* a, float abs_tol, float rel_tol, int32_t n, float gain, int32_t max_passes,
               bool have_outs, int64_t cap, const int64_t* n_out) {
    int rc = check_plan(who, a, abs_tol, rel_tol, n, gain, max_passes);
    if (rc == RT_OK && !n_out) rc = fail(RT_E_INVAL, std::string(who) + ": null argument");
    if (rc == RT_OK && (cap < 0 || (cap > 0 && !have_outs))) rc = fail(RT_E_INVAL, std::string(who) + ": bad output buffer");
    if (rc == RT_OK) rc = check_plan_passes(who, a);
    if (rc == RT_OK) rc = batch_ready(who, a);
    return rc;
}

// plan_run's res to the caller: the list length, and where asked the unit total and the largest final count.
void plan_result(const int64_t res[3], int64_t* n_out, int64_t* units_out, int64_t* passes_out) {
    *n_out = res[0];
    if (units_out) *units_out = res[1];
    if (passes_out) *passes_out = res[2];
}

// The plan on `st`: the variance into the staging area, the wanted counts and their histogram, the frame cap on the
// host (the largest C' whose unit total fits a frame), then ids and final counts into d_pixels / d_counts (device,
// cap entries). res = list length, unit total, largest final count. Waits.
int plan_run(const char* who, rt_accum* a, float abs_tol, float rel_tol, int32_t max_n, int32_t n, float gain,
             int32_t max_passes, uint32_t* d_pixels, uint8_t* d_counts, int64_t cap, int64_t res[3], hipStream_t st) {
    uint32_t* words = a->batch_words();
    hipError_t e = accum_resolve_enqueue(a, nullptr, a->stage_var(), nullptr, st);
    if (e == hipSuccess)
        e = rt::launch_accum_plan_count(a->S, a->stage_var(), a->sparse ? a->cnt() : nullptr, a->N, a->width, a->height,
                                        abs_tol, rel_tol, max_n, n, gain, max_passes, a->adapt_scratch(), a->batch_want(),
                                        words, a->adapt_total(), st);
    uint32_t hist[RT_PASSES_MAX + 1] = {0}, total = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(hist, words, sizeof hist, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, a->adapt_total(), sizeof total, hipMemcpyDeviceToHost, st);
    hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    const int64_t npix = (int64_t)a->npix();
    int32_t cmax = 1;
    int64_t units = 0;
    for (int32_t c1 = max_passes; c1 >= 1; --c1) {
        units = 0;
        for (int32_t c = 1; c <= RT_PASSES_MAX; ++c) units += (int64_t)hist[c] * std::min(c, c1);
        cmax = c1;
        if (units <= npix) break;
    }
    int32_t used = 0;
    for (int32_t c = 1; c <= RT_PASSES_MAX; ++c)
        if (hist[c]) used = std::min(c, cmax);
    res[0] = (int64_t)total;
    res[1] = total ? units : 0;
    res[2] = used;
    if (total == 0 || cap <= 0) return RT_OK;
    e = rt::launch_accum_plan_write(a->adapt_scratch(), a->batch_want(), (long)npix, cmax, d_pixels, d_counts, (long)cap, st);
    es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return RT_OK;
}

// Expands the accumulator's device lists (adapt_list, batch_counts: n_pixels entries, `units` units in all), renders
// the units into the staging buffer with the 16 seeds in batch_seeds and merges them; RT_CANCELLED merges nothing.
int batch_render_merge(const char* who, rt_accum* a, const rt_scene* scene, const rt_render_params* p, int64_t n_pixels,
                       int64_t units, RenderCall& call) {
    hipStream_t st = call.cs.st;
    const hipError_t e = rt::launch_accum_expand(a->adapt_list(), a->batch_counts(), (long)n_pixels, a->batch_runs(),
                                                 a->batch_off(), a->batch_units(), (long)units, a->batch_words() + 20, st);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    // RT_LIST_AUTO: the scene's pool wherever it has one
    int rc = render_units_enqueue(const_cast<rt_scene*>(scene), p, {a->batch_units(), units, a->batch_seeds()}, nullptr,
                                  a->stage_sub(), st, call.mirror.dev, &call.ps, RT_LIST_AUTO, kBatchRender);
    rc = call.finish(who, rc);
    if (rc != RT_OK) return rc;  // failed, or cancelled: nothing merged
    return accum_merge_list(a, a->adapt_list(), n_pixels, a->stage_sub(), p->spp / 4, st, a->batch_counts(), a->batch_off());
}

}  // namespace

extern "C" {

int rt_render_pixel_passes_with(const rt_scene* scene, const rt_render_params* p, const uint32_t* pixels,
                                const uint8_t* counts, int64_t n_pixels, const uint64_t* seeds, int32_t n_seeds, int32_t path,
                                uint8_t* rgb_out, double* sub_out, const volatile int32_t* cancel, rt_render_stats* stats) {
    const char* who = "rt_render_pixel_passes";
    int rc = check_passes(who, scene, p, pixels, counts, n_pixels, seeds, n_seeds);
    if (rc == RT_OK) rc = check_pixel_list(who, pixels, n_pixels, (int64_t)p->width * p->height);
    int64_t units = 0;
    if (rc == RT_OK) rc = check_pass_counts(who, counts, n_pixels, n_seeds, (int64_t)p->width * p->height, &units);
    int family;
    if (rc == RT_OK) rc = list_family_of(who, scene, p, units, path, &family);
    if (rc != RT_OK) return rc;
    if (n_pixels == 0) return empty_list(stats);
    rc = need_device(who, p->device);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    // the expansion on the host: unit off[e] + i = pixel | i << 28
    std::vector<uint32_t> words((size_t)units);
    {
        size_t u = 0;
        for (int64_t e = 0; e < n_pixels; ++e)
            for (uint32_t i = 0; i < counts[e]; ++i) words[u++] = pixels[e] | (i << 28);
    }
    uint64_t h_seeds[RT_PASSES_MAX];
    const size_t n = (size_t)units, b_sub = n * 12 * sizeof(double);
    RenderCall call;
    const size_t at_sub = call.mem.part(b_sub), at_units = call.mem.part(n * sizeof(uint32_t)), at_rgb = call.mem.part(n * 3),
                 at_seeds = call.mem.part(sizeof h_seeds);
    rc = call.init(who, cancel, stats);
    if (rc != RT_OK) return rc;
    double* d_sub = call.mem.at<double>(at_sub);
    uint32_t* d_units = call.mem.at<uint32_t>(at_units);
    uint8_t* d_rgb = call.mem.at<uint8_t>(at_rgb);
    uint64_t* d_seeds = call.mem.at<uint64_t>(at_seeds);
    hipError_t e = hipMemcpyAsync(d_units, words.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, call.cs.st);
    if (e == hipSuccess) e = seeds_upload(d_seeds, seeds, n_seeds, h_seeds, call.cs.st);
    if (e != hipSuccess) return oom_or_hip(e, who);
    rc = render_units_enqueue(const_cast<rt_scene*>(scene), p, {d_units, units, d_seeds}, rgb_out ? d_rgb : nullptr, d_sub,
                              call.cs.st, call.mirror.dev, &call.ps, path, kBatchRender);
    return call.finish(who, rc, {{rgb_out, d_rgb, n * 3}, {sub_out, d_sub, b_sub}});
}

int rt_render_pixel_passes(const rt_scene* scene, const rt_render_params* p, const uint32_t* pixels, const uint8_t* counts,
                           int64_t n_pixels, const uint64_t* seeds, int32_t n_seeds, uint8_t* rgb_out, double* sub_out,
                           const volatile int32_t* cancel, rt_render_stats* stats) {
    return rt_render_pixel_passes_with(scene, p, pixels, counts, n_pixels, seeds, n_seeds, RT_LIST_AUTO, rgb_out, sub_out,
                                       cancel, stats);
}

int rt_render_pixel_passes_with_device(const rt_scene* scene, const rt_render_params* p, const void* d_pixels,
                                       const void* d_counts, int64_t n_pixels, int64_t units, const uint64_t* seeds,
                                       int32_t n_seeds, int32_t path, void* d_rgb, void* d_sub, void* stream,
                                       rt_render_stats* stats) {
    const char* who = "rt_render_pixel_passes_device";
    int rc = check_passes(who, scene, p, d_pixels, d_counts, n_pixels, seeds, n_seeds);
    if (rc == RT_OK && (units < n_pixels || units > n_pixels * n_seeds || units > (int64_t)p->width * p->height))
        rc = fail(RT_E_INVAL, std::string(who) + ": units must be the sum of the counts, at most width * height");
    int family;
    if (rc == RT_OK) rc = list_family_of(who, scene, p, units, path, &family);
    if (rc != RT_OK) return rc;
    if (n_pixels == 0) return empty_list(stats);
    rc = need_device(who, p->device);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    uint64_t h_seeds[RT_PASSES_MAX];
    DeviceBlock mem;
    const size_t at_units = mem.part((size_t)units * sizeof(uint32_t)), at_runs = mem.part(rt::runs_scratch_bytes((long)n_pixels)),
                 at_total = mem.part(16), at_seeds = mem.part(sizeof h_seeds);
    hipError_t e = mem.alloc();
    if (e != hipSuccess) return oom_or_hip(e, who);
    PendingStats ps;
    ps.out = stats;
    e = seeds_upload(mem.at<uint64_t>(at_seeds), seeds, n_seeds, h_seeds, st);
    if (e == hipSuccess)
        e = rt::launch_accum_expand((const uint32_t*)d_pixels, (const uint8_t*)d_counts, (long)n_pixels, mem.at<void>(at_runs),
                                    nullptr, mem.at<uint32_t>(at_units), (long)units, mem.at<uint32_t>(at_total), st);
    if (e != hipSuccess) rc = fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    if (rc == RT_OK)
        rc = render_units_enqueue(const_cast<rt_scene*>(scene), p, {mem.at<uint32_t>(at_units), units, mem.at<uint64_t>(at_seeds)},
                                  (uint8_t*)d_rgb, (double*)d_sub, st, nullptr, stats ? &ps : nullptr, path, kBatchRender);
    // the call's scratch lives until the render is done: this form always waits
    e = hipStreamSynchronize(st);
    if (rc == RT_OK && e != hipSuccess) rc = fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return stats_sync(rc, st, stats ? &ps : nullptr);
}

int rt_render_pixel_passes_device(const rt_scene* scene, const rt_render_params* p, const void* d_pixels,
                                  const void* d_counts, int64_t n_pixels, int64_t units, const uint64_t* seeds,
                                  int32_t n_seeds, void* d_rgb, void* d_sub, void* stream, rt_render_stats* stats) {
    return rt_render_pixel_passes_with_device(scene, p, d_pixels, d_counts, n_pixels, units, seeds, n_seeds, RT_LIST_AUTO,
                                              d_rgb, d_sub, stream, stats);
}

int rt_accum_plan_device(void* accum, float abs_tol, float rel_tol, int32_t max_n, int32_t n, float gain, int32_t max_passes,
                         void* d_pixels, void* d_counts, int64_t cap, int64_t* n_out, int64_t* units_out,
                         int64_t* passes_out, void* stream) {
    const char* who = "rt_accum_plan_device";
    rt_accum* a = (rt_accum*)accum;
    int rc = plan_begin(who, a, abs_tol, rel_tol, n, gain, max_passes, d_pixels && d_counts, cap, n_out);
    if (rc != RT_OK) return rc;
    int64_t res[3];
    rc = plan_run(who, a, abs_tol, rel_tol, max_n, n, gain, max_passes, (uint32_t*)d_pixels, (uint8_t*)d_counts, cap, res,
                  (hipStream_t)stream);
    if (rc != RT_OK) return rc;
    plan_result(res, n_out, units_out, passes_out);
    return RT_OK;
}

int rt_accum_plan(void* accum, float abs_tol, float rel_tol, int32_t max_n, int32_t n, float gain, int32_t max_passes,
                  uint32_t* pixels_out, uint8_t* counts_out, int64_t cap, int64_t* n_out, int64_t* units_out,
                  int64_t* passes_out) {
    const char* who = "rt_accum_plan";
    rt_accum* a = (rt_accum*)accum;
    int rc = plan_begin(who, a, abs_tol, rel_tol, n, gain, max_passes, pixels_out && counts_out, cap, n_out);
    if (rc != RT_OK) return rc;
    CallStream cs;
    HIP_TRY(cs.init());
    const int64_t dcap = std::min<int64_t>(cap, (int64_t)a->npix());
    int64_t res[3];
    rc = plan_run(who, a, abs_tol, rel_tol, max_n, n, gain, max_passes, a->adapt_list(), a->batch_counts(), dcap, res, cs.st);
    if (rc != RT_OK) return rc;
    plan_result(res, n_out, units_out, passes_out);
    const int64_t m = std::min(res[0], dcap);
    if (m > 0) {
        HIP_TRY(hipMemcpy(pixels_out, a->adapt_list(), (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(counts_out, a->batch_counts(), (size_t)m, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

int rt_accum_add_passes(void* accum, const rt_scene* scene, const rt_render_params* p, const uint64_t* seeds,
                        int32_t n_seeds, const uint32_t* pixels, const uint8_t* counts, int64_t n_pixels,
                        const volatile int32_t* cancel, rt_render_stats* stats) {
    const char* who = "rt_accum_add_passes";
    rt_accum* a = (rt_accum*)accum;
    int rc = check_accum_add(a, scene, p);
    if (rc == RT_OK) rc = check_passes(who, scene, p, pixels, counts, n_pixels, seeds, n_seeds);
    if (rc == RT_OK) rc = check_pixel_list(who, pixels, n_pixels, (int64_t)a->npix());
    int64_t units = 0;
    if (rc == RT_OK) rc = check_pass_counts(who, counts, n_pixels, n_seeds, (int64_t)a->npix(), &units);
    if (rc == RT_OK) rc = check_sparse(who, a, pixels, n_pixels, false);  // (K >= 2, asked for last)
    if (rc != RT_OK) return rc;
    if (n_pixels == 0) return empty_list(stats);
    rc = batch_ready(who, a);
    if (rc != RT_OK) return rc;
    uint64_t h_seeds[RT_PASSES_MAX];
    RenderCall call;
    rc = call.init(who, cancel, stats);
    if (rc != RT_OK) return rc;
    hipStream_t st = call.cs.st;
    hipError_t e = hipMemcpyAsync(a->adapt_list(), pixels, (size_t)n_pixels * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(a->batch_counts(), counts, (size_t)n_pixels, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = seeds_upload(a->batch_seeds(), seeds, n_seeds, h_seeds, st);
    if (e != hipSuccess) return oom_or_hip(e, who);
    return batch_render_merge(who, a, scene, p, n_pixels, units, call);
}

int rt_accum_refine(void* accum, const rt_scene* scene, const rt_render_params* p, float abs_tol, float rel_tol,
                    int32_t max_n, float gain, const uint64_t* seeds, int32_t n_seeds, const volatile int32_t* cancel,
                    rt_render_stats* stats, int64_t out[3]) {
    const char* who = "rt_accum_refine";
    rt_accum* a = (rt_accum*)accum;
    int rc = check_accum_add(a, scene, p);
    if (rc == RT_OK) rc = check_passes(who, scene, p, nullptr, nullptr, 0, seeds, n_seeds);
    if (rc == RT_OK) rc = check_plan(who, a, abs_tol, rel_tol, p->spp / 4, gain, n_seeds);
    if (rc == RT_OK) rc = check_plan_passes(who, a);
    if (rc == RT_OK) rc = batch_ready(who, a);
    if (rc != RT_OK) return rc;
    uint64_t h_seeds[RT_PASSES_MAX];
    RenderCall call;
    rc = call.init(who, cancel, stats);
    if (rc != RT_OK) return rc;
    hipStream_t st = call.cs.st;
    int64_t res[3];
    rc = plan_run(who, a, abs_tol, rel_tol, max_n, p->spp / 4, gain, n_seeds, a->adapt_list(), a->batch_counts(),
                  (int64_t)a->npix(), res, st);
    if (rc != RT_OK) return rc;
    if (out) plan_result(res, &out[0], &out[1], &out[2]);
    if (res[0] == 0) return empty_list(stats);  // an empty plan launches nothing
    const hipError_t e = seeds_upload(a->batch_seeds(), seeds, n_seeds, h_seeds, st);
    if (e != hipSuccess) return oom_or_hip(e, who);
    return batch_render_merge(who, a, scene, p, res[0], res[1], call);
}

}  // extern "C"
