// C ABI (include/rt_ffi.h): frame renders on one device and on several, ray tracing, and what every render shares:
// the workspace pool, the kernels' arguments, the split-tail scratch and render_enqueue.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>

#include "../ab_knobs.h"
#include "api_common.hpp"

using namespace rt::api;

namespace rt::api {

std::unique_ptr<rt::Workspace> take_workspace(rt_scene* s, int device, hipStream_t st, hipError_t* err) {
    std::lock_guard<std::mutex> lk(s->mu);
    size_t idle = s->pool.size(), same = s->pool.size();
    for (size_t i = 0; i < s->pool.size(); ++i) {
        rt::Workspace& w = *s->pool[i];
        if (w.device != device) continue;
        if (!w.in_flight || hipEventQuery(w.busy) == hipSuccess) {
            idle = i;
            break;
        }
        if (w.last_stream == st && same == s->pool.size()) same = i;
    }
    (void)hipGetLastError();  // hipErrorNotReady from the queries is not an error
    *err = hipSuccess;
    const size_t pick = idle < s->pool.size() ? idle : same;
    if (pick < s->pool.size()) {
        std::unique_ptr<rt::Workspace> w = std::move(s->pool[pick]);
        s->pool.erase(s->pool.begin() + pick);
        if (pick == idle) {
            w->in_flight = false;
        } else {
            *err = hipStreamWaitEvent(st, w->busy, 0);
            if (*err != hipSuccess) {  // keep it pooled; the caller fails the render
                s->pool.push_back(std::move(w));
                return nullptr;
            }
        }
        return w;
    }
    auto w = std::make_unique<rt::Workspace>();
    w->device = device;
    return w;
}
void give_workspace(rt_scene* s, std::unique_ptr<rt::Workspace> w, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (!w->busy) e = hipEventCreateWithFlags(&w->busy, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(w->busy, st);
    if (e != hipSuccess) {  // cannot track its completion: wait for it here
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);
        w->in_flight = false;
    } else {
        w->in_flight = true;
        w->last_stream = st;
    }
    std::lock_guard<std::mutex> lk(s->mu);
    s->pool.push_back(std::move(w));
}

rt::RenderArgs make_render_args(const rt_scene* s, const rt_render_params* p) {
    const Packed& sp = s->packed;
    rt::RenderArgs a{};
    a.width = p->width;
    a.height = p->height;
    a.x0 = p->x0;
    a.y0 = p->y0;
    a.row_step = p->row_step > 1 ? p->row_step : 1;
    a.tw = p->tile_w;
    a.th = p->tile_h;
    a.n_samples = p->spp > 0 ? p->spp / 4 : 0;  // server.rs:332 (i32 division)
    a.mis = (p->flags & RT_FLAG_MIS) ? 1 : 0;
    a.features = (s->host.meshes.empty() ? 0 : 1) | (sp.phong ? 2 : 0) | (a.mis ? 4 : 0) | (sp.compact ? 8 : 0) |
                 (sp.spec ? 0 : 32);
    if ((p->flags & RT_FLAG_MESH_NEAREST) && !s->host.meshes.empty()) a.features |= 16;
    a.mesh_nodes = sp.mesh_nodes;
    a.all_flat = sp.all_flat;
    a.seed = p->seed;
    rt::host::camera_frame(s->cam_dir, s->cam_right, s->cam_fov, p->width, p->height, a.cx, a.cy);
    a.inv_n = a.n_samples > 0 ? 1. / (double)a.n_samples : 0.0;
    return a;
}

hipError_t finalize_rgb(int32_t width, int32_t height, const double* d_sub, uint8_t* d_rgb, hipStream_t st) {
    rt::RenderArgs a{};
    a.tw = width;
    a.th = height;
    a.rgb_out = d_rgb;
    return rt::launch_finalize_f64(a, d_sub, st);
}

void ensure_tail_scratch(rt::Workspace* ws, const rt::RenderArgs& a, size_t npix) {
    const bool walk = (a.features & 1) && !a.all_flat;
    int dev = 0, ncu = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    const size_t per_sub = rt::tail_scratch_per_subpixel(a.n_samples);
    // (A/B builds: RT_MK_TAIL_SCRATCH_PER_CU / RT_MK_TAIL_SCRATCH_MB override both bounds, ab_knobs.h)
    const long ncu_lanes = (long)std::max(ncu, 1) * 1024;
    const size_t per_cu = (size_t)rt::ab_knob("RT_MK_TAIL_SCRATCH_PER_CU",
                                              walk ? 6 * 1024 : 512 * rt::tail_split_x2((long)npix * 4, ncu_lanes));
    const size_t cap = (size_t)rt::ab_knob("RT_MK_TAIL_SCRATCH_MB", 3072) << 20;
    const size_t want = std::min<size_t>(cap, per_sub * std::min<size_t>(npix * 4, (size_t)std::max(ncu, 1) * per_cu));
    if (per_sub > 0 && want >= per_sub) {
        if (ws->ensure_tail(want) != hipSuccess) (void)hipGetLastError();  // no tail split then
    }
}

int render_enqueue(rt_scene* s, const rt_render_params* p, uint8_t* d_rgb, double* d_sub, hipStream_t st,
                   const int32_t* dcancel, const volatile int32_t* host_cancel, PendingStats* ps) {
    int rc = check_params(p);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    rt::DevScene ds;
    rc = upload(s, p->device, &ds);
    if (rc != RT_OK) return rc;
    rt::RenderArgs a = make_render_args(s, p);
    a.sub_out = d_sub;
    a.rgb_out = d_rgb;
    const bool fp32 = (p->flags & RT_FLAG_FP32) != 0;
    if (fp32) {
        // the f32 kernel covers diffuse / mirror BRDFs and sphere lights (every reference scene)
        if (s->packed.phong) return fail(RT_E_INVAL, "RT_FLAG_FP32: Phong BRDFs need the f64 path");
        const auto& L = s->packed.objects;
        if (ds.light >= 0 && ds.light < (int32_t)L.size() && L[ds.light].geom != rt::GEOM_SPHERE)
            return fail(RT_E_INVAL, "RT_FLAG_FP32: only sphere lights (mesh lights need the f64 path)");
    }
    if (!fp32 && (p->flags & RT_FLAG_MESH_NEAREST) && !(p->flags & RT_FLAG_MEGAKERNEL))
        return fail(RT_E_INVAL, "RT_FLAG_MESH_NEAREST needs RT_FLAG_MEGAKERNEL");
    const bool mk = fp32 || (p->flags & RT_FLAG_MEGAKERNEL);
    if (ps) {
        const hipError_t e = ps->init(ps->out);
        if (e != hipSuccess) return fail(RT_E_HIP, std::string("stats: ") + hipGetErrorString(e));
        ps->samples = (int64_t)p->tile_w * p->tile_h * 4 * (int64_t)a.n_samples;
        HIP_TRY(hipEventRecord(ps->e0, st));
    }
    hipError_t te;
    std::unique_ptr<rt::Workspace> ws = take_workspace(s, p->device, st, &te);
    if (!ws) return fail(RT_E_HIP, std::string("workspace: ") + hipGetErrorString(te));
    int out = RT_OK;
    std::string err;
    if (mk) {
        const size_t npix = (size_t)p->tile_w * p->tile_h;
        a.cancel = dcancel;
        hipError_t e = ws->ensure_counters();
        double* sub = d_sub;
        if (e == hipSuccess && !sub) {
            e = ws->ensure_sub(npix);
            sub = ws->sub_buf;
        }
        if (e == hipSuccess && ps) e = hipMemsetAsync(ws->counters, 0, 8 * sizeof(unsigned long long), st);
        if (e == hipSuccess && a.n_samples <= 0) e = hipMemsetAsync(sub, 0, npix * 12 * sizeof(double), st);
        if (e == hipSuccess) {
            a.counters = ps ? ws->counters : nullptr;
            if (!fp32) ensure_tail_scratch(ws.get(), a, npix);
            if (fp32) {
                static const int brute = (int)rt::ab_knob("RT_F32_BRUTE", 16);
                a.f32_brute = brute;
                e = rt::launch_megakernel_f32(ds, a, sub, (uint32_t*)(ws->counters + 4), st);
            } else {
                e = rt::launch_megakernel_f64(ds, a, sub, (uint32_t*)(ws->counters + 4), ws->tail_buf, ws->tail_cap, st);
            }
        }
        if (e == hipSuccess) e = rt::launch_finalize_f64(a, sub, st);
        if (e == hipSuccess && ps) e = hipEventRecord(ps->e1, st);
        if (e == hipSuccess && ps) e = hipMemcpyAsync(ps->count, ws->counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) { out = RT_E_HIP; err = std::string("megakernel: ") + hipGetErrorString(e); }
    } else {
        out = rt::wavefront_render_f64(ds, a, *ws, st, host_cancel, ps ? ps->out : nullptr, &err);
        if (ps && out >= 0) {
            hipError_t e = hipEventRecord(ps->e1, st);
            if (e == hipSuccess) e = hipEventSynchronize(ps->e1);
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, ps->e0, ps->e1);
            if (e != hipSuccess && out == RT_OK) { out = RT_E_HIP; err = std::string("stats: ") + hipGetErrorString(e); }
            ps->out->device_ms = ms;
            ps->device_done = true;
        }
    }
    give_workspace(s, std::move(ws), st);
    if (out < 0) return fail(out, err);
    return out;
}

}  // namespace rt::api

extern "C" {

int rt_render_device(const rt_scene* scene, const rt_render_params* params, void* d_rgb, void* d_sub, void* stream,
                     rt_render_stats* stats) {
    if (!scene || !d_rgb) return fail(RT_E_INVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    PendingStats ps;
    ps.out = stats;
    const int rc = render_enqueue(const_cast<rt_scene*>(scene), params, (uint8_t*)d_rgb, (double*)d_sub, st, nullptr,
                                  nullptr, stats ? &ps : nullptr);
    return stats_sync(rc, st, stats ? &ps : nullptr);
}

int rt_render(const rt_scene* scene, const rt_render_params* p, uint8_t* rgb_out, double* sub_out,
              const volatile int32_t* cancel, rt_render_stats* stats) {
    if (!scene || !rgb_out) return fail(RT_E_INVAL, "null argument");
    int rc = check_params(p);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    const size_t npix = (size_t)p->tile_w * p->tile_h;
    if (npix == 0) return RT_OK;
    RenderCall call;
    const size_t b_sub = npix * 12 * sizeof(double);
    const size_t at_sub = call.mem.part(sub_out ? b_sub : 0), at_rgb = call.mem.part(npix * 3);
    rc = call.init("rt_render", cancel, stats);
    if (rc != RT_OK) return rc;
    uint8_t* d_rgb = call.mem.at<uint8_t>(at_rgb);
    double* d_sub = sub_out ? call.mem.at<double>(at_sub) : nullptr;
    rc = render_enqueue(const_cast<rt_scene*>(scene), p, d_rgb, d_sub, call.cs.st, call.mirror.dev, cancel, &call.ps);
    return call.finish("rt_render", rc, {{rgb_out, d_rgb, npix * 3}, {sub_out, d_sub, b_sub}});
}

int32_t rt_band_plan(int32_t tile_h, int32_t n_workers, int32_t band_rows, int32_t cap, int32_t* first_row,
                     int32_t* rows) {
    if (tile_h <= 0) return 0;
    if (n_workers < 1) n_workers = 1;
    int32_t b = band_rows;
    if (b <= 0) b = std::max<int32_t>(1, (int32_t)(((int64_t)tile_h + 8LL * n_workers - 1) / (8LL * n_workers)));
    const int32_t n = (int32_t)(((int64_t)tile_h + b - 1) / b);
    for (int32_t i = 0; i < n && i < cap; ++i) {
        if (first_row) first_row[i] = i * b;
        if (rows) rows[i] = std::min(b, tile_h - i * b);
    }
    return n;
}

int rt_render_multi(const rt_scene* scene, const rt_render_params* p, const int32_t* devices, int32_t n_devices,
                    int32_t band_rows, uint8_t* rgb_out, const volatile int32_t* cancel, rt_render_stats* stats) {
    if (!scene || !rgb_out || !devices || n_devices <= 0) return fail(RT_E_INVAL, "null argument");
    int rc = check_params(p);
    if (rc != RT_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {  // no GPU or no runtime: not the caller's error
        (void)hipGetLastError();
        return fail(RT_E_NODEVICE, "rt_render_multi: no HIP device visible");
    }
    // an ordinal no visible device has is the caller's error (RT_E_INVAL), checked before anything runs
    for (int32_t i = 0; i < n_devices; ++i)
        if (devices[i] < 0 || devices[i] >= ndev)
            return fail(RT_E_INVAL, "device ordinal " + std::to_string(devices[i]) + " out of range (" +
                                        std::to_string(ndev) + " HIP devices visible)");
    const int32_t tw = p->tile_w, th = p->tile_h;
    if ((size_t)tw * th == 0) return RT_OK;
    const int32_t nb = rt_band_plan(th, n_devices, band_rows, 0, nullptr, nullptr);
    std::vector<int32_t> first(nb), rows(nb);
    rt_band_plan(th, n_devices, band_rows, nb, first.data(), rows.data());
    int32_t bmax = 0;
    for (int32_t r : rows) bmax = std::max(bmax, r);
    const int64_t step = p->row_step > 1 ? p->row_step : 1;
    std::atomic<int32_t> next{0};
    std::atomic<int> err_code{RT_OK};
    std::atomic<bool> stop{false};
    std::atomic<int64_t> samples{0}, vertices{0};
    std::atomic<int32_t> done{0};
    std::mutex err_mu;
    std::string err_msg;
    const auto t0 = std::chrono::steady_clock::now();
    rt_scene* s = const_cast<rt_scene*>(scene);

    // one device-visible cancel word for every band of the call (the megakernels poll it between
    // subpixels; each worker copies the caller's flag into it while it waits for a band)
    CancelMirror mirror;
    if (cancel) {
        const hipError_t e = mirror.init();
        if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_render_multi: cancel word: ") + hipGetErrorString(e));
    }

    auto worker = [&](int32_t dev) {
        auto record = [&](int code, const std::string& m) {
            std::lock_guard<std::mutex> lk(err_mu);
            if (err_code.load() == RT_OK) { err_code = code; err_msg = m; }
            stop = true;
        };
        if (hipSetDevice(dev) != hipSuccess) { record(RT_E_HIP, "hipSetDevice"); return; }
        constexpr int kSlots = 2;  // bands in flight per worker
        hipStream_t st[kSlots] = {nullptr, nullptr};
        uint8_t* d_rgb[kSlots] = {nullptr, nullptr};
        uint8_t* h_rgb[kSlots] = {nullptr, nullptr};
        int32_t pending[kSlots] = {-1, -1};
        rt_render_stats bs[kSlots];
        PendingStats ps[kSlots];
        const size_t band_bytes = (size_t)bmax * tw * 3;
        bool ok = true;
        for (int k = 0; k < kSlots && ok; ++k) {
            ok = hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking) == hipSuccess &&
                 hipMalloc(&d_rgb[k], band_bytes) == hipSuccess &&
                 hipHostMalloc((void**)&h_rgb[k], band_bytes, hipHostMallocDefault) == hipSuccess;
        }
        if (!ok) record(RT_E_OOM, "rt_render_multi: band buffers");
        // finishes band slot k: wait for its copy (relaying the cancel flag), collect its stats, put its
        // rows into the caller's frame
        auto drain = [&](int k) {
            if (pending[k] < 0) return;
            const int32_t b = pending[k];
            pending[k] = -1;
            if (wait_stream(st[k], cancel, &mirror) != hipSuccess) { record(RT_E_HIP, "rt_render_multi: band sync"); return; }
            if (stats) {
                std::string e;
                if (ps[k].finish(&e) < 0) { record(RT_E_HIP, "rt_render_multi: " + e); return; }
                samples += bs[k].samples;
                vertices += bs[k].vertices;
            }
            std::memcpy(rgb_out + (size_t)first[b] * tw * 3, h_rgb[k], (size_t)rows[b] * tw * 3);
            ++done;
        };
        for (int slot = 0; ok && !stop.load(); slot ^= 1) {
            drain(slot);
            if (stop.load() || (cancel && *cancel)) break;
            const int32_t b = next.fetch_add(1);
            if (b >= nb) break;
            rt_render_params q = *p;
            q.device = dev;
            q.y0 = (int32_t)(p->y0 + (int64_t)first[b] * step);
            q.tile_h = rows[b];
            ps[slot].out = &bs[slot];
            const int r = render_enqueue(s, &q, d_rgb[slot], nullptr, st[slot], mirror.dev, cancel, stats ? &ps[slot] : nullptr);
            if (r < 0) { record(r, rt_last_error()); break; }  // this worker thread's own message
            if (hipMemcpyAsync(h_rgb[slot], d_rgb[slot], (size_t)rows[b] * tw * 3, hipMemcpyDeviceToHost, st[slot]) !=
                hipSuccess) { record(RT_E_HIP, "rt_render_multi: band copy"); break; }
            pending[slot] = b;
        }
        for (int k = 0; k < kSlots; ++k) drain(k);
        for (int k = 0; k < kSlots; ++k) {
            if (st[k]) (void)hipStreamSynchronize(st[k]);
            if (d_rgb[k]) (void)hipFree(d_rgb[k]);
            if (h_rgb[k]) (void)hipHostFree(h_rgb[k]);
            if (st[k]) (void)hipStreamDestroy(st[k]);
        }
    };
    std::vector<std::thread> pool;
    for (int32_t i = 0; i < n_devices; ++i) pool.emplace_back(worker, devices[i]);
    for (auto& t : pool) t.join();
    if (err_code.load() != RT_OK) return fail(err_code.load(), err_msg);
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->samples = samples.load();
        stats->vertices = vertices.load();
        stats->device_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->kernel_launches[0] = nb;
    }
    // only a cancel leaves bands unrendered without an error; a band whose kernel saw the cancel word
    // stopped handing out subpixels early
    if (done.load() < nb || (cancel && *cancel)) return RT_CANCELLED;
    return RT_OK;
}

int rt_trace_rays(const rt_scene* scene, int32_t device, int64_t n, const double* origins, const double* dirs, double* t,
                  int32_t* object, double* pos, double* normal) {
    return rt_trace_rays_flags(scene, device, 0u, n, origins, dirs, t, object, pos, normal);
}

int rt_trace_rays_flags(const rt_scene* scene, int32_t device, uint32_t flags, int64_t n, const double* origins,
                        const double* dirs, double* t, int32_t* object, double* pos, double* normal) {
    if (!scene || n < 0 || (n && (!origins || !dirs || !t || !object))) return fail(RT_E_INVAL, "null argument");
    if (n == 0) return RT_OK;
    HIP_TRY(hipSetDevice(device));
    rt::DevScene ds;
    int rc = upload(const_cast<rt_scene*>(scene), device, &ds);
    if (rc != RT_OK) return rc;
    const size_t v3 = (size_t)n * 3 * sizeof(double);
    DeviceBlock buf;
    const size_t at_o = buf.part(v3), at_d = buf.part(v3), at_pos = buf.part(v3), at_n = buf.part(v3);
    const size_t at_t = buf.part((size_t)n * sizeof(double)), at_id = buf.part((size_t)n * sizeof(int32_t));
    hipError_t e = buf.alloc();
    if (e != hipSuccess) return oom_or_hip(e, "rt_trace_rays buffers");
    double *d_o = buf.at<double>(at_o), *d_d = buf.at<double>(at_d), *d_pos = buf.at<double>(at_pos);
    double *d_n = buf.at<double>(at_n), *d_t = buf.at<double>(at_t);
    int32_t* d_id = buf.at<int32_t>(at_id);
    e = hipMemcpy(d_o, origins, v3, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_d, dirs, v3, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = rt::launch_trace_f64(ds, (long)n, d_o, d_d, d_t, d_id, d_pos, d_n, (flags & RT_FLAG_MESH_NEAREST) != 0, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(t, d_t, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(object, d_id, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && pos) e = hipMemcpy(pos, d_pos, v3, hipMemcpyDeviceToHost);
    if (e == hipSuccess && normal) e = hipMemcpy(normal, d_n, v3, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_trace_rays: ") + hipGetErrorString(e));
    return RT_OK;
}

}  // extern "C"
