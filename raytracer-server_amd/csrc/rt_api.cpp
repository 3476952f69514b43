// C ABI (include/rt_ffi.h): per-device upload of the packed scene (host/scene_pack.hpp), render dispatch, error
// reporting.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt_diag.h"
#include "../../include/rt_ffi.h"
#include "ab_knobs.h"
#include "host/scene_pack.hpp"
#include "kernels/accum.h"
#include "kernels/denoise.h"
#include "kernels/kernels.h"
#include "kernels/reproject.h"
#include "kernels/wavefront.h"

namespace {

using rt::host::Packed;

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// A failed HIP call as a return code: RT_E_OOM when the device is out of memory, RT_E_HIP otherwise.
int oom_or_hip(hipError_t e, const std::string& what) {
    return fail(e == hipErrorOutOfMemory ? RT_E_OOM : RT_E_HIP, what + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                       \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) return oom_or_hip(e_, #expr); \
    } while (0)

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct DeviceCopy {
    bool ready = false;
    void* blob = nullptr;
    rt::DevScene ds{};
};

}  // namespace

// What a loaded or created scene owns and its views share: host data, packed tables, device uploads, workspaces.
struct SceneData {
    rt::host::Scene host;
    Packed packed;
    std::mutex mu;
    std::vector<DeviceCopy> dev;
    std::vector<std::unique_ptr<rt::Workspace>> pool;  // free wavefront workspaces, per device tagged
    ~SceneData() {
        for (auto& d : dev)
            if (d.blob) (void)hipFree(d.blob);
        pool.clear();
    }
};

// A scene handle: the data (its own, or for a view, rt_scene_view, the root base's) and a camera. The members below
// refer to the root's data, so every entry point reads a view as it reads a scene; only the camera is the handle's.
struct rt_scene {
    std::unique_ptr<SceneData> own;  // null in a view
    const rt_scene* root;            // the handle that owns the data (this, unless a view)
    rt::host::Scene& host;
    Packed& packed;
    std::mutex& mu;
    std::vector<DeviceCopy>& dev;
    std::vector<std::unique_ptr<rt::Workspace>>& pool;
    double cam_pos[3] = {0, 0, 0}, cam_dir[3] = {0, 0, 1}, cam_right[3] = {1, 0, 0};
    double cam_fov = 0.5135;  // server.rs:330
    rt_scene()
        : own(new SceneData), root(this), host(own->host), packed(own->packed), mu(own->mu), dev(own->dev),
          pool(own->pool) {}
    explicit rt_scene(const rt_scene* base)  // a view of base (of base's root, when base is a view itself)
        : root(base->root), host(base->host), packed(base->packed), mu(base->mu), dev(base->dev), pool(base->pool) {}
};

namespace {

// The host image of a scene blob. put() appends one table (at a 256-byte boundary, with 16 bytes of slack) and notes
// the DevScene pointer it backs; binds set those pointers once the blob's device address is known. So every table is
// named once, and the order of the put() calls is the blob's layout.
struct BlobImage {
    std::vector<char> bytes;
    std::vector<std::function<void(char*)>> binds;
    template <class T>
    void put(const T** slot, const T* v, size_t n) {
        const size_t off = align_up(bytes.size(), 256);
        bytes.resize(off + n * sizeof(T) + 16);
        if (n) std::memcpy(bytes.data() + off, v, n * sizeof(T));
        binds.push_back([slot, off](char* base) { *slot = (const T*)(base + off); });
    }
};

int upload(rt_scene* s, int device, rt::DevScene* out) {
    std::lock_guard<std::mutex> lk(s->mu);
    if ((int)s->dev.size() <= device) s->dev.resize(device + 1);
    DeviceCopy& dc = s->dev[device];
    if (!dc.ready) {
        const Packed& p = s->packed;
        rt::DevScene ds{};
        BlobImage blob;
        blob.put(&ds.ctab, &p.ctab, 1);
        blob.put(&ds.ctab32, &p.ctab32, 1);
        blob.put(&ds.objects, p.objects.data(), p.objects.size());
        blob.put(&ds.meshes, p.meshes.data(), p.meshes.size());
        blob.put(&ds.node_kids, p.kids.data(), p.kids.size());
        blob.put(&ds.node_up, p.up.data(), p.up.size());
        blob.put(&ds.leaf_span, p.leaves.data(), p.leaves.size());
        blob.put(&ds.ltris, p.ltris.data(), p.ltris.size());
        blob.put(&ds.ltri_id, p.ltri_id.data(), p.ltri_id.size());
        blob.put(&ds.tris, p.tris.data(), p.tris.size());
        blob.put(&ds.tri_cum_area, p.cum_area.data(), p.cum_area.size());
        blob.put(&ds.bvh, p.bvh.data(), p.bvh.size());
        blob.put(&ds.btris, p.btris.data(), p.btris.size());
        blob.put(&ds.btri_id, p.btri_id.data(), p.btri_id.size());
        blob.put(&ds.obj32, p.obj32.data(), p.obj32.size());
        blob.put(&ds.bvh32, p.bvh32.data(), p.bvh32.size());
        blob.put(&ds.btris32, p.btris32.data(), p.btris32.size());
        blob.put(&ds.node_slot, p.slots.data(), p.slots.size());
        blob.put(&ds.node_box, p.node_box.data(), p.node_box.size());
        blob.put(&ds.pid_up, p.pid_up.data(), p.pid_up.size());
        void* d = nullptr;
        HIP_TRY(hipMalloc(&d, blob.bytes.size()));
        hipError_t e = hipMemcpy(d, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail(RT_E_HIP, std::string("scene upload: ") + hipGetErrorString(e));
        }
        for (const auto& bind : blob.binds) bind((char*)d);
        if (p.slots.empty()) {  // the node_kids walk: no slot tables
            ds.node_slot = nullptr;
            ds.node_box = nullptr;
            ds.pid_up = nullptr;
        }
        ds.n_pid = p.slots.empty() ? 0 : (int32_t)p.pid_up.size();
        // RT_TEST_ANC_OFF (tests only): report more pids than a 16-bit ancestor column holds, so the role
        // pool's walkers pop through pid_up (the path of octrees with > 65536 parents)
        if (std::getenv("RT_TEST_ANC_OFF") && ds.n_pid > 0) ds.n_pid = 0x7FFFFFFF;
        ds.n_objects = (int32_t)p.objects.size();
        ds.n_meshes = (int32_t)p.meshes.size();
        ds.off32 = p.off32;
        ds.compact = p.compact;
        ds.light = s->host.light;
        ds.light_pdf = p.light_pdf;
        dc.blob = d;
        dc.ds = ds;
        dc.ready = true;
    }
    *out = dc.ds;
    // the camera is the handle's own (a view shares everything else): the kernels read it from this kernarg copy
    std::memcpy(out->cam_pos, s->cam_pos, sizeof out->cam_pos);
    std::memcpy(out->cam_dir, s->cam_dir, sizeof out->cam_dir);
    return RT_OK;
}

int check_params(const rt_render_params* p) {
    if (!p) return fail(RT_E_INVAL, "null params");
    if (p->width <= 0 || p->height <= 0) return fail(RT_E_INVAL, "width/height must be positive");
    if (p->row_step < 0) return fail(RT_E_INVAL, "row_step must be >= 0");
    const int64_t step = p->row_step > 1 ? p->row_step : 1;
    if (p->tile_w < 0 || p->tile_h < 0 || p->x0 < 0 || p->y0 < 0 || p->x0 + p->tile_w > p->width ||
        (p->tile_h > 0 && p->y0 + (int64_t)(p->tile_h - 1) * step >= p->height))
        return fail(RT_E_INVAL, "tile outside the image");
    if ((int64_t)p->width * p->height > (int64_t)UINT32_MAX) return fail(RT_E_INVAL, "image too large for 32-bit pixel ids");
    return RT_OK;
}

// Per-render scratch (ticket counter, subpixel buffer, split-tail buffer, wavefront streams) comes
// from a per-scene pool. rt_render_device returns before its kernels finish, so a pooled workspace
// may still be in use: an idle one (its completion event has fired) is taken first; else one last
// used on the same stream, with a device-side wait on its completion event enqueued on `st` (so the
// reuse is ordered even if the caller destroyed that stream and HIP handed its handle to a new one);
// otherwise a new workspace is made (concurrent renders on one scene each get their own, rt_ffi.h).
// A reused in-flight workspace never reallocates under its previous kernels: Workspace::ensure_*
// wait for `busy` before freeing (wavefront_f64.hip).
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

// Device-visible mirror of a caller's cancel flag: a pinned, mapped word the megakernels poll
// (RenderArgs::cancel) between subpixels. The caller's flag itself is never registered with HIP (it
// may be shared by concurrent renders, or sit on memory HIP cannot pin): the host thread that waits
// for the render copies it into the mirror (wait_stream), so its lifetime stays the caller's.
// The words come from a process-wide free list and go back to it once the render has drained: a
// cancellable render (the WebSocket server renders chunk by chunk with a flag) costs no pinned
// allocation after the first. The words are never freed (one per concurrently cancellable render).
struct CancelWord {
    int32_t* host;
    int32_t* dev;
};
struct CancelWordPool {
    std::mutex mu;
    std::vector<CancelWord> free;
};
CancelWordPool& cancel_words() {
    static CancelWordPool* pool = new CancelWordPool;  // never destroyed: no HIP calls at process teardown
    return *pool;
}
struct CancelMirror {
    int32_t* host = nullptr;
    int32_t* dev = nullptr;
    CancelMirror() = default;
    CancelMirror(const CancelMirror&) = delete;
    CancelMirror& operator=(const CancelMirror&) = delete;
    ~CancelMirror() {
        if (!host) return;
        CancelWordPool& p = cancel_words();
        std::lock_guard<std::mutex> lk(p.mu);
        p.free.push_back(CancelWord{host, dev});
    }
    hipError_t init() {
        {
            CancelWordPool& p = cancel_words();
            std::lock_guard<std::mutex> lk(p.mu);
            if (!p.free.empty()) {
                host = p.free.back().host;
                dev = p.free.back().dev;
                p.free.pop_back();
            }
        }
        if (!host) {
            // coherent (fine-grained): hipHostMalloc's default is non-coherent memory the GPU may cache, so
            // a host write could stay invisible to the polling kernel until the line is evicted
            hipError_t e = hipHostMalloc((void**)&host, sizeof(int32_t),
                                         hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent);
            if (e != hipSuccess) {
                host = nullptr;
                return e;
            }
            e = hipHostGetDevicePointer((void**)&dev, host, 0);
            if (e != hipSuccess) {
                (void)hipHostFree(host);
                host = nullptr;
                return e;
            }
        }
        __atomic_store_n(host, 0, __ATOMIC_RELEASE);
        return hipSuccess;
    }
    void raise() {
        if (host) __atomic_store_n(host, 1, __ATOMIC_RELEASE);
    }
};

// Waits for everything enqueued on `st`, copying the caller's cancel flag into the mirror meanwhile.
// Polls with a growing pause (10 us doubling to 200 us), so a short render (one WebSocket chunk) is
// seen done within about its own duration.
hipError_t wait_stream(hipStream_t st, const volatile int32_t* cancel, CancelMirror* mirror) {
    if (!cancel || !mirror || !mirror->host) return hipStreamSynchronize(st);
    int us = 10;
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
        if (*cancel) mirror->raise();
        std::this_thread::sleep_for(std::chrono::microseconds(us));
        us = std::min(200, 2 * us);
    }
}

// Statistics of an enqueued megakernel render, completed once its stream has drained (finish): the
// render's HIP events and a pinned copy of the workspace's vertex counter (copied on the stream
// before the workspace goes back to the pool). Nothing here synchronises, so callers can keep several
// renders in flight (rt_render_multi) and still collect their stats. The events and the pinned word
// are made by the first init and reused by later ones (rt_render_multi: one PendingStats per band
// slot of a worker), and freed only when the object goes (after its renders have drained).
struct PendingStats {
    rt_render_stats* out = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    unsigned long long* count = nullptr;  // pinned host word
    int64_t samples = 0;
    bool device_done = false;  // the wavefront path filled `out` itself
    PendingStats() = default;
    PendingStats(const PendingStats&) = delete;
    PendingStats& operator=(const PendingStats&) = delete;
    ~PendingStats() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (count) (void)hipHostFree(count);
    }
    hipError_t init(rt_render_stats* o) {
        out = o;
        std::memset(out, 0, sizeof *out);
        device_done = false;
        hipError_t e = hipSuccess;
        if (!e0) e = hipEventCreate(&e0);
        if (e == hipSuccess && !e1) e = hipEventCreate(&e1);
        if (e == hipSuccess && !count) e = hipHostMalloc((void**)&count, sizeof(unsigned long long), hipHostMallocDefault);
        if (e == hipSuccess) *count = 0;
        return e;
    }
    // after the render's stream has completed
    int finish(std::string* err) {
        if (!out) return RT_OK;
        if (!device_done) {
            float ms = 0.f;
            const hipError_t e = hipEventElapsedTime(&ms, e0, e1);
            if (e != hipSuccess) {
                *err = std::string("stats: ") + hipGetErrorString(e);
                return RT_E_HIP;
            }
            out->device_ms = ms;
            out->kernel_ms[0] = ms;
            out->kernel_launches[0] = 1;
            out->vertices = (int64_t)*count;
        }
        out->samples = samples;
        return RT_OK;
    }
};

// The tail of the _device render forms: with stats, the call is synchronous with respect to the stream (rt_ffi.h).
// rc: what the enqueue returned; ps: null without stats.
int stats_sync(int rc, hipStream_t st, PendingStats* ps) {
    if (rc < 0 || !ps) return rc;
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("stats sync: ") + hipGetErrorString(e));
    std::string err;
    const int f = ps->finish(&err);
    return f < 0 ? fail(f, err) : rc;
}

// Device memory that lives for one call, carved into 16-byte aligned parts: part() every part (its offset comes
// back), alloc() once, at<T>() the parts. The destructor frees it, so no path out of the call has a free of its own;
// declare it before the call's stream (CallStream, whose destructor waits), so the memory outlives the work on it.
struct DeviceBlock {
    char* base = nullptr;
    size_t bytes = 0;
    DeviceBlock() = default;
    DeviceBlock(const DeviceBlock&) = delete;
    DeviceBlock& operator=(const DeviceBlock&) = delete;
    ~DeviceBlock() {
        if (base) (void)hipFree(base);
    }
    size_t part(size_t n) {
        const size_t at = bytes;
        bytes += align_up(n, 16);
        return at;
    }
    hipError_t alloc() {
        const hipError_t e = hipMalloc((void**)&base, bytes);
        if (e != hipSuccess) base = nullptr;
        return e;
    }
    template <class T>
    T* at(size_t off) const { return (T*)(base + off); }
};

// A stream for one call: waited for and destroyed when the call returns.
struct CallStream {
    hipStream_t st = nullptr;
    CallStream() = default;
    CallStream(const CallStream&) = delete;
    CallStream& operator=(const CallStream&) = delete;
    hipError_t init() { return hipStreamCreateWithFlags(&st, hipStreamNonBlocking); }
    // the destructor's work, for a call that ends with copies whose outcome it reports: the one wait of that path
    hipError_t close() {
        if (!st) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
        st = nullptr;
        return e;
    }
    ~CallStream() { (void)close(); }
};

// What a host render call that waits for its render owns (rt_render, rt_render_pixels, rt_accum_add,
// rt_accum_add_pixels, rt_accum_fill). Members go in reverse order, and the order is the rule: the stream goes first,
// and its destructor waits for it, so on every path out of the call nothing enqueued can still write the stats'
// pinned word, poll the cancel word or touch the call's memory when the stats' events are destroyed, the word goes
// back to the pool (where the next render may take it) and the memory is freed.
struct RenderCall {
    DeviceBlock mem;  // the call's device buffers, for a call that has any: part() them before init()
    CancelMirror mirror;
    rt_render_stats local;  // where the stats go when the caller wants none
    PendingStats ps;
    CallStream cs;
    const volatile int32_t* cancel = nullptr;

    // One device-to-host copy of the readback; a null dst is skipped.
    struct Copy {
        void* dst;
        const void* src;
        size_t bytes;
    };

    // The stream, the memory parted so far and, for a cancellable call, the mirror of the caller's flag.
    int init(const char* who, const volatile int32_t* cancel_flag, rt_render_stats* stats) {
        cancel = cancel_flag;
        ps.out = stats ? stats : &local;
        hipError_t e = cs.init();
        if (e == hipSuccess && mem.bytes) e = mem.alloc();
        if (e == hipSuccess && cancel) e = mirror.init();
        return e == hipSuccess ? RT_OK : oom_or_hip(e, who);
    }

    // After render_enqueue / render_units_enqueue on cs.st returned rc: waits for the render while relaying the
    // cancel flag, copies back, completes the stats; RT_CANCELLED when the flag is up by then (the caller merges
    // nothing). An enqueue that failed left its message in g_err, and the stream is drained of whatever it did
    // enqueue before anything it used is released.
    int finish(const char* who, int rc, std::initializer_list<Copy> readback = {}) {
        if (rc != RT_OK) {
            (void)hipStreamSynchronize(cs.st);
            return rc;
        }
        // wait for the render first (relaying the cancel flag), then copy back: a copy into the
        // caller's pageable buffers would block inside hipMemcpyAsync until the kernel ends, with
        // nobody relaying the flag
        hipError_t e = wait_stream(cs.st, cancel, &mirror);
        bool copied = false;
        for (const Copy& c : readback)
            if (e == hipSuccess && c.dst) {
                e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, cs.st);
                copied = true;
            }
        if (e == hipSuccess && copied) e = cs.close();
        if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
        std::string err;
        const int f = ps.finish(&err);
        if (f < 0) return fail(f, err);
        return cancel && *cancel ? RT_CANCELLED : RT_OK;
    }
};

// The kernels' view of `p` on the scene: frame, tile, samples, seed, camera frame and the Cfg<F> feature bits (no
// output pointers, no scheduling). Read from the packed scene alone, so the answer needs no device.
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

// The RGB8 of a width x height buffer of subpixel means: rt_render's own (k_finalize_f64), byte for byte.
hipError_t finalize_rgb(int32_t width, int32_t height, const double* d_sub, uint8_t* d_rgb, hipStream_t st) {
    rt::RenderArgs a{};
    a.tw = width;
    a.th = height;
    a.rgb_out = d_rgb;
    return rt::launch_finalize_f64(a, d_sub, st);
}

// Split-tail scratch for an f64 megakernel launch over npix pixels (a frame's tile, or a pixel list through a pool
// kernel) on the current device (megakernel_common.h plan_tail): the samples after chunk 0 of the subpixels a
// launch splits — kernels.h tail_split_x2 / 2 per resident lane in the analytic and flat-mesh kernels
// (no more than 1024 lanes per CU: 4 waves/SIMD, the 1024-thread query pool), so 1536 per CU (393,216 on
// 256 CUs: 2.1 GB at 1024 spp), 2048 for frames of <= 4 subpixels per lane; six per path slot in the
// mesh walk kernels (<= 1024 slots per CU) — at most 3 GB. A smaller buffer only splits fewer
// subpixels (plan_tail; rt_debug_last_split reports the split wanted and made), with the same frame bits.
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

// Enqueue one render on `st` (device buffers); returns without waiting for the device (except in
// wavefront mode, whose host loop drives the bounces and polls host_cancel). dcancel: device view of
// a cancel word the megakernels poll (CancelMirror::dev) or null; ps: stats to complete after the
// stream drains (PendingStats::finish) or null.
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

}  // namespace

extern "C" {

const char* rt_last_error(void) { return g_err.c_str(); }
int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int finish_scene(rt::host::Scene&& sc, rt_scene** out) {
    auto s = std::make_unique<rt_scene>();
    s->host = std::move(sc);
    rt::host::cp3(s->cam_pos, s->host.cam_pos);
    rt::host::cp3(s->cam_dir, s->host.cam_dir);
    std::string err;
    const int rc = rt::host::pack_scene(s->host, &s->packed, &err);
    if (rc != RT_OK) return fail(rc, err);
    *out = s.release();
    return RT_OK;
}

int rt_scene_view(const rt_scene* base, const double view[10], rt_scene** out) {
    if (out) *out = nullptr;
    if (!base || !view || !out) return fail(RT_E_INVAL, "rt_scene_view: null argument");
    for (int k = 0; k < 10; ++k)
        if (!std::isfinite(view[k])) return fail(RT_E_INVAL, "rt_scene_view: every component must be finite");
    const double *dir = view + 3, *right = view + 6, fov = view[9];
    if (!(fov > 0.0)) return fail(RT_E_INVAL, "rt_scene_view: fov must be > 0");
    const double c[3] = {right[1] * dir[2] - right[2] * dir[1], right[2] * dir[0] - right[0] * dir[2],
                         right[0] * dir[1] - right[1] * dir[0]};
    if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]) || (c[0] == 0.0 && c[1] == 0.0 && c[2] == 0.0))
        return fail(RT_E_INVAL, "rt_scene_view: cross(right, dir) must be finite and not zero");
    rt_scene* v = new rt_scene(base);
    std::memcpy(v->cam_pos, view, 3 * sizeof(double));
    std::memcpy(v->cam_dir, dir, 3 * sizeof(double));
    std::memcpy(v->cam_right, right, 3 * sizeof(double));
    v->cam_fov = fov;
    *out = v;
    return RT_OK;
}

int rt_scene_get_view(const rt_scene* scene, double view_out[10]) {
    if (!scene || !view_out) return fail(RT_E_INVAL, "rt_scene_get_view: null argument");
    std::memcpy(view_out, scene->cam_pos, 3 * sizeof(double));
    std::memcpy(view_out + 3, scene->cam_dir, 3 * sizeof(double));
    std::memcpy(view_out + 6, scene->cam_right, 3 * sizeof(double));
    view_out[9] = scene->cam_fov;
    return RT_OK;
}

int rt_scene_load_toml(const char* toml_path, const char* assets_dir, rt_scene** out) {
    if (!toml_path || !out) return fail(RT_E_INVAL, "null argument");
    *out = nullptr;
    std::string path(toml_path), assets;
    if (assets_dir) assets = assets_dir;
    else {
        size_t sl = path.find_last_of('/');
        assets = (sl == std::string::npos ? std::string(".") : path.substr(0, sl)) + "/assets";
    }
    rt::host::Scene sc;
    std::string err;
    int rc = rt::host::load_scene_toml(path, assets, &sc, &err);
    if (rc != RT_OK) return fail(rc, err);
    return finish_scene(std::move(sc), out);
}

int rt_scene_create(const rt_scene_desc* desc, rt_scene** out) {
    if (!out) return fail(RT_E_INVAL, "null argument");
    *out = nullptr;
    rt::host::Scene sc;
    std::string err;
    int rc = rt::host::scene_from_desc(desc, &sc, &err);
    if (rc != RT_OK) return fail(rc, err);
    return finish_scene(std::move(sc), out);
}

void rt_scene_destroy(rt_scene* s) { delete s; }

int rt_scene_info(const rt_scene* s, int64_t info[16]) {
    if (!s || !info) return fail(RT_E_INVAL, "null argument");
    std::memset(info, 0, 16 * sizeof(int64_t));
    info[0] = (int64_t)s->host.objects.size();
    info[1] = s->host.light;
    info[2] = (int64_t)s->host.meshes.size();
    for (const auto& m : s->host.meshes) {
        info[3] += (int64_t)m.octree.size();
        info[4] += m.octree.parents;
        info[5] += m.octree.leaves;
        info[6] += (int64_t)m.octree.refs.size();
        info[7] += (int64_t)m.num_triangles();
        info[8] += (int64_t)m.vertices.size();
        if (m.octree.max_leaf > info[9]) info[9] = m.octree.max_leaf;
        if (m.octree.max_depth > info[10]) info[10] = m.octree.max_depth;
    }
    info[11] = s->packed.slots.empty() ? 0 : 1;
    return RT_OK;
}

int rt_scene_mesh(const rt_scene* s, int32_t object, int64_t counts[4], double bbox[6], double* surface_area,
                  double* vertices, uint32_t* indices, int32_t* kind, int32_t* child, int32_t* leaf_off,
                  int32_t* leaf_cnt, int32_t* refs) {
    if (!s || object < 0 || (size_t)object >= s->host.objects.size()) return fail(RT_E_INVAL, "bad object index");
    const auto& o = s->host.objects[object];
    if (o.geom != RT_GEOM_MESH) return fail(RT_E_INVAL, "object is not a mesh");
    const auto& m = s->host.meshes[o.mesh];
    const auto& oc = m.octree;
    if (counts) {
        counts[0] = (int64_t)oc.size();
        counts[1] = (int64_t)oc.refs.size();
        counts[2] = (int64_t)m.num_triangles();
        counts[3] = (int64_t)m.vertices.size();
    }
    if (bbox) {
        double b[6] = {m.bbox.min.x, m.bbox.min.y, m.bbox.min.z, m.bbox.max.x, m.bbox.max.y, m.bbox.max.z};
        std::memcpy(bbox, b, sizeof b);
    }
    if (surface_area) *surface_area = m.surface_area;
    if (vertices)
        for (size_t i = 0; i < m.vertices.size(); ++i) {
            vertices[3 * i] = m.vertices[i].x;
            vertices[3 * i + 1] = m.vertices[i].y;
            vertices[3 * i + 2] = m.vertices[i].z;
        }
    if (indices) std::memcpy(indices, m.indices.data(), m.indices.size() * sizeof(uint32_t));
    for (size_t i = 0; i < oc.size(); ++i) {
        if (kind) kind[i] = oc.kind[i];
        if (child) std::memcpy(child + 8 * i, &oc.child[8 * i], 8 * sizeof(int32_t));
        if (leaf_off) leaf_off[i] = oc.leaf_off[i];
        if (leaf_cnt) leaf_cnt[i] = oc.leaf_cnt[i];
    }
    if (refs) std::memcpy(refs, oc.refs.data(), oc.refs.size() * sizeof(int32_t));
    return RT_OK;
}

int rt_scene_object_bvh(const rt_scene* s, int64_t counts[4], double* boxes, int32_t* a, int32_t* count, int32_t* axis,
                        int32_t* refs, int32_t* rest) {
    if (!s) return fail(RT_E_INVAL, "null argument");
    const rt::host::ObjectBvh& t = s->packed.obvh;
    if (counts) {
        counts[0] = (int64_t)t.nodes.size();
        counts[1] = (int64_t)t.refs.size();
        counts[2] = t.nodes.empty() ? 0 : (int64_t)t.rest.size();
        counts[3] = t.depth;
    }
    for (size_t i = 0; i < t.nodes.size(); ++i) {
        const rt::DevBvhNode& nd = t.nodes[i];
        if (boxes) {
            std::memcpy(boxes + 6 * i, nd.bmin, 3 * sizeof(double));
            std::memcpy(boxes + 6 * i + 3, nd.bmax, 3 * sizeof(double));
        }
        if (a) a[i] = nd.a;
        if (count) count[i] = nd.count;
        if (axis) axis[i] = nd.axis;
    }
    if (refs && !t.refs.empty()) std::memcpy(refs, t.refs.data(), t.refs.size() * sizeof(int32_t));
    if (rest && !t.nodes.empty() && !t.rest.empty()) std::memcpy(rest, t.rest.data(), t.rest.size() * sizeof(int32_t));
    return RT_OK;
}

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
            if (r < 0) { record(r, g_err); break; }
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

// Denoised previews ---------------------------------------------------------------------

namespace {

// The ordinal names a visible HIP device: RT_E_NODEVICE without one (or without the runtime), as rt_render_multi.
int need_device(const char* who, int32_t device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        return fail(RT_E_NODEVICE, std::string(who) + ": no HIP device visible");
    }
    if (device < 0 || device >= n)
        return fail(RT_E_INVAL, std::string(who) + ": device ordinal " + std::to_string(device) + " out of range");
    return RT_OK;
}

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

// The filter's scratch (32 bytes per pixel): one idle buffer of at most kScratchKeep bytes is kept for the next
// call (a 1080p frame needs 66 MB; a preview server filters frame after frame), anything else is freed when the call
// returns. A call that finds the kept buffer taken, too small or on another device allocates its own.
constexpr size_t kScratchKeep = (size_t)128 << 20;
struct ScratchKeep {
    std::mutex mu;
    void* ptr = nullptr;
    size_t bytes = 0;
    int device = -1;
} g_scratch;

void* scratch_take(int device, size_t bytes, hipError_t* err) {
    {
        std::lock_guard<std::mutex> lk(g_scratch.mu);
        if (g_scratch.ptr && g_scratch.device == device && g_scratch.bytes >= bytes) {
            void* p = g_scratch.ptr;
            g_scratch.ptr = nullptr;
            return p;
        }
    }
    void* p = nullptr;
    *err = hipMalloc(&p, bytes);
    return *err == hipSuccess ? p : nullptr;
}
// (the stream that used it has been waited for)
void scratch_give(int device, void* p, size_t bytes) {
    void* drop = p;
    if (bytes <= kScratchKeep) {
        std::lock_guard<std::mutex> lk(g_scratch.mu);
        if (!g_scratch.ptr || g_scratch.bytes < bytes) {  // keep the larger one
            drop = g_scratch.ptr;
            const int drop_dev = g_scratch.device;
            g_scratch.ptr = p;
            g_scratch.bytes = bytes;
            g_scratch.device = device;
            if (drop && drop_dev != device) {
                (void)hipSetDevice(drop_dev);
                (void)hipFree(drop);
                (void)hipSetDevice(device);
                drop = nullptr;
            }
        }
    }
    if (drop) (void)hipFree(drop);
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

// Progressive accumulation ----------------------------------------------------------------

// The device memory comes lazily (rt_ffi.h): the sums with the first pass, the staging area (a pass's sub, a variance
// image, an RGB8 frame) with the first call that needs one. rt_accum_add and the host forms run on a stream of their
// own that lives for the call, as rt_render's does.
struct rt_accum {
    int32_t device = 0, width = 0, height = 0;
    int64_t K = 0, N = 0;
    double* S = nullptr;
    double* Q = nullptr;
    char* stage = nullptr;
    // rendering to an error target: the per-pixel counts cnt[pix][2] = (K_p, N_p) head a buffer made by
    // the first sparse merge or selection; they are valid (and used) once a sparse pass has been merged
    char* adapt = nullptr;
    bool sparse = false;
    // seeded by rt_accum_reproject: S, Q and the per-pixel counts hold reprojected history although
    // no full-frame pass has been merged since (K = N = 0), so the next merge adds instead of storing
    bool seeded = false;
    // covered by rt_accum_fill: a seeded accumulator whose every K_p >= 2 without two full-frame
    // passes; it passes wherever K >= 1 or K >= 2 is asked for
    bool covered = false;
    // batched passes: the plan's and the expansion's buffers, made by the first call that needs them
    char* batch = nullptr;
    uint32_t* cnt() const { return (uint32_t*)adapt; }
    size_t npix() const { return (size_t)width * height; }
    size_t sub_bytes() const { return npix() * 12 * sizeof(double); }
    double* stage_sub() const { return (double*)stage; }
    float* stage_var() const { return (float*)(stage + sub_bytes()); }
    uint8_t* stage_rgb() const { return (uint8_t*)(stage + sub_bytes() + npix() * 4 * sizeof(float)); }
};

namespace {

// The accumulator's error-target buffers: cnt | list | selection scratch | total.
// (the scratch and the total 16-byte aligned; the scratch holds 8-byte words)
size_t adapt_scratch_at(const rt_accum* a) { return align_up(a->npix() * 12, 16); }
size_t adapt_total_at(const rt_accum* a) {
    return adapt_scratch_at(a) + align_up(rt::select_scratch_bytes((long)a->npix()), 16);
}
size_t adapt_bytes(const rt_accum* a) { return adapt_total_at(a) + 16; }
uint32_t* adapt_list(const rt_accum* a) { return (uint32_t*)(a->adapt + a->npix() * 8); }
void* adapt_scratch(const rt_accum* a) { return a->adapt + adapt_scratch_at(a); }
uint32_t* adapt_total(const rt_accum* a) { return (uint32_t*)(a->adapt + adapt_total_at(a)); }

// Makes the accumulator's device state ready for the entry point `who`, after its checks that need no device: the
// ordinal names a visible device, which is selected; the sums exist, and what the call needs of the staging area
// and of the error-target buffers.
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
        e = hipMalloc((void**)&a->stage, a->sub_bytes() + a->npix() * 4 * sizeof(float) + align_up(a->npix() * 3, 16));
        if (e != hipSuccess) a->stage = nullptr;
    }
    if (e != hipSuccess) return oom_or_hip(e, "rt_accum buffers");
    if (adapt && !a->adapt) {
        e = hipMalloc((void**)&a->adapt, adapt_bytes(a));
        if (e != hipSuccess) {
            a->adapt = nullptr;
            return oom_or_hip(e, "rt_accum error-target buffers");
        }
    }
    return RT_OK;
}

// Merges the pass in d_sub on `st`, waits for it and counts it.
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

// Enqueues the resolve on `st`: sub (or, when only the RGB8 is wanted, the staging sub), var, rgb.
hipError_t accum_resolve_enqueue(rt_accum* a, double* d_sub, float* d_var, uint8_t* d_rgb, hipStream_t st) {
    hipError_t e = a->sparse ? rt::launch_accum_resolve_cnt(a->S, a->Q, a->cnt(), (long)a->npix(), d_sub, d_var, st)
                             : rt::launch_accum_resolve(a->S, a->Q, (long)a->npix(), a->N, a->K, d_sub, d_var, st);
    if (e == hipSuccess && d_rgb) e = finalize_rgb(a->width, a->height, d_sub, d_rgb, st);
    return e;
}

}  // namespace

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

// Rendering to a per-pixel error target ---------------------------------------------------

namespace {

// The arguments of a pixel-list render that need no device: the whole frame, the f64 fused path, the list's size.
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

// A host pixel list: strictly ascending (so unique) ids below npix.
int check_pixel_list(const char* who, const uint32_t* pixels, int64_t n_pixels, int64_t npix) {
    for (int64_t e = 0; e < n_pixels; ++e) {
        if ((int64_t)pixels[e] >= npix)
            return fail(RT_E_INVAL, std::string(who) + ": pixel id " + std::to_string(pixels[e]) + " outside the frame");
        if (e > 0 && pixels[e] <= pixels[e - 1])
            return fail(RT_E_INVAL, std::string(who) + ": the pixel list must be strictly ascending");
    }
    return RT_OK;
}

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
// path (a caller's choice, or RT_LIST_AUTO) -> the family that runs, or RT_E_INVAL for an unknown path or a family the
// scene has no instance of.
int list_family_of(const char* who, const rt_scene* s, const rt_render_params* p, int64_t n_pixels, int32_t path,
                   int* family) {
    if (path < RT_LIST_AUTO || path > RT_LIST_ROLES) return fail(RT_E_INVAL, std::string(who) + ": unknown kernel family");
    const int pool = list_pool_of(s, p);
    if (path == RT_LIST_AUTO) *family = list_auto_family(pool, n_pixels);
    else if (path == RT_LIST_FUSED || path == pool) *family = path;
    else return fail(RT_E_INVAL, std::string(who) + ": the scene has no pixel-list instance of this kernel family");
    return RT_OK;
}

// An empty list launches nothing: no stats to speak of.
int empty_list(rt_render_stats* stats) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    return RT_OK;
}

// render_enqueue for a device unit list (kernels.h UnitList, n > 0): a pixel list (what = "pixel-list render") or unit
// words with their 16 device seeds (what = "batched render"; the family rule is the pixel list's). The
// list or passes kernel of `path`'s family + k_finalize_f64 on the compact buffer; arguments checked by
// check_render_pixels or check_passes (and list_family_of for a path other than RT_LIST_AUTO). d_rgb and d_sub may be null.
constexpr const char* kListRender = "pixel-list render";
constexpr const char* kBatchRender = "batched render";
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

// host_list: the list is on the host and checked (strictly ascending ids below width * height).
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

// Merges the compact pass d_sub of the device list d_pixels on `st` and waits for it; the first sparse merge fills the
// per-pixel counts with the frame's (K, N). The merge launch is the varying part: one pass per pixel, or with d_counts
// and d_off (device, n_pixels entries) the run merge of a batched pass, d_counts[e] passes of pixel e from unit d_off[e] on.
int accum_merge_list(rt_accum* a, const uint32_t* d_pixels, int64_t n_pixels, const double* d_sub, int32_t n,
                     hipStream_t st, const uint8_t* d_counts = nullptr, const uint32_t* d_off = nullptr) {
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
    if (e == hipSuccess) e = hipMemcpyAsync(&total, adapt_total(a), sizeof total, hipMemcpyDeviceToHost, st);
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
    const int rc = run(adapt_list(a), dcap, cs.st);
    if (rc != RT_OK) return rc;
    const int64_t n = std::min(*n_out, dcap);
    if (n > 0) HIP_TRY(hipMemcpy(pixels_out, adapt_list(a), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

// Resolves the variance into the staging area, selects into d_out (device, cap ids) on `st`, waits, and reads the count.
int select_run(rt_accum* a, float abs_tol, float rel_tol, int32_t max_n, uint32_t* d_out, int64_t cap, int64_t* n_out,
               hipStream_t st) {
    hipError_t e = accum_resolve_enqueue(a, nullptr, a->stage_var(), nullptr, st);
    if (e == hipSuccess)
        e = rt::launch_accum_select(a->S, a->stage_var(), a->sparse ? a->cnt() : nullptr, a->N, a->width, a->height,
                                    abs_tol, rel_tol, max_n, adapt_scratch(a), d_out, (long)cap, adapt_total(a), st);
    return list_counts("rt_accum_select", a, e, st, n_out);
}

}  // namespace

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
    const hipError_t e = hipMemcpyAsync(adapt_list(a), pixels, (size_t)n_pixels * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return oom_or_hip(e, "rt_accum_add_pixels");
    rc = render_units_enqueue(const_cast<rt_scene*>(scene), p, {adapt_list(a), n_pixels, nullptr}, nullptr, a->stage_sub(),
                              st, call.mirror.dev, &call.ps, RT_LIST_AUTO, kListRender);
    rc = call.finish("rt_accum_add_pixels", rc);
    if (rc != RT_OK) return rc;  // failed, or cancelled: nothing merged
    return accum_merge_list(a, adapt_list(a), n_pixels, a->stage_sub(), p->spp / 4, st);
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
    HIP_TRY(hipMemcpyAsync(adapt_list(a), pixels, (size_t)n_pixels * sizeof(uint32_t), hipMemcpyHostToDevice, cs.st));
    HIP_TRY(hipMemcpyAsync(a->stage_sub(), sub, (size_t)n_pixels * 12 * sizeof(double), hipMemcpyHostToDevice, cs.st));
    return accum_merge_list(a, adapt_list(a), n_pixels, a->stage_sub(), n, cs.st);
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
    a.n_valid = (unsigned long long*)adapt_total(d);
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

// Filling the holes of a reprojection -------------------------------------------------------

namespace {

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
    unsigned long long* d_holes = (unsigned long long*)(adapt_total(a) + 2);
    hipError_t e = rt::launch_accum_holes(a->cnt(), a->width, a->height, period, phase, adapt_scratch(a), d_out, (long)cap,
                                          adapt_total(a), d_holes, st);
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
        rc = holes_run(a, pass == 0 ? period : 0, pass == 0 ? phase : 0, adapt_list(a), (int64_t)a->npix(), &n_list,
                       nullptr, st);
        if (rc != RT_OK) return rc;
        lens[pass] = n_list;
        if (n_list == 0) continue;  // an empty list launches nothing
        if (n_list > (int64_t)INT32_MAX / 4) return fail(RT_E_INVAL, "rt_accum_fill: the list's length * 4 must fit an int32");
        rt_render_params pp = *p;
        if (pass == 1) pp.seed = seed2;
        rc = render_units_enqueue(const_cast<rt_scene*>(scene), &pp, {adapt_list(a), n_list, nullptr}, nullptr,
                                  a->stage_sub(), st, call.mirror.dev, &call.ps, RT_LIST_AUTO, kListRender);
        rc = call.finish("rt_accum_fill", rc);
        if (rc < 0) return rc;
        if (rc != RT_OK) break;  // cancelled: this pass merges nothing and the accumulator stays uncovered
        rc = accum_merge_list(a, adapt_list(a), n_list, a->stage_sub(), p->spp / 4, st);
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

// Batched passes: several error-target passes per pixel in one launch ---------------------

namespace {

static_assert(RT_PASSES_MAX == rt::kPassesMax, "accum.h mirrors rt_ffi.h's RT_PASSES_MAX");
// a unit word holds the pixel id below the pass index (integrator_f64.h kPassShift)
constexpr int64_t kPassFramePixels = (int64_t)1 << 28;

// The accumulator's batch buffers: want | counts | off | units | expansion scratch | words | seeds.
// (words: hist[17] at 0, the expansion's unit total at 20; 16-byte aligned parts)
size_t batch_counts_at(const rt_accum* a) { return align_up(a->npix(), 16); }
size_t batch_off_at(const rt_accum* a) { return 2 * align_up(a->npix(), 16); }
size_t batch_units_at(const rt_accum* a) { return batch_off_at(a) + align_up(a->npix() * 4, 16); }
size_t batch_runs_at(const rt_accum* a) { return batch_units_at(a) + align_up(a->npix() * 4, 16); }
size_t batch_words_at(const rt_accum* a) { return batch_runs_at(a) + align_up(rt::runs_scratch_bytes((long)a->npix()), 16); }
size_t batch_seeds_at(const rt_accum* a) { return batch_words_at(a) + 128; }
size_t batch_bytes(const rt_accum* a) { return batch_seeds_at(a) + RT_PASSES_MAX * sizeof(uint64_t); }
uint8_t* batch_want(const rt_accum* a) { return (uint8_t*)a->batch; }
uint8_t* batch_counts(const rt_accum* a) { return (uint8_t*)(a->batch + batch_counts_at(a)); }
uint32_t* batch_off(const rt_accum* a) { return (uint32_t*)(a->batch + batch_off_at(a)); }
uint32_t* batch_units(const rt_accum* a) { return (uint32_t*)(a->batch + batch_units_at(a)); }
void* batch_runs(const rt_accum* a) { return a->batch + batch_runs_at(a); }
uint32_t* batch_words(const rt_accum* a) { return (uint32_t*)(a->batch + batch_words_at(a)); }
uint64_t* batch_seeds(const rt_accum* a) { return (uint64_t*)(a->batch + batch_seeds_at(a)); }

// accum_ready plus the batch buffers.
int batch_ready(const char* who, rt_accum* a) {
    const int rc = accum_ready(who, a, true, true);
    if (rc != RT_OK) return rc;
    if (!a->batch) {
        const hipError_t e = hipMalloc((void**)&a->batch, batch_bytes(a));
        if (e != hipSuccess) {
            a->batch = nullptr;
            return oom_or_hip(e, "rt_accum batch buffers");
        }
    }
    return RT_OK;
}

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

// The plan on `st`: the variance into the staging area, the wanted counts and their histogram, the frame cap on the
// host (the largest C' whose unit total fits a frame), then ids and final counts into d_pixels / d_counts (device,
// cap entries). res = list length, unit total, largest final count. Waits.
int plan_run(const char* who, rt_accum* a, float abs_tol, float rel_tol, int32_t max_n, int32_t n, float gain,
             int32_t max_passes, uint32_t* d_pixels, uint8_t* d_counts, int64_t cap, int64_t res[3], hipStream_t st) {
    uint32_t* words = batch_words(a);
    hipError_t e = accum_resolve_enqueue(a, nullptr, a->stage_var(), nullptr, st);
    if (e == hipSuccess)
        e = rt::launch_accum_plan_count(a->S, a->stage_var(), a->sparse ? a->cnt() : nullptr, a->N, a->width, a->height,
                                        abs_tol, rel_tol, max_n, n, gain, max_passes, adapt_scratch(a), batch_want(a), words,
                                        adapt_total(a), st);
    uint32_t hist[RT_PASSES_MAX + 1] = {0}, total = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(hist, words, sizeof hist, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, adapt_total(a), sizeof total, hipMemcpyDeviceToHost, st);
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
    e = rt::launch_accum_plan_write(adapt_scratch(a), batch_want(a), (long)npix, cmax, d_pixels, d_counts, (long)cap, st);
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
    const hipError_t e = rt::launch_accum_expand(adapt_list(a), batch_counts(a), (long)n_pixels, batch_runs(a), batch_off(a),
                                                 batch_units(a), (long)units, batch_words(a) + 20, st);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    // RT_LIST_AUTO: the scene's pool wherever it has one
    int rc = render_units_enqueue(const_cast<rt_scene*>(scene), p, {batch_units(a), units, batch_seeds(a)}, nullptr,
                                  a->stage_sub(), st, call.mirror.dev, &call.ps, RT_LIST_AUTO, kBatchRender);
    rc = call.finish(who, rc);
    if (rc != RT_OK) return rc;  // failed, or cancelled: nothing merged
    return accum_merge_list(a, adapt_list(a), n_pixels, a->stage_sub(), p->spp / 4, st, batch_counts(a), batch_off(a));
}

}  // namespace

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
    int rc = check_plan(who, a, abs_tol, rel_tol, n, gain, max_passes);
    if (rc == RT_OK && !n_out) rc = fail(RT_E_INVAL, std::string(who) + ": null argument");
    if (rc == RT_OK && (cap < 0 || (cap > 0 && (!d_pixels || !d_counts)))) rc = fail(RT_E_INVAL, std::string(who) + ": bad output buffer");
    if (rc == RT_OK) rc = check_plan_passes(who, a);
    if (rc == RT_OK) rc = batch_ready(who, a);
    if (rc != RT_OK) return rc;
    int64_t res[3];
    rc = plan_run(who, a, abs_tol, rel_tol, max_n, n, gain, max_passes, (uint32_t*)d_pixels, (uint8_t*)d_counts, cap, res,
                  (hipStream_t)stream);
    if (rc != RT_OK) return rc;
    *n_out = res[0];
    if (units_out) *units_out = res[1];
    if (passes_out) *passes_out = res[2];
    return RT_OK;
}

int rt_accum_plan(void* accum, float abs_tol, float rel_tol, int32_t max_n, int32_t n, float gain, int32_t max_passes,
                  uint32_t* pixels_out, uint8_t* counts_out, int64_t cap, int64_t* n_out, int64_t* units_out,
                  int64_t* passes_out) {
    const char* who = "rt_accum_plan";
    rt_accum* a = (rt_accum*)accum;
    int rc = check_plan(who, a, abs_tol, rel_tol, n, gain, max_passes);
    if (rc == RT_OK && !n_out) rc = fail(RT_E_INVAL, std::string(who) + ": null argument");
    if (rc == RT_OK && (cap < 0 || (cap > 0 && (!pixels_out || !counts_out)))) rc = fail(RT_E_INVAL, std::string(who) + ": bad output buffer");
    if (rc == RT_OK) rc = check_plan_passes(who, a);
    if (rc == RT_OK) rc = batch_ready(who, a);
    if (rc != RT_OK) return rc;
    CallStream cs;
    HIP_TRY(cs.init());
    const int64_t dcap = std::min<int64_t>(cap, (int64_t)a->npix());
    int64_t res[3];
    rc = plan_run(who, a, abs_tol, rel_tol, max_n, n, gain, max_passes, adapt_list(a), batch_counts(a), dcap, res, cs.st);
    if (rc != RT_OK) return rc;
    *n_out = res[0];
    if (units_out) *units_out = res[1];
    if (passes_out) *passes_out = res[2];
    const int64_t m = std::min(res[0], dcap);
    if (m > 0) {
        HIP_TRY(hipMemcpy(pixels_out, adapt_list(a), (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(counts_out, batch_counts(a), (size_t)m, hipMemcpyDeviceToHost));
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
    hipError_t e = hipMemcpyAsync(adapt_list(a), pixels, (size_t)n_pixels * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(batch_counts(a), counts, (size_t)n_pixels, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = seeds_upload(batch_seeds(a), seeds, n_seeds, h_seeds, st);
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
    rc = plan_run(who, a, abs_tol, rel_tol, max_n, p->spp / 4, gain, n_seeds, adapt_list(a), batch_counts(a),
                  (int64_t)a->npix(), res, st);
    if (rc != RT_OK) return rc;
    if (out) {
        out[0] = res[0];
        out[1] = res[1];
        out[2] = res[2];
    }
    if (res[0] == 0) return empty_list(stats);  // an empty plan launches nothing
    const hipError_t e = seeds_upload(batch_seeds(a), seeds, n_seeds, h_seeds, st);
    if (e != hipSuccess) return oom_or_hip(e, who);
    return batch_render_merge(who, a, scene, p, res[0], res[1], call);
}

// Batch query diagnostics (include/rt_diag.h, kernels/diag_queries.h) -------------------------------------

namespace {

// The arguments of rt_diag_trace / rt_diag_visible that need no device: form, flags and what the form asks of
// the scene.
int check_diag(const char* who, const rt_scene* s, int32_t form, uint32_t flags, int64_t n, bool ptrs) {
    if (!s || !ptrs) return fail(RT_E_INVAL, std::string(who) + ": null argument");
    if (n < 0) return fail(RT_E_INVAL, std::string(who) + ": n must be >= 0");
    if (form < RT_DIAG_FUSED || form > RT_DIAG_FUSED_G1) return fail(RT_E_INVAL, std::string(who) + ": unknown form");
    if (flags & ~RT_FLAG_MESH_NEAREST) return fail(RT_E_INVAL, std::string(who) + ": unknown flag");
    if (flags && form != RT_DIAG_FUSED && form != RT_DIAG_FUSED_G1)
        return fail(RT_E_INVAL, std::string(who) + ": RT_FLAG_MESH_NEAREST needs a fused form");
    const int32_t compact = s->packed.compact;
    const bool meshes = !s->host.meshes.empty();
    if (form == RT_DIAG_FUSED_G0 && (meshes || !compact))
        return fail(RT_E_INVAL, std::string(who) + ": the mesh-free fused form needs a compact scene without meshes");
    if (form >= RT_DIAG_SPLIT_SLOTS && (!meshes || !compact))
        return fail(RT_E_INVAL, std::string(who) + ": this form needs a compact scene with meshes");
    if (form == RT_DIAG_SPLIT_SLOTS && s->packed.slots.empty())
        return fail(RT_E_INVAL, std::string(who) + ": the slot-walk form needs the scene's slot tables");
    if (form == RT_DIAG_SPLIT_FLAT && !s->packed.all_flat)  // meshes: checked above (Packed::all_flat)
        return fail(RT_E_INVAL, std::string(who) + ": the flat-query form needs flat octrees only");
    return RT_OK;
}

// Uploads the inputs, runs the form's kernel, reads back: in[2] are [n][3] doubles; outs: (host, bytes per query).
struct DiagOut {
    void* host;
    size_t per;
    void** dev;
};
int diag_run(const char* who, const rt_scene* scene, int32_t device, int32_t form, uint32_t flags, bool visible,
             rt::DiagArgs& a, const double* in0, const double* in1, const double** d_in0, const double** d_in1,
             DiagOut* outs, int n_outs) {
    HIP_TRY(hipSetDevice(device));
    rt::DevScene ds;
    int rc = upload(const_cast<rt_scene*>(scene), device, &ds);
    if (rc != RT_OK) return rc;
    const size_t n = (size_t)a.n, v3 = n * 3 * sizeof(double);
    DeviceBlock buf;
    const size_t at_in0 = buf.part(v3), at_in1 = buf.part(v3), at_outs = buf.bytes;
    size_t at[8];  // n_outs <= 5
    for (int k = 0; k < n_outs; ++k) at[k] = buf.part(outs[k].host ? n * outs[k].per : 0);
    hipError_t e = buf.alloc();
    if (e != hipSuccess) return oom_or_hip(e, std::string(who) + " buffers");
    *d_in0 = buf.at<const double>(at_in0);
    *d_in1 = buf.at<const double>(at_in1);
    for (int k = 0; k < n_outs; ++k) *outs[k].dev = outs[k].host ? buf.at<void>(at[k]) : nullptr;
    e = hipMemcpy(buf.at<void>(at_in0), in0, v3, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf.at<void>(at_in1), in1, v3, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(buf.at<void>(at_outs), 0, buf.bytes - at_outs);
    if (e == hipSuccess) {
        if (form == RT_DIAG_FUSED || form == RT_DIAG_FUSED_G0 || form == RT_DIAG_FUSED_G1)
            e = rt::launch_diag_fused(ds, a, visible, form == RT_DIAG_FUSED_G0 ? 1 : form == RT_DIAG_FUSED_G1 ? 2 : 0,
                                      (flags & RT_FLAG_MESH_NEAREST) != 0, nullptr);
        else if (form == RT_DIAG_SPLIT_SLOTS) e = rt::launch_diag_slots(ds, a, visible, nullptr);
        else if (form == RT_DIAG_SPLIT_KIDS) e = rt::launch_diag_kids(ds, a, visible, nullptr);
        else e = rt::launch_diag_flat(ds, a, visible, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int k = 0; k < n_outs && e == hipSuccess; ++k)
        if (outs[k].host) e = hipMemcpy(outs[k].host, *outs[k].dev, n * outs[k].per, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return RT_OK;
}

}  // namespace

int rt_diag_trace(const rt_scene* scene, int32_t device, int32_t form, uint32_t flags, int64_t n, const double* o,
                  const double* d, double* t, int32_t* obj, int32_t* prim, double* pos, double* nrm) {
    int rc = check_diag("rt_diag_trace", scene, form, flags, n, o && d && t && obj && prim && pos && nrm);
    if (rc != RT_OK || n == 0) return rc;
    if ((rc = need_device("rt_diag_trace", device)) != RT_OK) return rc;
    rt::DiagArgs a{};
    a.n = (long)n;
    DiagOut outs[5] = {{t, sizeof(double), (void**)&a.t},
                       {obj, sizeof(int32_t), (void**)&a.obj},
                       {prim, sizeof(int32_t), (void**)&a.prim},
                       {pos, 3 * sizeof(double), (void**)&a.pos},
                       {nrm, 3 * sizeof(double), (void**)&a.nrm}};
    return diag_run("rt_diag_trace", scene, device, form, flags, false, a, o, d, &a.a, &a.b, outs, 5);
}

int rt_diag_visible(const rt_scene* scene, int32_t device, int32_t form, uint32_t flags, int64_t n, const double* x,
                    const double* y, uint8_t* vis, uint32_t* near_mask) {
    int rc = check_diag("rt_diag_visible", scene, form, flags, n, x && y && vis);
    if (rc != RT_OK || n == 0) return rc;
    if ((rc = need_device("rt_diag_visible", device)) != RT_OK) return rc;
    rt::DiagArgs a{};
    a.n = (long)n;
    DiagOut outs[2] = {{vis, sizeof(uint8_t), (void**)&a.vis}, {near_mask, sizeof(uint32_t), (void**)&a.near_mask}};
    return diag_run("rt_diag_visible", scene, device, form, flags, true, a, x, y, &a.a, &a.b, outs, 2);
}

int rt_diag_vertex(const rt_scene* scene, int32_t device, int32_t form, uint32_t flags, int64_t n, const double* st,
                   const uint64_t* rng, const int32_t* dk, double* st_out, uint64_t* rng_out, int32_t* dk_out,
                   int32_t* info) {
    const char* who = "rt_diag_vertex";
    if (!scene || !st || !rng || !dk || !st_out || !rng_out || !dk_out || !info)
        return fail(RT_E_INVAL, std::string(who) + ": null argument");
    if (n < 0) return fail(RT_E_INVAL, std::string(who) + ": n must be >= 0");
    if (form < RT_DIAG_FUSED || form > RT_DIAG_SPLIT_ROLES) return fail(RT_E_INVAL, std::string(who) + ": unknown form");
    if (flags & ~(uint32_t)(RT_FLAG_MIS | RT_FLAG_MESH_NEAREST)) return fail(RT_E_INVAL, std::string(who) + ": unknown flag");
    const bool split = (form >= RT_DIAG_SPLIT_SLOTS && form <= RT_DIAG_SPLIT_FLAT) || form == RT_DIAG_SPLIT_ROLES;
    if (split) {  // what rt_diag_trace asks of the scene for these forms (the roles form: what the slot form asks);
                  // their kernels walk octrees only
        const int rc = check_diag(who, scene, form == RT_DIAG_SPLIT_ROLES ? RT_DIAG_SPLIT_SLOTS : form,
                                  flags & RT_FLAG_MESH_NEAREST, n, true);
        if (rc != RT_OK) return rc;
    }
    const int32_t compact = scene->packed.compact;
    const bool meshes = !scene->host.meshes.empty();
    if (!compact) return fail(RT_E_INVAL, std::string(who) + ": needs a compact scene");
    if (form == RT_DIAG_FUSED_G0 && (meshes || (flags & RT_FLAG_MESH_NEAREST)))
        return fail(RT_E_INVAL, std::string(who) + ": the mesh-free fused form needs a scene without meshes and no mesh flag");
    if (form == RT_DIAG_FUSED_G1 && !meshes)
        return fail(RT_E_INVAL, std::string(who) + ": this form needs a scene with meshes");
    if (n == 0) return RT_OK;
    int rc = need_device(who, device);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    rt::DevScene ds;
    if ((rc = upload(const_cast<rt_scene*>(scene), device, &ds)) != RT_OK) return rc;
    rt_render_params p{};
    p.width = p.height = p.tile_w = p.tile_h = 4;
    p.spp = 4;
    p.flags = flags;
    const rt::RenderArgs a = make_render_args(scene, &p);  // the Cfg bits of a render with these flags
    const size_t rows = (size_t)n;
    const size_t b_st = rows * 19 * sizeof(double), b_rng = rows * 2 * sizeof(uint64_t), b_dk = rows * 2 * sizeof(int32_t),
                 b_info = rows * 4 * sizeof(int32_t);
    DeviceBlock buf;
    const size_t at_st = buf.part(b_st), at_rng = buf.part(b_rng), at_dk = buf.part(b_dk), at_sto = buf.part(b_st),
                 at_rngo = buf.part(b_rng), at_dko = buf.part(b_dk), at_info = buf.part(b_info);
    hipError_t e = buf.alloc();
    if (e != hipSuccess) return oom_or_hip(e, std::string(who) + " buffers");
    rt::DiagVertexArgs v{};
    v.n = (long)n;
    v.st = buf.at<const double>(at_st);
    v.rng = buf.at<const uint64_t>(at_rng);
    v.dk = buf.at<const int32_t>(at_dk);
    v.st_out = buf.at<double>(at_sto);
    v.rng_out = buf.at<uint64_t>(at_rngo);
    v.dk_out = buf.at<int32_t>(at_dko);
    v.info = buf.at<int32_t>(at_info);
    e = hipMemcpy(buf.at<void>(at_st), st, b_st, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf.at<void>(at_rng), rng, b_rng, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf.at<void>(at_dk), dk, b_dk, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(buf.at<void>(at_sto), 0, buf.bytes - at_sto);
    if (e == hipSuccess) {
        if (form == RT_DIAG_SPLIT_SLOTS) e = rt::launch_diag_vertex_slots(ds, a, v, false, nullptr);
        else if (form == RT_DIAG_SPLIT_ROLES) e = rt::launch_diag_vertex_slots(ds, a, v, true, nullptr);
        else if (form == RT_DIAG_SPLIT_KIDS) e = rt::launch_diag_vertex_kids(ds, a, v, nullptr);
        else if (form == RT_DIAG_SPLIT_FLAT) e = rt::launch_diag_vertex_flat(ds, a, v, nullptr);
        else
            e = rt::launch_diag_vertex_fused(ds, a, v, form == RT_DIAG_FUSED_G0 ? 1 : form == RT_DIAG_FUSED_G1 ? 2
                                                       : form == RT_DIAG_FUSED_LDS ? 3 : 0,
                                             (flags & RT_FLAG_MESH_NEAREST) != 0 && meshes, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(st_out, v.st_out, b_st, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rng_out, v.rng_out, b_rng, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(dk_out, v.dk_out, b_dk, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(info, v.info, b_info, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return RT_OK;
}

int rt_diag_sincos(int32_t device, int64_t n, const double* x, double* s, double* c) {
    const char* who = "rt_diag_sincos";
    if (!x || !s || !c) return fail(RT_E_INVAL, std::string(who) + ": null argument");
    if (n < 0) return fail(RT_E_INVAL, std::string(who) + ": n must be >= 0");
    if (n == 0) return RT_OK;
    int rc = need_device(who, device);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n * sizeof(double);
    DeviceBlock buf;
    const size_t at_x = buf.part(bytes), at_s = buf.part(bytes), at_c = buf.part(bytes);
    hipError_t e = buf.alloc();
    if (e != hipSuccess) return oom_or_hip(e, std::string(who) + " buffers");
    e = hipMemcpy(buf.at<void>(at_x), x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = rt::launch_diag_sincos((long)n, buf.at<const double>(at_x), buf.at<double>(at_s), buf.at<double>(at_c), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(s, buf.at<void>(at_s), bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(c, buf.at<void>(at_c), bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return RT_OK;
}

}  // extern "C"
