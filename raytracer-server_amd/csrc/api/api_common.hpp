// What more than one unit of the C ABI (include/rt_ffi.h, include/rt_diag.h) uses: error reporting, the call-lifetime
// types, the scene handle and the enqueue functions. Declarations only: each function is defined once, in the unit
// named beside it; the process-wide pools and the thread-local error string are objects of common.cpp alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/rt_ffi.h"
#include "../host/scene_pack.hpp"
#include "../kernels/kernels.h"
#include "../kernels/wavefront.h"

namespace rt::api {

using rt::host::Packed;

// Errors and argument checks (common.cpp) -----------------------------------------------------------------

// Leaves msg for rt_last_error on the calling thread and returns code.
int fail(int code, const std::string& msg);

// A failed HIP call as a return code: RT_E_OOM when the device is out of memory, RT_E_HIP otherwise.
int oom_or_hip(hipError_t e, const std::string& what);

#define HIP_TRY(expr)                                                    \
    do {                                                                 \
        hipError_t e_ = (expr);                                          \
        if (e_ != hipSuccess) return ::rt::api::oom_or_hip(e_, #expr); \
    } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The ordinal names a visible HIP device: RT_E_NODEVICE without one (or without the runtime), as rt_render_multi.
int need_device(const char* who, int32_t device);

int check_params(const rt_render_params* p);

// An empty list launches nothing: no stats to speak of.
int empty_list(rt_render_stats* stats);

// Call-lifetime types (common.cpp) ------------------------------------------------------------------------

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

// Device-visible mirror of a caller's cancel flag: a pinned, mapped word the megakernels poll
// (RenderArgs::cancel) between subpixels. The caller's flag itself is never registered with HIP (it
// may be shared by concurrent renders, or sit on memory HIP cannot pin): the host thread that waits
// for the render copies it into the mirror (wait_stream), so its lifetime stays the caller's.
// The words come from a process-wide free list and go back to it once the render has drained: a
// cancellable render (the WebSocket server renders chunk by chunk with a flag) costs no pinned
// allocation after the first. The words are never freed (one per concurrently cancellable render).
struct CancelWordPool;
CancelWordPool& cancel_words();  // the one pool of the process
struct CancelMirror {
    int32_t* host = nullptr;
    int32_t* dev = nullptr;
    CancelMirror() = default;
    CancelMirror(const CancelMirror&) = delete;
    CancelMirror& operator=(const CancelMirror&) = delete;
    ~CancelMirror();
    hipError_t init();
    void raise() {
        if (host) __atomic_store_n(host, 1, __ATOMIC_RELEASE);
    }
};

// Waits for everything enqueued on `st`, copying the caller's cancel flag into the mirror meanwhile.
// Polls with a growing pause (10 us doubling to 200 us), so a short render (one WebSocket chunk) is
// seen done within about its own duration.
hipError_t wait_stream(hipStream_t st, const volatile int32_t* cancel, CancelMirror* mirror);

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
    ~PendingStats();
    hipError_t init(rt_render_stats* o);
    // after the render's stream has completed
    int finish(std::string* err);
};

// The tail of the _device render forms: with stats, the call is synchronous with respect to the stream (rt_ffi.h).
// rc: what the enqueue returned; ps: null without stats.
int stats_sync(int rc, hipStream_t st, PendingStats* ps);

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
    int init(const char* who, const volatile int32_t* cancel_flag, rt_render_stats* stats);

    // After render_enqueue / render_units_enqueue on cs.st returned rc: waits for the render while relaying the
    // cancel flag, copies back, completes the stats; RT_CANCELLED when the flag is up by then (the caller merges
    // nothing). An enqueue that failed left its message in g_err, and the stream is drained of whatever it did
    // enqueue before anything it used is released.
    int finish(const char* who, int rc, std::initializer_list<Copy> readback = {});
};

// The filter's scratch (32 bytes per pixel): one idle buffer of at most kScratchKeep bytes is kept for the next
// call (a 1080p frame needs 66 MB; a preview server filters frame after frame), anything else is freed when the call
// returns. A call that finds the kept buffer taken, too small or on another device allocates its own.
void* scratch_take(int device, size_t bytes, hipError_t* err);
// (the stream that used it has been waited for)
void scratch_give(int device, void* p, size_t bytes);

// Scene types (scene.cpp) ---------------------------------------------------------------------------------

struct DeviceCopy {
    bool ready = false;
    void* blob = nullptr;
    rt::DevScene ds{};
};

// What a loaded or created scene owns and its views share: host data, packed tables, device uploads, workspaces.
struct SceneData {
    rt::host::Scene host;
    Packed packed;
    std::mutex mu;
    std::vector<DeviceCopy> dev;
    std::vector<std::unique_ptr<rt::Workspace>> pool;  // free wavefront workspaces, per device tagged
    ~SceneData();
};

}  // namespace rt::api

// A scene handle: the data (its own, or for a view, rt_scene_view, the root base's) and a camera. The members below
// refer to the root's data, so every entry point reads a view as it reads a scene; only the camera is the handle's.
struct rt_scene {
    std::unique_ptr<rt::api::SceneData> own;  // null in a view
    const rt_scene* root;                     // the handle that owns the data (this, unless a view)
    rt::host::Scene& host;
    rt::api::Packed& packed;
    std::mutex& mu;
    std::vector<rt::api::DeviceCopy>& dev;
    std::vector<std::unique_ptr<rt::Workspace>>& pool;
    double cam_pos[3] = {0, 0, 0}, cam_dir[3] = {0, 0, 1}, cam_right[3] = {1, 0, 0};
    double cam_fov = 0.5135;  // server.rs:330
    rt_scene()
        : own(new rt::api::SceneData), root(this), host(own->host), packed(own->packed), mu(own->mu), dev(own->dev),
          pool(own->pool) {}
    explicit rt_scene(const rt_scene* base)  // a view of base (of base's root, when base is a view itself)
        : root(base->root), host(base->host), packed(base->packed), mu(base->mu), dev(base->dev), pool(base->pool) {}
};

namespace rt::api {

// The scene's tables on `device` (uploaded by the first call that asks) and the handle's camera, as the kernels'
// DevScene.
int upload(rt_scene* s, int device, rt::DevScene* out);

// Render helpers (render.cpp) -----------------------------------------------------------------------------

// Per-render scratch (ticket counter, subpixel buffer, split-tail buffer, wavefront streams) comes
// from a per-scene pool. rt_render_device returns before its kernels finish, so a pooled workspace
// may still be in use: an idle one (its completion event has fired) is taken first; else one last
// used on the same stream, with a device-side wait on its completion event enqueued on `st` (so the
// reuse is ordered even if the caller destroyed that stream and HIP handed its handle to a new one);
// otherwise a new workspace is made (concurrent renders on one scene each get their own, rt_ffi.h).
// A reused in-flight workspace never reallocates under its previous kernels: Workspace::ensure_*
// wait for `busy` before freeing (wavefront_f64.hip).
std::unique_ptr<rt::Workspace> take_workspace(rt_scene* s, int device, hipStream_t st, hipError_t* err);
void give_workspace(rt_scene* s, std::unique_ptr<rt::Workspace> w, hipStream_t st);

// The kernels' view of `p` on the scene: frame, tile, samples, seed, camera frame and the Cfg<F> feature bits (no
// output pointers, no scheduling). Read from the packed scene alone, so the answer needs no device.
rt::RenderArgs make_render_args(const rt_scene* s, const rt_render_params* p);

// The RGB8 of a width x height buffer of subpixel means: rt_render's own (k_finalize_f64), byte for byte.
hipError_t finalize_rgb(int32_t width, int32_t height, const double* d_sub, uint8_t* d_rgb, hipStream_t st);

// Split-tail scratch for an f64 megakernel launch over npix pixels (a frame's tile, or a pixel list through a pool
// kernel) on the current device (megakernel_common.h plan_tail): the samples after chunk 0 of the subpixels a
// launch splits — kernels.h tail_split_x2 / 2 per resident lane in the analytic and flat-mesh kernels
// (no more than 1024 lanes per CU: 4 waves/SIMD, the 1024-thread query pool), so 1536 per CU (393,216 on
// 256 CUs: 2.1 GB at 1024 spp), 2048 for frames of <= 4 subpixels per lane; six per path slot in the
// mesh walk kernels (<= 1024 slots per CU) — at most 3 GB. A smaller buffer only splits fewer
// subpixels (plan_tail; rt_debug_last_split reports the split wanted and made), with the same frame bits.
void ensure_tail_scratch(rt::Workspace* ws, const rt::RenderArgs& a, size_t npix);

// Enqueue one render on `st` (device buffers); returns without waiting for the device (except in
// wavefront mode, whose host loop drives the bounces and polls host_cancel). dcancel: device view of
// a cancel word the megakernels poll (CancelMirror::dev) or null; ps: stats to complete after the
// stream drains (PendingStats::finish) or null.
int render_enqueue(rt_scene* s, const rt_render_params* p, uint8_t* d_rgb, double* d_sub, hipStream_t st,
                   const int32_t* dcancel, const volatile int32_t* host_cancel, PendingStats* ps);

// Feature buffers (denoise.cpp) ---------------------------------------------------------------------------

// Enqueues the first-hit feature pass of `p` on `st` (arguments checked by the caller).
int features_enqueue(rt_scene* s, const rt_render_params* p, float* d_feat, hipStream_t st);

// Pixel lists (pixels.cpp) --------------------------------------------------------------------------------

// The arguments of a pixel-list render that need no device: the whole frame, the f64 fused path, the list's size.
int check_render_pixels(const char* who, const rt_scene* scene, const rt_render_params* p, const void* pixels,
                        int64_t n_pixels);

// A host pixel list: strictly ascending (so unique) ids below npix.
int check_pixel_list(const char* who, const uint32_t* pixels, int64_t n_pixels, int64_t npix);

// path (a caller's choice, or RT_LIST_AUTO) -> the family that runs, or RT_E_INVAL for an unknown path or a family the
// scene has no instance of.
int list_family_of(const char* who, const rt_scene* s, const rt_render_params* p, int64_t n_pixels, int32_t path,
                   int* family);

// render_enqueue for a device unit list (kernels.h UnitList, n > 0): a pixel list (what = "pixel-list render") or unit
// words with their 16 device seeds (what = "batched render"; the family rule is the pixel list's). The
// list or passes kernel of `path`'s family + k_finalize_f64 on the compact buffer; arguments checked by
// check_render_pixels or check_passes (and list_family_of for a path other than RT_LIST_AUTO). d_rgb and d_sub may be null.
inline constexpr const char* kListRender = "pixel-list render";
inline constexpr const char* kBatchRender = "batched render";
int render_units_enqueue(rt_scene* s, const rt_render_params* p, const rt::UnitList& units, uint8_t* d_rgb, double* d_sub,
                         hipStream_t st, const int32_t* dcancel, PendingStats* ps, int32_t path, const char* what);

}  // namespace rt::api
