// C ABI (include/rt_ffi.h): error reporting, the process-wide pools and the call-lifetime types of api_common.hpp.
// The thread-local error string, the cancel-word pool and the scratch keep are this unit's objects and no other's.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

#include "api_common.hpp"

namespace {

thread_local std::string g_err;

constexpr size_t kScratchKeep = (size_t)128 << 20;
struct ScratchKeep {
    std::mutex mu;
    void* ptr = nullptr;
    size_t bytes = 0;
    int device = -1;
} g_scratch;

}  // namespace

namespace rt::api {

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int oom_or_hip(hipError_t e, const std::string& what) {
    return fail(e == hipErrorOutOfMemory ? RT_E_OOM : RT_E_HIP, what + ": " + hipGetErrorString(e));
}

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

int empty_list(rt_render_stats* stats) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    return RT_OK;
}

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

CancelMirror::~CancelMirror() {
    if (!host) return;
    CancelWordPool& p = cancel_words();
    std::lock_guard<std::mutex> lk(p.mu);
    p.free.push_back(CancelWord{host, dev});
}

hipError_t CancelMirror::init() {
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

PendingStats::~PendingStats() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (count) (void)hipHostFree(count);
}

hipError_t PendingStats::init(rt_render_stats* o) {
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

int PendingStats::finish(std::string* err) {
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

int stats_sync(int rc, hipStream_t st, PendingStats* ps) {
    if (rc < 0 || !ps) return rc;
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("stats sync: ") + hipGetErrorString(e));
    std::string err;
    const int f = ps->finish(&err);
    return f < 0 ? fail(f, err) : rc;
}

int RenderCall::init(const char* who, const volatile int32_t* cancel_flag, rt_render_stats* stats) {
    cancel = cancel_flag;
    ps.out = stats ? stats : &local;
    hipError_t e = cs.init();
    if (e == hipSuccess && mem.bytes) e = mem.alloc();
    if (e == hipSuccess && cancel) e = mirror.init();
    return e == hipSuccess ? RT_OK : oom_or_hip(e, who);
}

int RenderCall::finish(const char* who, int rc, std::initializer_list<Copy> readback) {
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

}  // namespace rt::api

extern "C" {

const char* rt_last_error(void) { return g_err.c_str(); }
int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"
