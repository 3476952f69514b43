// Pixel-list render for gfx950: k_render_list_f64 traces only the listed frame pixels.
// launch_render_list_f64 runs it for analytic scenes, and for mesh scenes whose frame kernel has no list instance
// (Phong mesh scenes, octrees without slot tables) or whose list is short; the other mesh scenes' lists go through
// the list instances of the frame's own pool kernels (k_megakernel_fpool_list_f64, k_megakernel_roles_list_f64:
// DESIGN.md §16), which give the same bits.
//
// The sparse passes of a render to a per-pixel error target (rt_accum_select's active pixels) have no rectangular
// tile for the megakernels' ticket -> tile-local subpixel map (integrator_f64.h subpixel_of), so this kernel builds
// the SubPixel straight from the list: entry e, subpixel j is unit 4 e + j, pixel p = pixels[e] = row * width + col
// gives pid = p and yref = height - row - 1. Everything per vertex is the fused megakernel's (render_f64.hip
// k_megakernel_f64): camera_sample, begin_path, trace_closest<C>, shade_vertex<C> with the same Cfg<F> choice, the
// camera-sample ring and the cold state in LDS columns, acc = acc + L * inv_n in sample order. So sub[e] is
// rt_render's sub_out of pixel p bit for bit (the RNG is keyed by the global pixel id).
// Scheduling: tickets of runs of consecutive units (plan_units with the analytic kernel's min_run: at least 32
// samples per ticket), no split tail, no wait between blocks; every loop is bounded by the unit count.
// RT_FLAG_FP32 and RT_FLAG_MESH_NEAREST are out of scope (rt_api.cpp returns RT_E_INVAL).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../device/integrator_f64.h"
#include "kernels.h"
#include "megakernel_common.h"

namespace rt {
using namespace f64;

typedef __attribute__((address_space(3))) double LdsDouble;
typedef __attribute__((address_space(3))) uint64_t LdsU64;

#ifndef RT_OPT_LDSOBJ
#define RT_OPT_LDSOBJ 1  // as render_f64.hip
#endif
#ifndef RT_MK_MIN_RUN
#define RT_MK_MIN_RUN 32  // as render_f64.hip
#endif

// a.n_whole = 4 n_pixels units in runs of a.unit_subs per ticket (a.n_wunits tickets); a.chunk_lg = 0, a.tail_cps = 1.
template <int F, int W>
__global__ __launch_bounds__(256, W) void k_render_list_f64(DevScene sc_g, RenderArgs a_g,
                                                           const uint32_t* __restrict__ pixels,
                                                           double* __restrict__ sub_buf, uint32_t* next_unit, int refill) {
    using C = Cfg<F | ((RT_OPT_LDSOBJ && (F & 8)) ? kCfgLdsObj : 0) | ((F & 1) ? kCfgGuards1 : 0)>;
#if RT_KARG_VIEW
    const DevScene& sc = karg_scene();  // the arguments read in place (megakernel_common.h)
    const RenderArgs& a = karg_render_args();
#else
    const DevScene& sc = sc_g;
    const RenderArgs& a = a_g;
#endif
    if constexpr (C::ldsobj) lds_objects_fill(sc);
    // per-lane LDS columns as k_megakernel_f64: the accumulator, a one-slot camera-sample ring, the cold state
    __shared__ double s_acc[3 * 256], s_nbd[3 * 256];
    __shared__ uint64_t s_nbr[2 * 256];
    __shared__ double s_cold[6 * 256];
    const LdsCold cold{(LdsDouble*)s_cold + threadIdx.x};
    LdsDouble* acc_l = (LdsDouble*)s_acc + threadIdx.x;  // component k at [k * 256]
    LdsDouble* nbd = (LdsDouble*)s_nbd + threadIdx.x;
    LdsU64* nbr = (LdsU64*)s_nbr + threadIdx.x;
    uint32_t nverts = 0;
    const long nunits = a.n_wunits;  // tickets
    int id, s;                        // the unit in hand (< n_whole) and its sample
    const long t0 = wave_ticket(next_unit, true);
    {
        int end_unused;
        unit_of(a, t0 < nunits ? t0 : 0, id, end_unused, s);
    }
    bool active = t0 < nunits;
    uint32_t pix = active ? pixels[id >> 2] : 0u;  // (id >> 2 < n_pixels: id < n_whole)
    acc_l[0] = 0.0; acc_l[256] = 0.0; acc_l[512] = 0.0;
    PathState ps;
    bool fresh = true;
    bool buffered = false;  // the ring holds sample s + 1
    while (__any(active)) {
        bool done = false;
        // camera pass: lanes that start a path now without a buffered sample (sample s), plus lanes with a free
        // ring slot whose next sample is in the same unit; run when any lane needs a sample now or >= refill lanes
        // have a free slot
        {
            const bool now = active && fresh;
            const bool need = active && !fresh && !buffered && s + 1 < a.n_samples;
            if (__any(now) || (refill > 0 && __popcll(__ballot(need)) >= refill)) {
                if (now || (refill > 0 && need)) {
                    const CameraSample nb = camera_sample<C::g1>(sc, a, subpixel_of_pixel(a, pix, id), now ? s : s + 1);
                    if (now) {
                        begin_path(sc, nb, ps);
                        fresh = false;
                    } else {
                        nbd[0] = nb.d.x; nbd[256] = nb.d.y; nbd[512] = nb.d.z;
                        nbr[0] = nb.r0; nbr[256] = nb.r1;
                        buffered = true;
                    }
                }
            }
        }
        if (active) {
            HitRec hr = trace_closest<C>(sc, ps.ray);
            nverts += hr.obj >= 0;
            fresh = !shade_vertex<C>(sc, a, ps, hr, nullptr, cold);
            if (fresh) {
                V3 acc = v3(acc_l[0], acc_l[256], acc_l[512]);
                acc = acc + ps.L * a.inv_n;  // server.rs:357-358
                acc_l[0] = acc.x; acc_l[256] = acc.y; acc_l[512] = acc.z;
                if (++s == a.n_samples) {
                    double* o = sub_buf + (size_t)id * 3;  // sub[e][j][3], id = 4 e + j
                    o[0] = acc.x;
                    o[1] = acc.y;
                    o[2] = acc.z;
                    if (id + 1 < run_end(a, id)) {  // the next unit of the run, no ticket
                        ++id;
                        if ((id & 3) == 0) pix = pixels[id >> 2];
                        s = 0;
                        acc_l[0] = 0.0; acc_l[256] = 0.0; acc_l[512] = 0.0;
                        buffered = false;
                    } else {
                        done = true;
                    }
                }
                // the next sample of the same unit from the camera buffer, in this divergent block
                if (!done && buffered) {
                    begin_path(sc, CameraSample{v3(nbd[0], nbd[256], nbd[512]), nbr[0], nbr[256]}, ps);
                    fresh = false;
                    buffered = false;
                }
            }
        }
        // cancellation: checked where the megakernel checks it, when a lane would take a new ticket
        bool stop = false;
        if (a.cancel && __any(done)) stop = __hip_atomic_load(a.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
        const long nt = wave_ticket(next_unit, done && !stop);
        flush_count_if_full(a.counters, nverts, done);
        if (done) {
            active = !stop && nt < nunits;
            int end_unused;
            unit_of(a, active ? nt : 0, id, end_unused, s);
            if (active) pix = pixels[id >> 2];
            acc_l[0] = 0.0; acc_l[256] = 0.0; acc_l[512] = 0.0;
            fresh = true;
            buffered = false;
        }
    }
    flush_count(a.counters, nverts);
}

template <int F, int W>
static void launch_list(const DevScene& sc, const RenderArgs& a_in, const uint32_t* pixels, double* sub_buf,
                        uint32_t* next_unit, int refill, hipStream_t st) {
    const long nsub = a_in.n_whole;
    const long blocks = resident_blocks(k_render_list_f64<F, W>, (nsub + 255) / 256);
    RenderArgs a = a_in;
    plan_units(a, blocks * 256, 256, RT_MK_MIN_RUN);
    hipLaunchKernelGGL((k_render_list_f64<F, W>), dim3((unsigned)blocks), dim3(256), 0, st, sc, a, pixels, sub_buf,
                       next_unit, refill);
}

// mesh instances at 3 waves/SIMD, analytic at 4 (launch_megakernel_f64's shapes)
template <int F>
static void launch_list_shape(const DevScene& sc, const RenderArgs& a, const uint32_t* pixels, double* sub_buf,
                              uint32_t* next_unit, int refill, hipStream_t st) {
    if constexpr ((F & 1) != 0) launch_list<F, 3>(sc, a, pixels, sub_buf, next_unit, refill, st);
    else launch_list<F, RT_MK_W4>(sc, a, pixels, sub_buf, next_unit, refill, st);
}

hipError_t launch_render_list_f64(const DevScene& sc, const RenderArgs& a_in, const uint32_t* pixels, long n_pixels,
                                  double* sub_buf, uint32_t* next_unit, int family, double* tail_buf, size_t tail_cap,
                                  hipStream_t st) {
    if (n_pixels <= 0 || a_in.n_samples <= 0) return hipSuccess;
    if (n_pixels > 0x7fffffffL / 4) return hipErrorInvalidValue;
    RenderArgs a = a_in;
    a.n_whole = (int32_t)(n_pixels * 4);  // every unit is a whole subpixel unless a pool launcher plans a split tail
    a.chunk_lg = 0;
    a.tail_cps = 1;
    a.tail_buf = nullptr;
    t_tail_plan = TailPlan{};
    hipError_t e = hipMemsetAsync(next_unit, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    // a mesh scene's pool family (the kernel its full frame runs); a family the scene has no
    // instance of is an error, never a quiet change of kernel
    if (family != kListFused) {
        if (family != list_pool_family(a, sc.node_slot != nullptr)) return hipErrorInvalidValue;
        if (family == kListFpool)
            return launch_render_list_flat_f64(sc, a, pixels, n_pixels, sub_buf, next_unit, tail_buf, tail_cap, st);
        return launch_render_list_roles_f64(sc, a, pixels, n_pixels, sub_buf, next_unit, tail_buf, tail_cap, st);
    }
    static const int refill = env_int("RT_MK_CAM_REFILL", 40);  // the megakernel's camera-ring refill threshold
#define RT_LIST_CASE(F)                                                       \
    case F:                                                                   \
        launch_list_shape<F>(sc, a, pixels, sub_buf, next_unit, refill, st);  \
        break;
    switch (a.features & 15) {
        RT_LIST_CASE(0) RT_LIST_CASE(1) RT_LIST_CASE(2) RT_LIST_CASE(3) RT_LIST_CASE(4) RT_LIST_CASE(5) RT_LIST_CASE(6)
        RT_LIST_CASE(7) RT_LIST_CASE(8) RT_LIST_CASE(9) RT_LIST_CASE(10) RT_LIST_CASE(11) RT_LIST_CASE(12)
        RT_LIST_CASE(13) RT_LIST_CASE(14) RT_LIST_CASE(15)
    }
#undef RT_LIST_CASE
    return hipGetLastError();
}

}  // namespace rt
