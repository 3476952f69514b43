// Batch query diagnostics (include/rt_diag.h, kernels/diag_queries.h): the rt_diag_* entry points. (The rt_debug_*
// readers of the same header live beside the counters they read, in kernels/render_f64.hip.)
#include "../../../include/rt_diag.h"
#include "api_common.hpp"

using namespace rt::api;

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

extern "C" {

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
