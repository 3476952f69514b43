// Batch query diagnostics (include/rt_diag.h rt_diag_trace / rt_diag_visible): one lane per query through the
// query code of one kernel family. Each form's kernel lives in the translation unit that owns the code it calls
// (kernels.h launch_diag_*); this header holds what they share: the argument block, the loads and the stores.
// Included by the kernel TUs after path_f64.h.
#pragma once

#include "../device/integrator_f64.h"
#include "../device/path_f64.h"
#include "kernels.h"

namespace rt {
namespace f64 {

RT_DEV Ray diag_ray(const DiagArgs& a, long i) {
    return Ray{v3(a.a[3 * i], a.a[3 * i + 1], a.a[3 * i + 2]), v3(a.b[3 * i], a.b[3 * i + 1], a.b[3 * i + 2])};
}
// The shadow ray of segment i as mutually_visible builds it (scene.rs:258-262) and shade_vertex reuses it:
// direction and length from one div_sqrt.
template <bool G1 = false>
RT_DEV Ray diag_segment(const DiagArgs& a, long i, V3* y, double* dist) {
    const V3 x = v3(a.a[3 * i], a.a[3 * i + 1], a.a[3 * i + 2]);
    *y = v3(a.b[3 * i], a.b[3 * i + 1], a.b[3 * i + 2]);
    const V3 diff = *y - x;
    const V3 dir = div_sqrt<G1>(diff, dot(diff, diff), dist);
    return Ray{x, dir};
}
// A trace result as k_trace_f64 stores it: t = 0 and no position for a miss; pos / nrm through surface<>.
RT_DEV void diag_store_hit(const DevScene& sc, const DiagArgs& a, long i, const Ray& r, const HitRec& h, uint32_t near) {
    a.obj[i] = h.obj;
    a.prim[i] = h.obj >= 0 ? h.prim : -1;
    a.t[i] = h.obj >= 0 ? h.t : 0.0;
    if (a.near_mask) a.near_mask[i] = near;
    if (h.obj >= 0) {
        V3 p, nn;
        surface<Cfg<1>>(sc, r, h, &p, &nn);
        a.pos[3 * i] = p.x; a.pos[3 * i + 1] = p.y; a.pos[3 * i + 2] = p.z;
        a.nrm[3 * i] = nn.x; a.nrm[3 * i + 1] = nn.y; a.nrm[3 * i + 2] = nn.z;
    }
}
RT_DEV void diag_store_vis(const DiagArgs& a, long i, bool visible, uint32_t near) {
    a.vis[i] = visible ? 1 : 0;
    if (a.near_mask) a.near_mask[i] = near;
}


// Batch vertex diagnostics (rt_diag_vertex, kernels.h DiagVertexArgs): row i as the PathState a render lane would
// hold on arrival at the vertex, and the state it carries on after shade_vertex. The kernel TUs include
// integrator_f64.h (PathState) before this header.
RT_DEV PathState diag_vertex_load(const DiagVertexArgs& v, long i) {
    const double* s = v.st + 19 * i;
    PathState ps;
    ps.ray = Ray{v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5])};
    ps.beta = v3(s[6], s[7], s[8]);
    ps.L = v3(s[9], s[10], s[11]);
    ps.bemit = v3(s[12], s[13], s[14]);
    ps.o = v3(s[15], s[16], s[17]);
    ps.pdf_prev = s[18];
    ps.r0 = v.rng[2 * i];
    ps.r1 = v.rng[2 * i + 1];
    ps.depth = (uint32_t)v.dk[2 * i];
    ps.kind = v.dk[2 * i + 1];
    return ps;
}
// bemit / o: what the form's Cold holds after the vertex (RegCold: ps's own).
RT_DEV void diag_vertex_store(const DiagVertexArgs& v, long i, const PathState& ps, V3 bemit, V3 o, int obj, bool cont,
                              bool pending, uint32_t meshes) {
    double* s = v.st_out + 19 * i;
    s[0] = ps.ray.o.x; s[1] = ps.ray.o.y; s[2] = ps.ray.o.z;
    s[3] = ps.ray.d.x; s[4] = ps.ray.d.y; s[5] = ps.ray.d.z;
    s[6] = ps.beta.x; s[7] = ps.beta.y; s[8] = ps.beta.z;
    s[9] = ps.L.x; s[10] = ps.L.y; s[11] = ps.L.z;
    s[12] = bemit.x; s[13] = bemit.y; s[14] = bemit.z;
    s[15] = o.x; s[16] = o.y; s[17] = o.z;
    s[18] = ps.pdf_prev;
    v.rng_out[2 * i] = ps.r0;
    v.rng_out[2 * i + 1] = ps.r1;
    v.dk_out[2 * i] = (int32_t)ps.depth;
    v.dk_out[2 * i + 1] = ps.kind;
    v.info[4 * i] = obj;
    v.info[4 * i + 1] = cont ? 1 : 0;
    v.info[4 * i + 2] = pending ? 1 : 0;
    v.info[4 * i + 3] = (int32_t)meshes;
}

}  // namespace f64
}  // namespace rt
