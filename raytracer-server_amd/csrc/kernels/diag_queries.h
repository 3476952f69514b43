// Batch query diagnostics (include/rt_diag.h rt_diag_trace / rt_diag_visible): one lane per query through the
// query code of one kernel family. Each form's kernel lives in the translation unit that owns the code it calls
// (kernels.h launch_diag_*); this header holds what they share: the argument block, the loads and the stores.
// Included by the kernel TUs after path_f64.h.
#pragma once

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

}  // namespace f64
}  // namespace rt
