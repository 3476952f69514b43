// C ABI (include/rt_ffi.h): scene packing + per-device upload, render dispatch, error reporting.
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
#include "device/scene_layout.h"
#include "host/scene_host.hpp"
#include "kernels/accum.h"
#include "kernels/denoise.h"
#include "kernels/kernels.h"
#include "kernels/reproject.h"
#include "kernels/wavefront.h"

#ifndef RT_LTRI_INDEX
#define RT_LTRI_INDEX 0  // as path_f64.h (1: leaf triangle lists as indices, no per-leaf copies uploaded)
#endif

namespace {

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

// Host image of the device scene, packed once per scene.
struct Packed {
    std::vector<rt::DevObject> objects;
    std::vector<rt::DevMesh> meshes;
    std::vector<int32_t> kids;   // [node][8]
    std::vector<int2> up;        // [node]
    std::vector<int2> leaves;    // [leaf] {first ltri, count}
    std::vector<rt::LeafTri> ltris;
    std::vector<int32_t> ltri_id;
    std::vector<rt::DevTri> tris;
    std::vector<double> cum_area;
    std::vector<rt::DevBvhNode> bvh;  // nearest-triangle mode (RT_FLAG_MESH_NEAREST)
    std::vector<rt::DevTri> btris;
    std::vector<int32_t> btri_id;
    std::vector<rt::KidSlot> slots;      // [pid][8] child entry + subtree triangle bounds (scene_layout.h KidSlot);
                                         // empty when a node id does not fit a slot entry (the node_kids walk)
    std::vector<double> node_box;        // [pid][6] parents' octant boxes, the walk's arithmetic (DevScene::node_box)
    std::vector<int32_t> pid_up;         // [pid] the parent's parent as a pid, -1 at the root (DevScene::pid_up)
};

// A child slot (scene_layout.h KidSlot): the child entry and its subtree's triangle bounds b (lo xyz,
// hi xyz, already padded), rounded OUTWARD to 16-bit codes over the mesh's range (base + q * step), one
// extra step each way so that device-side rounding of the dequantised bounds cannot move them inward.
// The device decodes every code as base + q * step (path_f64.h kid_tight_hit), so a bound is conservative
// only if its code was not clamped to the range: for a mesh of extent E > 0 the codes of its padded
// triangle bounds lie in about [E / step, 2 E / step] = [21845, 43690], but a mesh whose cull padding
// exceeds E (a sub-1e-7 mesh far from the origin) would clamp. *exact turns false then, and the scene
// walks without slot tables (node_kids: the same result without the subtree culls).
rt::KidSlot make_slot(int32_t kid, const rt::DevMesh& dm, const double* b, bool* exact) {
    rt::KidSlot s{};
    s.kid = kid;
    for (int k = 0; k < 3; ++k) {
        s.lo[k] = 0;
        s.hi[k] = (uint16_t)rt::kTightTop;
        if (kid == rt::kKidEmpty) continue;  // never picked: its slot is not read
        if (!(dm.tight_step > 0.0) || !std::isfinite(dm.tight_step)) {
            *exact = false;
            continue;
        }
        const double ql = std::floor((b[k] - dm.tight_base[k]) / dm.tight_step) - 1.0;
        const double qh = std::ceil((b[3 + k] - dm.tight_base[k]) / dm.tight_step) + 1.0;
        if (!(ql >= 1.0 && qh <= (double)(rt::kTightTop - 1))) *exact = false;
        s.lo[k] = ql >= 1.0 ? (uint16_t)std::min(ql, (double)(rt::kTightTop - 1)) : (uint16_t)0;
        s.hi[k] = qh <= (double)(rt::kTightTop - 1) ? (uint16_t)std::max(qh, 1.0) : (uint16_t)rt::kTightTop;
    }
    return s;
}

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

void cp3(double* dst, const rt::host::D3& v) {
    dst[0] = v.x;
    dst[1] = v.y;
    dst[2] = v.z;
}

// BVH over one mesh's triangles for the nearest-triangle mode: median split of the triangle
// centroids along the longest axis, leaves of <= 4 triangles (or at depth kBvhMaxDepth - 1), nodes
// in DFS pre-order (DevBvhNode). Node boxes are the triangles' vertex bounds; the traversal's slab test pads
// them (near_box, DevMesh::cull_pad), so a triangle the ray hits is never culled.
// RT_BVH_SAH=0 selects the median-split build (A/B); default: binned SAH.
constexpr int kBins = 16;      // SAH bins per axis
constexpr int kSahDepth = 16;  // deeper BVH nodes split at the median (depth stays <= kBvhMaxDepth)
bool bvh_sah_enabled() { return rt::ab_knob("RT_BVH_SAH", 1) != 0; }

void build_bvh(Packed& p, const rt::host::Mesh& m, int32_t tri_base) {
    using rt::host::D3;
    struct Item { double lo[3], hi[3], c[3]; int32_t id; };
    const size_t n = m.num_triangles();
    std::vector<Item> it(n);
    for (size_t t = 0; t < n; ++t) {
        const D3 v[3] = {m.vertices[m.indices[3 * t]], m.vertices[m.indices[3 * t + 1]], m.vertices[m.indices[3 * t + 2]]};
        Item& x = it[t];
        x.id = (int32_t)t;
        for (int k = 0; k < 3; ++k) {
            const double a = k == 0 ? v[0].x : k == 1 ? v[0].y : v[0].z;
            const double b = k == 0 ? v[1].x : k == 1 ? v[1].y : v[1].z;
            const double c = k == 0 ? v[2].x : k == 1 ? v[2].y : v[2].z;
            x.lo[k] = std::min({a, b, c});
            x.hi[k] = std::max({a, b, c});
            x.c[k] = 0.5 * (x.lo[k] + x.hi[k]);
        }
    }
    struct Rec {
        Packed& p;
        std::vector<Item>& it;
        int32_t tri_base;
        bool sah;
        // Binned surface-area heuristic (16 bins per axis over the centroid bounds): the split
        // minimising area(L) * n(L) + area(R) * n(R); items are partitioned in place (left = lower
        // centroids along *ax). *mid = b when no split separates the items.
        static double half_area(const double* lo, const double* hi) {
            const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
            return dx * dy + dy * dz + dz * dx;
        }
        void sah_split(size_t b, size_t e, const double* clo, const double* chi, int* ax_out, size_t* mid) {
            double best = INFINITY;
            int best_ax = -1, best_bin = -1;
            for (int ax = 0; ax < 3; ++ax) {
                const double ext = chi[ax] - clo[ax];
                if (!(ext > 0.0)) continue;
                double lo[kBins][3], hi[kBins][3];
                size_t cnt[kBins] = {0};
                for (int q = 0; q < kBins; ++q)
                    for (int k = 0; k < 3; ++k) { lo[q][k] = INFINITY; hi[q][k] = -INFINITY; }
                for (size_t i = b; i < e; ++i) {
                    int q = (int)((it[i].c[ax] - clo[ax]) / ext * kBins);
                    q = std::min(kBins - 1, std::max(0, q));
                    ++cnt[q];
                    for (int k = 0; k < 3; ++k) {
                        lo[q][k] = std::min(lo[q][k], it[i].lo[k]);
                        hi[q][k] = std::max(hi[q][k], it[i].hi[k]);
                    }
                }
                double ra[kBins];
                size_t rc[kBins];
                double al[3] = {INFINITY, INFINITY, INFINITY}, ah[3] = {-INFINITY, -INFINITY, -INFINITY};
                size_t ac = 0;
                for (int q = kBins - 1; q > 0; --q) {  // suffix boxes: bins q..15
                    for (int k = 0; k < 3; ++k) { al[k] = std::min(al[k], lo[q][k]); ah[k] = std::max(ah[k], hi[q][k]); }
                    ac += cnt[q];
                    rc[q] = ac;
                    ra[q] = ac ? half_area(al, ah) : 0.0;
                }
                double pl[3] = {INFINITY, INFINITY, INFINITY}, ph[3] = {-INFINITY, -INFINITY, -INFINITY};
                size_t pc = 0;
                for (int q = 1; q < kBins; ++q) {  // split between bins q-1 and q
                    for (int k = 0; k < 3; ++k) { pl[k] = std::min(pl[k], lo[q - 1][k]); ph[k] = std::max(ph[k], hi[q - 1][k]); }
                    pc += cnt[q - 1];
                    if (pc == 0 || rc[q] == 0) continue;
                    const double cost = half_area(pl, ph) * (double)pc + ra[q] * (double)rc[q];
                    if (cost < best) { best = cost; best_ax = ax; best_bin = q; }
                }
            }
            *mid = b;
            if (best_ax < 0) return;
            const int ax = best_ax;
            const double ext = chi[ax] - clo[ax];
            auto left = [&](const Item& x) {
                int q = (int)((x.c[ax] - clo[ax]) / ext * kBins);
                return std::min(kBins - 1, std::max(0, q)) < best_bin;
            };
            *mid = (size_t)(std::stable_partition(it.begin() + b, it.begin() + e, left) - it.begin());
            *ax_out = ax;
        }
        void build(size_t b, size_t e, int depth) {
            const size_t node = p.bvh.size();
            p.bvh.push_back(rt::DevBvhNode{});
            rt::DevBvhNode nd{};
            double clo[3], chi[3];
            for (int k = 0; k < 3; ++k) {
                nd.bmin[k] = clo[k] = INFINITY;
                nd.bmax[k] = chi[k] = -INFINITY;
            }
            for (size_t i = b; i < e; ++i)
                for (int k = 0; k < 3; ++k) {
                    nd.bmin[k] = std::min(nd.bmin[k], it[i].lo[k]);
                    nd.bmax[k] = std::max(nd.bmax[k], it[i].hi[k]);
                    clo[k] = std::min(clo[k], it[i].c[k]);
                    chi[k] = std::max(chi[k], it[i].c[k]);
                }
            if (e - b <= 4 || depth + 1 >= rt::kBvhMaxDepth) {
                nd.a = (int32_t)p.btris.size();
                nd.count = (int32_t)(e - b);
                std::sort(it.begin() + b, it.begin() + e, [](const Item& x, const Item& y) { return x.id < y.id; });
                for (size_t i = b; i < e; ++i) {
                    p.btris.push_back(p.tris[tri_base + it[i].id]);
                    p.btri_id.push_back(tri_base + it[i].id);
                }
            } else {
                int ax = 0;
                size_t mid = 0;
                if (sah && depth < kSahDepth) sah_split(b, e, clo, chi, &ax, &mid);
                if (mid <= b || mid >= e) {  // median split (no SAH split found, or deep nodes)
                    ax = 0;
                    for (int k = 1; k < 3; ++k)
                        if (chi[k] - clo[k] > chi[ax] - clo[ax]) ax = k;
                    mid = (b + e) / 2;
                    std::nth_element(it.begin() + b, it.begin() + mid, it.begin() + e,
                                     [ax](const Item& x, const Item& y) { return x.c[ax] < y.c[ax] || (x.c[ax] == y.c[ax] && x.id < y.id); });
                }
                nd.axis = ax;
                build(b, mid, depth + 1);
                nd.a = (int32_t)p.bvh.size();  // global index of the right child
                build(mid, e, depth + 1);
            }
            p.bvh[node] = nd;
        }
    } rec{p, it, tri_base, bvh_sah_enabled()};
    if (n > 0) rec.build(0, n, 0);
}

// RT_OK, or RT_E_INVAL when the octree tables cannot encode the mesh (kid_leaf: leaf ids < 2^25). Parent
// ordinals beyond a KidSlot entry's range (>= kSlotMaxNode, counted over the scene's meshes) leave the scene
// without slot tables: its walks then read node_kids (walk_step<false>, the same result without the
// subtree culls).
int pack_scene(rt_scene* s) {
    using namespace rt::host;
    Packed& p = s->packed;
    const Scene& sc = s->host;
    bool slots_ok = true;
    // RT_TEST_SLOT_MAX_PID (tests only): a lower limit on the parent ordinals (pid, the slot rows a KidSlot
    // entry can name), down to 0 = no slot tables (the node_kids walk for every scene), standing in for a
    // mesh whose pids exceed the encoding (kSlotMaxNode); named as a test switch so no stray setting of a
    // production-sounding variable slows every scene down
    int32_t slot_max = rt::kSlotMaxNode;
    if (const char* v = std::getenv("RT_TEST_SLOT_MAX_PID")) slot_max = std::max(0, std::min(slot_max, std::atoi(v)));
    if (slot_max == 0) slots_ok = false;
    for (const Mesh& m : sc.meshes) {
        rt::DevMesh dm{};
        dm.node_base = (int32_t)p.up.size();
        dm.n_nodes = (int32_t)m.octree.size();
        dm.root_leaf = -1;
        dm.max_depth = (int32_t)m.octree.max_depth;
        dm.tri_base = (int32_t)p.tris.size();
        dm.n_tris = (int32_t)m.num_triangles();
        const Box& rb = m.octree.root;
        double rbox[6] = {rb.min.x, rb.min.y, rb.min.z, rb.max.x, rb.max.y, rb.max.z};
        std::memcpy(dm.root_box, rbox, sizeof rbox);
        // root octant centres, with the same arithmetic as BoundingBox::octant(i).center()
        D3 c{(rb.min.x + rb.max.x) / 2.0, (rb.min.y + rb.max.y) / 2.0, (rb.min.z + rb.max.z) / 2.0};
        for (int i = 0; i < 8; ++i) {
            D3 lo{(i & 4) ? c.x : rb.min.x, (i & 2) ? c.y : rb.min.y, (i & 1) ? c.z : rb.min.z};
            D3 hi{(i & 4) ? rb.max.x : c.x, (i & 2) ? rb.max.y : c.y, (i & 1) ? rb.max.z : c.z};
            dm.oct_center[i][0] = (lo.x + hi.x) / 2.0;
            dm.oct_center[i][1] = (lo.y + hi.y) / 2.0;
            dm.oct_center[i][2] = (lo.z + hi.z) / 2.0;
        }
        dm.surface_area = m.surface_area;
        std::memcpy(dm.cull_box, rbox, sizeof rbox);
        for (const D3& v : m.vertices) {
            const double xyz[3] = {v.x, v.y, v.z};
            for (int k = 0; k < 3; ++k) {
                dm.cull_box[k] = std::fmin(dm.cull_box[k], xyz[k]);
                dm.cull_box[3 + k] = std::fmax(dm.cull_box[3 + k], xyz[k]);
            }
        }
        {
            double mx = 1.0;
            for (double v : dm.cull_box) mx = std::fmax(mx, std::fabs(v));
            dm.cull_pad = 1e-7 * mx;
            // f32 copy rounded outward (path_f64.h near_mesh32)
            for (int k = 0; k < 3; ++k) {
                float lo = (float)dm.cull_box[k], hi = (float)dm.cull_box[3 + k];
                if ((double)lo > dm.cull_box[k]) lo = std::nextafter(lo, -INFINITY);
                if ((double)hi < dm.cull_box[3 + k]) hi = std::nextafter(hi, INFINITY);
                dm.cull32[k] = lo;
                dm.cull32[3 + k] = hi;
            }
            dm.cull32_s = (float)mx * (1.0f + 0x1p-20f);
        }
        double cum = 0.0;
        for (size_t t = 0; t < m.num_triangles(); ++t) {
            D3 a = m.vertices[m.indices[3 * t]], b = m.vertices[m.indices[3 * t + 1]], cc = m.vertices[m.indices[3 * t + 2]];
            rt::DevTri dt{};
            D3 ab{b.x - a.x, b.y - a.y, b.z - a.z}, ac{cc.x - a.x, cc.y - a.y, cc.z - a.z};
            // Triangle::normal: (c - a).cross(b - a).norm()
            D3 cr{ac.y * ab.z - ac.z * ab.y, ac.z * ab.x - ac.x * ab.z, ac.x * ab.y - ac.y * ab.x};
            double mg = std::sqrt(cr.x * cr.x + cr.y * cr.y + cr.z * cr.z);
            D3 n{cr.x / mg, cr.y / mg, cr.z / mg};
            cp3(dt.a, a);
            cp3(dt.ab, ab);
            cp3(dt.ac, ac);
            cp3(dt.n, n);
            p.tris.push_back(dt);
            cum += t < m.areas.size() ? m.areas[t] : 0.0;
            p.cum_area.push_back(cum);
        }
        dm.total_weight = cum;
        const Octree& oc = m.octree;
        // leaf ids in node order; leaf triangles copied in the leaf's own order
        std::vector<int32_t> leaf_of(oc.size(), -1);
        for (size_t i = 0; i < oc.size(); ++i) {
            if (!oc.kind[i]) continue;
            leaf_of[i] = (int32_t)p.leaves.size();
            p.leaves.push_back(int2{(int32_t)p.ltri_id.size(), oc.leaf_cnt[i]});
            for (int32_t r = 0; r < oc.leaf_cnt[i]; ++r) {
                const int32_t t = oc.refs[oc.leaf_off[i] + r];
#if !RT_LTRI_INDEX
                const rt::DevTri& lt = p.tris[dm.tri_base + t];
#if RT_LTRI72
                rt::LeafTri l72{};
                for (int k = 0; k < 3; ++k) { l72.a[k] = lt.a[k]; l72.ab[k] = lt.ab[k]; l72.ac[k] = lt.ac[k]; }
                p.ltris.push_back(l72);
#else
                p.ltris.push_back(lt);
#endif
#endif
                p.ltri_id.push_back(dm.tri_base + t);
            }
        }
        if (oc.size() > 0 && oc.kind[0]) dm.root_leaf = leaf_of[0];
        // flat octree tables (DevMesh::flat): which leaves hold each triangle, leaf lists ascending
        dm.flat = 0;
        if (oc.size() > 0 && m.num_triangles() <= (size_t)rt::kFlatMaxTris) {
            bool ok = true;
            uint8_t lm[rt::kFlatMaxTris] = {0};
            auto add_leaf = [&](int32_t node, int bit) {
                int32_t prev = -1;
                for (int32_t r = 0; r < oc.leaf_cnt[node]; ++r) {
                    const int32_t t = oc.refs[oc.leaf_off[node] + r];
                    ok &= t > prev && t < (int32_t)m.num_triangles();
                    prev = t;
                    if (ok) lm[t] |= (uint8_t)(1u << bit);
                }
            };
            if (oc.kind[0]) {
                dm.flat_root_leaf = 1;
                dm.flat_kids = 1;
                add_leaf(0, 0);
            } else {
                dm.flat_root_leaf = 0;
                dm.flat_kids = 0;
                for (int k = 0; k < 8 && ok; ++k) {
                    const int32_t c8 = oc.child[k];
                    if (c8 < 0) continue;
                    ok &= oc.kind[c8] != 0;  // every child a leaf
                    if (ok) {
                        dm.flat_kids |= 1 << k;
                        add_leaf(c8, k);
                    }
                }
            }
            if (ok) {
                dm.flat = 1;
                for (int j = 0; j < rt::kFlatMaxTris; ++j) dm.flat_leaf[j / 4] |= (uint32_t)lm[j] << (8 * (j % 4));
            }
        }
        dm.bvh_base = (int32_t)p.bvh.size();
        dm.btri_base = (int32_t)p.btris.size();
        build_bvh(p, m, dm.tri_base);
        dm.bvh_n = (int32_t)p.bvh.size() - dm.bvh_base;
        for (size_t i = 0; i < oc.size(); ++i) {
            p.up.push_back(int2{oc.parent[i] >= 0 ? oc.parent[i] + dm.node_base : -1, oc.slot[i]});
            for (int k = 0; k < 8; ++k) {
                const int32_t c8 = oc.child[8 * i + k];
                if (c8 >= 0 && oc.kind[c8] && leaf_of[c8] >= (1 << 25))  // kid_leaf's escape keeps leaf << 6 in an int32
                    return fail(RT_E_INVAL, "mesh octree too large: leaf ids must stay below 2^25 (scene_layout.h kid_leaf)");
                p.kids.push_back(c8 < 0 ? rt::kKidEmpty
                                 : oc.kind[c8] ? rt::kid_leaf(leaf_of[c8], p.leaves[leaf_of[c8]].x, p.leaves[leaf_of[c8]].y)
                                               : c8 + dm.node_base);
            }
        }
        {
            // subtree triangle bounds (nodes are in DFS pre-order: children after their parent), then each
            // parent's children quantised against the parent's box (scene_layout.h kTightTop)
            std::vector<double> sb(oc.size() * 6);
            auto tri_grow = [&](double* b, uint32_t t) {
                const D3 v[3] = {m.vertices[m.indices[3 * t]], m.vertices[m.indices[3 * t + 1]], m.vertices[m.indices[3 * t + 2]]};
                const rt::DevTri& dt = p.tris[dm.tri_base + t];
                for (int k = 0; k < 3; ++k) {
                    // the vertices, and a + ab / a + ac as tri_t's parametrisation sees them
                    const double c[5] = {k == 0 ? v[0].x : k == 1 ? v[0].y : v[0].z, k == 0 ? v[1].x : k == 1 ? v[1].y : v[1].z,
                                         k == 0 ? v[2].x : k == 1 ? v[2].y : v[2].z, dt.a[k] + dt.ab[k], dt.a[k] + dt.ac[k]};
                    for (double x : c) {
                        b[k] = std::fmin(b[k], x);
                        b[3 + k] = std::fmax(b[3 + k], x);
                    }
                }
            };
            for (size_t j = oc.size(); j-- > 0;) {
                double* b = &sb[6 * j];
                for (int k = 0; k < 3; ++k) { b[k] = INFINITY; b[3 + k] = -INFINITY; }
                if (oc.kind[j]) {
                    for (int32_t r = 0; r < oc.leaf_cnt[j]; ++r) tri_grow(b, (uint32_t)oc.refs[oc.leaf_off[j] + r]);
                } else {
                    for (int k = 0; k < 8; ++k) {
                        const int32_t c8 = oc.child[8 * j + k];
                        if (c8 < 0) continue;
                        for (int q = 0; q < 3; ++q) {
                            b[q] = std::fmin(b[q], sb[6 * (size_t)c8 + q]);
                            b[3 + q] = std::fmax(b[3 + q], sb[6 * (size_t)c8 + 3 + q]);
                        }
                    }
                }
            }
            // every node's box as the walk computes it: the root box, then per level the octant of the
            // parent's box with c = (mn + mx) / 2 (path_f64.h walk_node_slots; DFS pre-order: parents first)
            std::vector<double> nb(6 * oc.size());
            for (size_t j = 0; j < oc.size(); ++j) {
                if (oc.parent[j] < 0) {
                    std::memcpy(&nb[6 * j], rbox, sizeof rbox);
                    continue;
                }
                const double* pb = &nb[6 * (size_t)oc.parent[j]];
                const uint32_t oi = (uint32_t)oc.slot[j];
                for (int k = 0; k < 3; ++k) {
                    const double c = (pb[k] + pb[3 + k]) / 2.0;
                    const bool hi = ((oi >> (2 - k)) & 1u) != 0;
                    nb[6 * j + k] = hi ? c : pb[k];
                    nb[6 * j + 3 + k] = hi ? pb[3 + k] : c;
                }
            }
            // parent ordinals (pid, the slot walk's rows: scene_layout.h KidSlot), DFS order, over all meshes
            std::vector<int32_t> pid(oc.size(), -1);
            for (size_t j = 0; j < oc.size(); ++j)
                if (!oc.kind[j]) {
                    pid[j] = (int32_t)(p.node_box.size() / 6);
                    p.node_box.insert(p.node_box.end(), &nb[6 * j], &nb[6 * j] + 6);
                }
            dm.root_pid = oc.size() > 0 && !oc.kind[0] ? pid[0] : -1;
            for (size_t j = 0; j < oc.size(); ++j)  // each parent's own parent, as a pid (the slot walk's pops
                if (!oc.kind[j]) p.pid_up.push_back(oc.parent[j] >= 0 ? pid[oc.parent[j]] : -1);  // without anc)
            // the 16-bit code range: the cull box's min - E .. min + 2E per axis (E its largest extent)
            double E = 0.0;
            for (int k = 0; k < 3; ++k) E = std::fmax(E, dm.cull_box[3 + k] - dm.cull_box[k]);
            for (int k = 0; k < 3; ++k) dm.tight_base[k] = dm.cull_box[k] - E;
            dm.tight_step = 3.0 * E / (double)rt::kTightTop;
            dm.root_exist = 0;
            if (oc.size() > 0 && !oc.kind[0])
                for (int q = 0; q < 8; ++q) dm.root_exist |= (oc.child[q] >= 0 ? 1 : 0) << q;
            for (size_t j = 0; j < oc.size(); ++j) {
                if (oc.kind[j]) continue;  // rows for parents only (row pid[j])
                for (int k = 0; k < 8; ++k) {
                    const int32_t c8 = oc.child[8 * j + k];
                    double b[6] = {0, 0, 0, 0, 0, 0};
                    if (c8 >= 0)
                        for (int q = 0; q < 3; ++q) {
                            b[q] = sb[6 * (size_t)c8 + q] - dm.cull_pad;
                            b[3 + q] = sb[6 * (size_t)c8 + 3 + q] + dm.cull_pad;
                        }
                    int32_t e = p.kids[8 * (j + (size_t)dm.node_base) + k];
                    if (e >= 0) {  // a parent: its row (pid) and its own existence mask (KidSlot)
                        e = pid[c8];
                        if (e >= slot_max) slots_ok = false;  // checked after the loop: no slot tables
                        uint32_t ex = 0;
                        for (int q = 0; q < 8; ++q) ex |= (oc.child[8 * (size_t)c8 + q] >= 0 ? 1u : 0u) << q;
                        e = rt::slot_parent(e, ex);
                    }
                    bool exact = true;
                    p.slots.push_back(make_slot(e, dm, b, &exact));
                    if (!exact) slots_ok = false;  // a clamped bound code: no slot tables (make_slot)
                }
            }
        }
        p.meshes.push_back(dm);
    }
    if (!slots_ok) {  // the node_kids walk: no slot rows, and no parent boxes (only the slot walk's pops read them)
        p.slots.clear();
        p.pid_up.clear();
        p.node_box.clear();
    }
    for (const Object& o : sc.objects) {
        rt::DevObject d{};
        d.geom = o.geom;
        d.brdf = o.brdf;
        d.mesh = o.mesh;
        d.ph_power = o.ph_power;
        cp3(d.emitted, o.emitted);
        cp3(d.k, o.k);
        cp3(d.pos, o.pos);
        d.r = o.r;
        cp3(d.n, o.n);
        d.ph_kd = o.ph_kd;
        d.ph_ks = o.ph_ks;
        cp3(d.color_d, o.color_d);
        cp3(d.color_s, o.color_s);
        d.emissive = (o.emitted.x != 0.0 || o.emitted.y != 0.0 || o.emitted.z != 0.0) ? 1 : 0;
        d.axis = -1;
        if (o.geom == RT_GEOM_PLANE) {
            const double n3[3] = {o.n.x, o.n.y, o.n.z};
            int nz = 0, ax = -1;
            for (int k = 0; k < 3; ++k)
                if (n3[k] != 0.0) { ++nz; ax = k; }
            if (nz == 1 && std::fabs(n3[ax]) == 1.0) d.axis = ax;
        }
        p.objects.push_back(d);
    }
    // diffuse objects: kd / pi and the NEE term's Le_light * kd / pi, with the device's operations
    // (path_f64.h brdf_eval: ld3(k) * FRAC_1_PI; integrator_f64.h: mult(Le, f)), so the same bits
    const double FRAC_1_PI = 0.318309886183790671537767526745028724;  // path_f64.h FRAC_1_PI
    for (rt::DevObject& d : p.objects) {
        if (d.brdf != rt::BRDF_DIFFUSE) continue;
        for (int k = 0; k < 3; ++k) d.kpi[k] = d.k[k] * FRAC_1_PI;
        if (sc.light >= 0 && sc.light < (int)p.objects.size())
            for (int k = 0; k < 3; ++k) d.lef[k] = p.objects[sc.light].emitted[k] * d.kpi[k];
    }
    return RT_OK;
}

// Groups objects for the compact trace (axis planes per axis, spheres, everything else).
void fill_compact(const Packed& p, rt::CompactTab* ds, int32_t* compact) {
    int nax[3] = {0, 0, 0}, ns = 0, ng = 0;
    bool ok = p.objects.size() <= (size_t)rt::kMaxCompactObjects;
    for (size_t i = 0; i < p.objects.size(); ++i) {
        const rt::DevObject& o = p.objects[i];
        if (o.geom == rt::GEOM_PLANE && o.axis >= 0) {
            // A later axis plane at the same coordinate as an earlier one yields the same t for
            // every ray (the axis path divides (pos_k - o_k) by d_k only), so it can never be the
            // nearest hit (ties go to the lower index, scene.rs:278) nor change a shadow test:
            // leave it out (cornell_box.toml's "wall behind camera" repeats the right wall).
            bool dup = false;
            for (int j = 0; j < nax[o.axis]; ++j) dup |= ds->ax_pos[o.axis][j] == o.pos[o.axis];
            if (dup) continue;
            if (nax[o.axis] == rt::kMaxAxisPlanes) { ok = false; break; }
            ds->ax_idx[o.axis][nax[o.axis]] = (int32_t)i;
            ds->ax_pos[o.axis][nax[o.axis]] = o.pos[o.axis];
            ++nax[o.axis];
        } else if (o.geom == rt::GEOM_SPHERE) {
            if (ns == rt::kMaxSpheres) { ok = false; break; }
            ds->sph_idx[ns] = (int32_t)i;
            ds->sph[ns][0] = o.pos[0];
            ds->sph[ns][1] = o.pos[1];
            ds->sph[ns][2] = o.pos[2];
            ds->sph[ns][3] = o.r * o.r;
            ++ns;
        } else {
            if (ng == rt::kMaxGeneric) { ok = false; break; }
            ds->gen_idx[ng++] = (int32_t)i;
        }
    }
    *compact = ok ? 1 : 0;
    for (int k = 0; k < 3; ++k) ds->n_ax[k] = ok ? nax[k] : 0;
    ds->n_sph = ok ? ns : 0;
    ds->n_gen = ok ? ng : 0;
    ds->last_mesh_g = -1;
    for (int g = 0; g < ds->n_gen; ++g)
        if (p.objects[ds->gen_idx[g]].geom == rt::GEOM_MESH) ds->last_mesh_g = g;
    ds->gen_analytic = 0;
    for (int g = 0; g < rt::kMaxGeneric; ++g) {
        ds->gen_mesh[g] = -1;
        if (g >= ds->n_gen) continue;
        const rt::DevObject& o = p.objects[ds->gen_idx[g]];
        if (o.geom == rt::GEOM_SPHERE || o.geom == rt::GEOM_PLANE) ds->gen_analytic |= 1u << g;
        if (o.geom == rt::GEOM_MESH && o.mesh >= 0 && o.mesh < (int)p.meshes.size() && p.meshes[o.mesh].n_nodes > 0) {
            const rt::DevMesh& m = p.meshes[o.mesh];
            ds->gen_mesh[g] = o.mesh;
            for (int k = 0; k < 6; ++k) ds->gen_cull32[g][k] = m.cull32[k];
            ds->gen_cull32[g][6] = m.cull32_s;
        }
    }
}

// f32 perf-mode tables (scene_layout.h: Obj32 / Bvh32 / Tri32). BVH boxes are rounded outward and
// padded by a few f32 ulps of their largest coordinate, so the f32 slab test never culls a box the
// f64 one would enter; off32 (the hit-point offset) is 2^-16 of the scene's largest coordinate.
float f32_down(double x) {
    float f = (float)x;
    if ((double)f > x) f = std::nextafter(f, -INFINITY);
    return f;
}
float f32_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, INFINITY);
    return f;
}
void pack_f32(const Packed& p, std::vector<rt::Obj32>* objs, std::vector<rt::Bvh32>* bvh,
              std::vector<rt::Tri32>* tris, float* off32) {
    double scale = 1.0;
    auto grow = [&](double v) { scale = std::max(scale, std::fabs(v)); };
    for (const auto& o : p.objects) {
        rt::Obj32 q{};
        q.geom = o.geom;
        q.brdf = o.brdf;
        q.mesh = o.mesh;
        q.emissive = o.emissive;
        for (int k = 0; k < 3; ++k) {
            q.emitted[k] = (float)o.emitted[k];
            q.k[k] = (float)o.k[k];
            q.pos[k] = (float)o.pos[k];
            q.n[k] = (float)o.n[k];
            if (o.geom == rt::GEOM_SPHERE) grow(std::fabs(o.pos[k]) + o.r);
            else if (o.geom == rt::GEOM_PLANE && o.n[k] != 0.0) grow(o.pos[k]);
        }
        q.axis = o.geom == rt::GEOM_PLANE ? o.axis : -1;
        q.r = (float)o.r;
        q.r2 = (float)(o.r * o.r);
        objs->push_back(q);
    }
    for (const auto& m : p.meshes)
        for (int k = 0; k < 6; ++k) grow(m.root_box[k]);
    for (const auto& n : p.bvh) {
        rt::Bvh32 q{};
        double pad = 0.0;
        for (int k = 0; k < 3; ++k) pad = std::max({pad, std::fabs(n.bmin[k]), std::fabs(n.bmax[k])});
        pad *= 0x1p-20;
        for (int k = 0; k < 3; ++k) {
            q.bmin[k] = f32_down(n.bmin[k] - pad);
            q.bmax[k] = f32_up(n.bmax[k] + pad);
        }
        q.a = n.a;
        q.cnt_axis = n.count * 4 + n.axis;
        bvh->push_back(q);
    }
    for (const auto& t : p.btris) {
        rt::Tri32 q{};
        for (int k = 0; k < 3; ++k) {
            q.a[k] = (float)t.a[k];
            q.ab[k] = (float)t.ab[k];
            q.ac[k] = (float)t.ac[k];
            q.n[k] = (float)t.n[k];
        }
        tris->push_back(q);
    }
    *off32 = (float)std::max(1e-5, scale * 0x1p-16);
}

template <class T>
void put(std::vector<char>& blob, size_t* off, const std::vector<T>& v) {
    *off = align_up(blob.size(), 256);
    blob.resize(*off + v.size() * sizeof(T) + 16);
    if (!v.empty()) std::memcpy(blob.data() + *off, v.data(), v.size() * sizeof(T));
}

int upload(rt_scene* s, int device, rt::DevScene* out) {
    std::lock_guard<std::mutex> lk(s->mu);
    if ((int)s->dev.size() <= device) s->dev.resize(device + 1);
    DeviceCopy& dc = s->dev[device];
    if (!dc.ready) {
        const Packed& p = s->packed;
        std::vector<char> blob;
        size_t o_obj, o_mesh, o_kids, o_up, o_leaf, o_ltri, o_lid, o_tris, o_cum, o_tab, o_bvh, o_btri, o_bid;
        size_t o_obj32, o_bvh32, o_tri32;
        std::vector<rt::Obj32> obj32;
        std::vector<rt::Bvh32> bvh32;
        std::vector<rt::Tri32> tri32;
        float off32 = 0.f;
        pack_f32(p, &obj32, &bvh32, &tri32, &off32);
        std::vector<rt::CompactTab> tab(1);
        std::memset(tab.data(), 0, sizeof(rt::CompactTab));
        int32_t compact = 0;
        fill_compact(p, tab.data(), &compact);
        put(blob, &o_tab, tab);
        std::vector<rt::Compact32> tab32(1);
        {
            rt::Compact32& c = tab32[0];
            std::memset(&c, 0, sizeof c);
            const rt::CompactTab& t = tab[0];
            c.ok = compact;
            for (int k = 0; k < 3; ++k) {
                c.n_ax[k] = t.n_ax[k];
                for (int j = 0; j < rt::kMaxAxisPlanes; ++j) {
                    c.ax_idx[k][j] = t.ax_idx[k][j];
                    c.ax_pos[k][j] = (float)t.ax_pos[k][j];
                }
            }
            c.n_sph = t.n_sph;
            c.n_gen = t.n_gen;
            for (int j = 0; j < rt::kMaxSpheres; ++j) {
                c.sph_idx[j] = t.sph_idx[j];
                for (int q = 0; q < 4; ++q) c.sph[j][q] = (float)t.sph[j][q];
            }
            for (int j = 0; j < rt::kMaxGeneric; ++j) c.gen_idx[j] = t.gen_idx[j];
        }
        size_t o_tab32;
        put(blob, &o_tab32, tab32);
        put(blob, &o_obj, p.objects);
        put(blob, &o_mesh, p.meshes);
        put(blob, &o_kids, p.kids);
        put(blob, &o_up, p.up);
        put(blob, &o_leaf, p.leaves);
        put(blob, &o_ltri, p.ltris);
        put(blob, &o_lid, p.ltri_id);
        put(blob, &o_tris, p.tris);
        put(blob, &o_cum, p.cum_area);
        put(blob, &o_bvh, p.bvh);
        put(blob, &o_btri, p.btris);
        put(blob, &o_bid, p.btri_id);
        put(blob, &o_obj32, obj32);
        put(blob, &o_bvh32, bvh32);
        put(blob, &o_tri32, tri32);
        size_t o_slot;
        put(blob, &o_slot, p.slots);
        size_t o_nbox, o_pup;
        put(blob, &o_nbox, p.node_box);
        put(blob, &o_pup, p.pid_up);
        void* d = nullptr;
        HIP_TRY(hipMalloc(&d, blob.size()));
        hipError_t e = hipMemcpy(d, blob.data(), blob.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail(RT_E_HIP, std::string("scene upload: ") + hipGetErrorString(e));
        }
        char* b = (char*)d;
        rt::DevScene ds{};
        ds.objects = (const rt::DevObject*)(b + o_obj);
        ds.meshes = (const rt::DevMesh*)(b + o_mesh);
        ds.node_kids = (const int32_t*)(b + o_kids);
        ds.node_up = (const int2*)(b + o_up);
        ds.leaf_span = (const int2*)(b + o_leaf);
        ds.ltris = (const rt::LeafTri*)(b + o_ltri);
        ds.ltri_id = (const int32_t*)(b + o_lid);
        ds.tris = (const rt::DevTri*)(b + o_tris);
        ds.tri_cum_area = (const double*)(b + o_cum);
        ds.n_objects = (int32_t)p.objects.size();
        ds.ctab = (const rt::CompactTab*)(b + o_tab);
        ds.bvh = (const rt::DevBvhNode*)(b + o_bvh);
        ds.btris = (const rt::DevTri*)(b + o_btri);
        ds.btri_id = (const int32_t*)(b + o_bid);
        ds.obj32 = (const rt::Obj32*)(b + o_obj32);
        ds.bvh32 = (const rt::Bvh32*)(b + o_bvh32);
        ds.btris32 = (const rt::Tri32*)(b + o_tri32);
        ds.off32 = off32;
        ds.ctab32 = (const rt::Compact32*)(b + o_tab32);
        ds.compact = compact;
        ds.node_slot = p.slots.empty() ? nullptr : (const rt::KidSlot*)(b + o_slot);
        ds.node_box = p.slots.empty() ? nullptr : (const double*)(b + o_nbox);
        ds.pid_up = p.slots.empty() ? nullptr : (const int32_t*)(b + o_pup);
        ds.n_pid = p.slots.empty() ? 0 : (int32_t)p.pid_up.size();
        // RT_TEST_ANC_OFF (tests only): report more pids than a 16-bit ancestor column holds, so the role
        // pool's walkers pop through pid_up (the path of octrees with > 65536 parents)
        if (std::getenv("RT_TEST_ANC_OFF") && ds.n_pid > 0) ds.n_pid = 0x7FFFFFFF;
        ds.light = s->host.light;
        ds.light_pdf = 0.0;
        if (ds.light >= 0 && ds.light < (int32_t)p.objects.size()) {
            const rt::DevObject& L = p.objects[ds.light];
            const double PI = 3.14159265358979323846264338327950288;  // path_f64.h PI
            if (L.geom == rt::GEOM_SPHERE) ds.light_pdf = 1.0 / (4.0 * PI * L.r * L.r);  // geometry.rs:583
            else if (L.geom == rt::GEOM_MESH) ds.light_pdf = 1. / p.meshes[L.mesh].surface_area;  // :591
        }
        ds.n_meshes = (int32_t)p.meshes.size();
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

// The kernels' view of `p` on the uploaded scene `ds`: frame, tile, samples, seed, camera frame and the Cfg<F>
// feature bits (no output pointers, no scheduling).
rt::RenderArgs make_render_args(const rt_scene* s, const rt_render_params* p, int32_t compact);
rt::RenderArgs make_render_args(const rt_scene* s, const rt_render_params* p, const rt::DevScene& ds) {
    return make_render_args(s, p, ds.compact);
}
// The same from the host side alone (compact: fill_compact's answer, which is what upload gives DevScene::compact).
rt::RenderArgs make_render_args(const rt_scene* s, const rt_render_params* p, int32_t compact) {
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
    {
        bool phong = false, spec = false;
        for (const auto& o : s->host.objects) {
            phong |= o.brdf == RT_BRDF_PHONG;
            spec |= o.brdf == RT_BRDF_SPECULAR;
        }
        a.features = (s->host.meshes.empty() ? 0 : 1) | (phong ? 2 : 0) | (a.mis ? 4 : 0) | (compact ? 8 : 0) |
                     (spec ? 0 : 32);
        if ((p->flags & RT_FLAG_MESH_NEAREST) && !s->host.meshes.empty()) a.features |= 16;
        for (const auto& m : s->host.meshes) a.mesh_nodes = std::max(a.mesh_nodes, (int32_t)m.octree.size());
        a.all_flat = !s->packed.meshes.empty() && s->packed.meshes.size() <= (size_t)rt::kFlatMeshes;
        for (const auto& dm : s->packed.meshes) a.all_flat &= dm.flat != 0;
    }
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
    rt::RenderArgs a = make_render_args(s, p, ds);
    a.sub_out = d_sub;
    a.rgb_out = d_rgb;
    const bool fp32 = (p->flags & RT_FLAG_FP32) != 0;
    if (fp32) {
        // the f32 kernel covers diffuse / mirror BRDFs and sphere lights (every reference scene)
        for (const auto& o : s->host.objects)
            if (o.brdf == RT_BRDF_PHONG) return fail(RT_E_INVAL, "RT_FLAG_FP32: Phong BRDFs need the f64 path");
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
    cp3(s->cam_pos, s->host.cam_pos);
    cp3(s->cam_dir, s->host.cam_dir);
    const int rc = pack_scene(s.get());
    if (rc != RT_OK) return rc;
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
    int32_t compact = 0;
    {
        rt::CompactTab tab;
        fill_compact(s->packed, &tab, &compact);
    }
    return rt::list_pool_family(make_render_args(s, p, compact), !s->packed.slots.empty());
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
    rt::RenderArgs a = make_render_args(s, p, ds);
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
    int32_t compact = 0;
    {
        rt::CompactTab tab;
        fill_compact(s->packed, &tab, &compact);
    }
    const bool meshes = !s->host.meshes.empty();
    if (form == RT_DIAG_FUSED_G0 && (meshes || !compact))
        return fail(RT_E_INVAL, std::string(who) + ": the mesh-free fused form needs a compact scene without meshes");
    if (form >= RT_DIAG_SPLIT_SLOTS && (!meshes || !compact))
        return fail(RT_E_INVAL, std::string(who) + ": this form needs a compact scene with meshes");
    if (form == RT_DIAG_SPLIT_SLOTS && s->packed.slots.empty())
        return fail(RT_E_INVAL, std::string(who) + ": the slot-walk form needs the scene's slot tables");
    if (form == RT_DIAG_SPLIT_FLAT) {
        bool all_flat = s->packed.meshes.size() <= (size_t)rt::kFlatMeshes;
        for (const auto& dm : s->packed.meshes) all_flat &= dm.flat != 0;
        if (!all_flat) return fail(RT_E_INVAL, std::string(who) + ": the flat-query form needs flat octrees only");
    }
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
    int32_t compact = 0;
    {
        rt::CompactTab tab;
        fill_compact(scene->packed, &tab, &compact);
    }
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
    const rt::RenderArgs a = make_render_args(scene, &p, ds.compact);  // the Cfg bits of a render with these flags
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
