// Scene packing (scene_pack.hpp): host code only, no HIP call.
#include "scene_pack.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../ab_knobs.h"

namespace rt::host {
namespace {

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

// BVH over one mesh's triangles for the nearest-triangle mode: median split of the triangle
// centroids along the longest axis, leaves of <= 4 triangles (or at depth kBvhMaxDepth - 1), nodes
// in DFS pre-order (DevBvhNode). Node boxes are the triangles' vertex bounds; the traversal's slab test pads
// them (near_box, DevMesh::cull_pad), so a triangle the ray hits is never culled.
// RT_BVH_SAH=0 selects the median-split build (A/B); default: binned SAH.
constexpr int kBins = 16;      // SAH bins per axis
constexpr int kSahDepth = 16;  // deeper BVH nodes split at the median (depth stays <= kBvhMaxDepth)
bool bvh_sah_enabled() { return rt::ab_knob("RT_BVH_SAH", 1) != 0; }

struct BvhItem { double lo[3], hi[3], c[3]; int32_t id; };
// The recursive build shared by the mesh BVHs (items = triangles) and the object BVH (items = spheres): nodes
// appended to `nodes` (child indices are indices into it); a leaf's run starts at leaf.first() and its items,
// sorted by id, go to leaf.push(id).
template <class Leaf>
struct BvhRec {
    std::vector<rt::DevBvhNode>& nodes;
    std::vector<BvhItem>& it;
    bool sah;
    Leaf& leaf;
    int depth_seen = 0;  // the deepest leaf (root = 0)
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
        auto left = [&](const BvhItem& x) {
            int q = (int)((x.c[ax] - clo[ax]) / ext * kBins);
            return std::min(kBins - 1, std::max(0, q)) < best_bin;
        };
        *mid = (size_t)(std::stable_partition(it.begin() + b, it.begin() + e, left) - it.begin());
        *ax_out = ax;
    }
    void build(size_t b, size_t e, int depth) {
        const size_t node = nodes.size();
        nodes.push_back(rt::DevBvhNode{});
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
            nd.a = leaf.first();
            nd.count = (int32_t)(e - b);
            depth_seen = std::max(depth_seen, depth);
            std::sort(it.begin() + b, it.begin() + e, [](const BvhItem& x, const BvhItem& y) { return x.id < y.id; });
            for (size_t i = b; i < e; ++i) leaf.push(it[i].id);
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
                                 [ax](const BvhItem& x, const BvhItem& y) { return x.c[ax] < y.c[ax] || (x.c[ax] == y.c[ax] && x.id < y.id); });
            }
            nd.axis = ax;
            build(b, mid, depth + 1);
            nd.a = (int32_t)nodes.size();  // index of the right child (global, for p.bvh)
            build(mid, e, depth + 1);
        }
        nodes[node] = nd;
    }
};

void build_bvh(Packed& p, const Mesh& m, int32_t tri_base) {
    const size_t n = m.num_triangles();
    std::vector<BvhItem> it(n);
    for (size_t t = 0; t < n; ++t) {
        const D3 v[3] = {m.vertices[m.indices[3 * t]], m.vertices[m.indices[3 * t + 1]], m.vertices[m.indices[3 * t + 2]]};
        BvhItem& x = it[t];
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
    struct TriLeaf {  // the leaf's triangles copied to btris, their global indices to btri_id
        Packed& p;
        int32_t tri_base;
        int32_t first() const { return (int32_t)p.btris.size(); }
        void push(int32_t id) {
            p.btris.push_back(p.tris[tri_base + id]);
            p.btri_id.push_back(tri_base + id);
        }
    } leaf{p, tri_base};
    BvhRec<TriLeaf> rec{p.bvh, it, bvh_sah_enabled(), leaf};
    if (n > 0) rec.build(0, n, 0);
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

// The object BVH (scene_pack.hpp ObjectBvh) of a scene that does not fit the compact tables: BvhRec's tree over the
// spheres (box = centre +- r per axis), the leaf runs of scene object indices, and the rest list (planes and meshes,
// scene order). Host data only: nothing of it is uploaded. A sphere with a non-finite centre or radius: no tree.
void build_object_bvh(Packed& p) {
    if (p.compact) return;
    ObjectBvh t;
    std::vector<BvhItem> it;
    for (size_t i = 0; i < p.objects.size(); ++i) {
        const rt::DevObject& o = p.objects[i];
        if (o.geom != rt::GEOM_SPHERE) {
            t.rest.push_back((int32_t)i);
            continue;
        }
        if (!(std::isfinite(o.pos[0]) && std::isfinite(o.pos[1]) && std::isfinite(o.pos[2]) && std::isfinite(o.r))) return;
        BvhItem x;
        x.id = (int32_t)i;
        for (int k = 0; k < 3; ++k) {
            x.lo[k] = o.pos[k] - std::fabs(o.r);
            x.hi[k] = o.pos[k] + std::fabs(o.r);
            x.c[k] = o.pos[k];
        }
        it.push_back(x);
    }
    if (it.size() < (size_t)kObvhMinSpheres) return;
    struct RefLeaf {
        std::vector<int32_t>& refs;
        int32_t first() const { return (int32_t)refs.size(); }
        void push(int32_t id) { refs.push_back(id); }
    } leaf{t.refs};
    BvhRec<RefLeaf> rec{t.nodes, it, bvh_sah_enabled(), leaf};
    rec.build(0, it.size(), 0);
    t.depth = rec.depth_seen;
    p.obvh = std::move(t);
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

// CompactTab in f32 (scene_layout.h Compact32), unused entries zero.
void fill_compact32(const rt::CompactTab& t, int32_t compact, rt::Compact32& c) {
    std::memset(&c, 0, sizeof c);
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

}  // namespace

// RT_OK, or RT_E_INVAL when the octree tables cannot encode the mesh (kid_leaf: leaf ids < 2^25). Parent
// ordinals beyond a KidSlot entry's range (>= kSlotMaxNode, counted over the scene's meshes) leave the scene
// without slot tables: its walks then read node_kids (walk_step<false>, the same result without the
// subtree culls).
int pack_scene(const Scene& sc, Packed* out, std::string* err) {
    Packed& p = *out;
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
                p.ltris.push_back(p.tris[dm.tri_base + t]);
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
                if (c8 >= 0 && oc.kind[c8] && leaf_of[c8] >= (1 << 25)) {  // kid_leaf's escape keeps leaf << 6 in an int32
                    *err = "mesh octree too large: leaf ids must stay below 2^25 (scene_layout.h kid_leaf)";
                    return RT_E_INVAL;
                }
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
    std::memset(&p.ctab, 0, sizeof p.ctab);
    fill_compact(p, &p.ctab, &p.compact);
    fill_compact32(p.ctab, p.compact, p.ctab32);
    pack_f32(p, &p.obj32, &p.bvh32, &p.btris32, &p.off32);
    build_object_bvh(p);
    if (sc.light >= 0 && sc.light < (int32_t)p.objects.size()) {
        const rt::DevObject& L = p.objects[sc.light];
        const double PI = 3.14159265358979323846264338327950288;  // path_f64.h PI
        if (L.geom == rt::GEOM_SPHERE) p.light_pdf = 1.0 / (4.0 * PI * L.r * L.r);  // geometry.rs:583
        else if (L.geom == rt::GEOM_MESH) p.light_pdf = 1. / p.meshes[L.mesh].surface_area;  // :591
    }
    for (const Object& o : sc.objects) {
        p.phong |= o.brdf == RT_BRDF_PHONG;
        p.spec |= o.brdf == RT_BRDF_SPECULAR;
    }
    for (const Mesh& m : sc.meshes) p.mesh_nodes = std::max(p.mesh_nodes, (int32_t)m.octree.size());
    p.all_flat = !p.meshes.empty() && p.meshes.size() <= (size_t)rt::kFlatMeshes;
    for (const rt::DevMesh& dm : p.meshes) p.all_flat &= dm.flat != 0;
    return RT_OK;
}

}  // namespace rt::host
