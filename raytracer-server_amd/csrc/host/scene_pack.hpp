// Scene packing: a loaded rt::host::Scene turned into the tables the kernels read (device/scene_layout.h), once per
// scene and without a device (host code, -ffp-contract=off); the C ABI's upload only lays them out in one blob and
// copies it. tools/pack_dump.cpp prints a digest of every table (tests/test_scene_pack.py).
#pragma once

#include "../device/scene_layout.h"
#include "scene_host.hpp"

namespace rt::host {

// The BVH over the spheres of a scene that does not fit the compact tables (at least kObvhMinSpheres spheres), as
// rt_scene_object_bvh reports it. Host data: no kernel walks it and nothing of it is uploaded.
// nodes are in DFS pre-order as the mesh BVHs' (an inner node's left child is the next node, `a` its right child,
// `axis` the split axis; indices into `nodes`); a leaf (count > 0) holds refs[a .. a + count), scene object indices,
// ascending. rest = the scene's planes and meshes, in scene order. depth = the deepest leaf's (root 0).
constexpr int kObvhMinSpheres = 1;
struct ObjectBvh {
    std::vector<rt::DevBvhNode> nodes;
    std::vector<int32_t> refs, rest;
    int depth = 0;
};

// Host image of the device scene, packed once per scene.
struct Packed {
    std::vector<rt::DevObject> objects;
    std::vector<rt::DevMesh> meshes;
    std::vector<int32_t> kids;   // [node][8]
    std::vector<int2> up;        // [node]
    std::vector<int2> leaves;    // [leaf] {first ltri, count}
    std::vector<rt::DevTri> ltris;
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
    rt::CompactTab ctab;                 // fill_compact's tables, unused entries zero
    int32_t compact = 0;                 // DevScene::compact: the scene fits ctab
    rt::Compact32 ctab32;                // ctab in f32 (ok = compact)
    std::vector<rt::Obj32> obj32;        // f32 perf-mode tables (pack_f32)
    std::vector<rt::Bvh32> bvh32;
    std::vector<rt::Tri32> btris32;
    ObjectBvh obvh;                      // the BVH over the scene's spheres (host only; empty: no tree)
    float off32 = 0.f;                   // DevScene::off32
    double light_pdf = 0.0;              // DevScene::light_pdf
    bool phong = false, spec = false;    // some object has a Phong / a specular BRDF (RenderArgs::features)
    int32_t mesh_nodes = 0;              // the largest octree's node count (RenderArgs::mesh_nodes)
    bool all_flat = false;               // the scene has meshes, at most kFlatMeshes, every one flat (DevMesh::flat).
                                         // A scene without meshes is not flat: the diagnostics' flat-query form asks
                                         // for meshes before it asks this, so the one definition serves it too
};

inline void cp3(double* dst, const D3& v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; }

// Fills *p (empty on entry) from sc: RT_OK, or RT_E_INVAL with its message in *err (a mesh the tables cannot encode).
int pack_scene(const Scene& sc, Packed* p, std::string* err);

}  // namespace rt::host
