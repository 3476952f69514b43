// C ABI (include/rt_ffi.h): scene handles and views, and the per-device upload of the packed scene
// (host/scene_pack.hpp).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "api_common.hpp"

using namespace rt::api;

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

int finish_scene(rt::host::Scene&& sc, rt_scene** out) {
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

}  // namespace

namespace rt::api {

SceneData::~SceneData() {
    for (auto& d : dev)
        if (d.blob) (void)hipFree(d.blob);
    pool.clear();
}

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

}  // namespace rt::api

extern "C" {

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

}  // extern "C"
