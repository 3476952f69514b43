// pack_dump scene.toml assets_dir: loads a scene and packs it (csrc/host/scene_host.cpp, scene_pack.cpp: host code
// only, no HIP library) and prints one line per table of the packed scene: name, element count and the 64-bit FNV-1a
// of the table's bytes; scalars as their value (floating point as %a). Two builds that print the same lines hand the
// kernels the same scene; when a GPU frame diverges, the first differing line names the table to look at.
// tests/test_scene_pack.py compares the lines with tests/golden/scene_pack_tables.txt. Built by `make pack_dump`.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../raytracer-server_amd/csrc/host/scene_host.hpp"
#include "../raytracer-server_amd/csrc/host/scene_pack.hpp"

static uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) {
        h ^= b[i];
        h *= 0x100000001b3ull;
    }
    return h;
}
template <class T>
static void row(const char* name, const T* v, size_t n) {
    std::printf("%s %zu %016llx\n", name, n, (unsigned long long)fnv1a(v, n * sizeof(T)));
}
template <class T>
static void row(const char* name, const std::vector<T>& v) {
    row(name, v.data(), v.size());
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: pack_dump scene.toml assets_dir\n");
        return 2;
    }
    rt::host::Scene sc;
    rt::host::Packed p;
    std::string err;
    int rc = rt::host::load_scene_toml(argv[1], argv[2], &sc, &err);
    if (rc == RT_OK) rc = rt::host::pack_scene(sc, &p, &err);
    if (rc != RT_OK) {
        std::fprintf(stderr, "pack_dump: %s (code %d)\n", err.c_str(), rc);
        return 1;
    }
    row("objects", p.objects);
    row("meshes", p.meshes);
    row("kids", p.kids);
    row("up", p.up);
    row("leaves", p.leaves);
    row("ltris", p.ltris);
    row("ltri_id", p.ltri_id);
    row("tris", p.tris);
    row("cum_area", p.cum_area);
    row("bvh", p.bvh);
    row("btris", p.btris);
    row("btri_id", p.btri_id);
    row("slots", p.slots);
    row("node_box", p.node_box);
    row("pid_up", p.pid_up);
    row("ctab", &p.ctab, 1);
    std::printf("compact %d\n", (int)p.compact);
    row("ctab32", &p.ctab32, 1);
    row("obj32", p.obj32);
    row("bvh32", p.bvh32);
    row("btris32", p.btris32);
    std::printf("off32 %a\n", (double)p.off32);
    std::printf("light_pdf %a\n", p.light_pdf);
    std::printf("phong %d\nspec %d\nmesh_nodes %d\nall_flat %d\n", (int)p.phong, (int)p.spec, (int)p.mesh_nodes,
                (int)p.all_flat);
    return 0;
}
