// Stand-alone driver of csrc/tt_refit_items_host.h (the host-only checks of tt_blas_refit_many), for the host
// sanitizers: item lists built here, every array exactly as long as the checks may read, the status and a word of
// the reason compared. Prints "<n> cases, <m> mismatches"; exit status 0 when m == 0.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tt_refit_items_host.h"

namespace {

struct Mesh {  // one deforming mesh: n triangles over 3 n vertices of stride 6, cut into parts
    std::vector<float> v;
    std::vector<int32_t> idx, leaf;
    std::vector<tt_blas_refit_part> parts;
    Mesh(uint32_t n, const std::vector<uint32_t>& cuts) : v((size_t)18 * n, 0.5f), idx((size_t)3 * n), leaf(n) {
        for (uint32_t i = 0; i < 3 * n; i++) idx[i] = (int32_t)(i % (3 * n));
        for (uint32_t i = 0; i < n; i++) leaf[i] = (int32_t)(n - 1 - i);
        for (size_t k = 0; k + 1 < cuts.size(); k++) {
            tt_blas_refit_part p{};
            p.vertices = v.data();
            p.n_vertices = 3 * n;
            p.vertex_stride = 6;
            p.indices = idx.data() + 3 * cuts[k];
            p.n_tris = cuts[k + 1] - cuts[k];
            p.first_tri = cuts[k];
            parts.push_back(p);
        }
    }
    tt_blas_refit_item item(uint32_t mesh_index) const {
        tt_blas_refit_item it{};
        it.mesh_index = mesh_index;
        it.n_tris = (uint32_t)leaf.size();
        it.leaf_of_triangle = leaf.data();
        it.parts = parts.data();
        it.n_parts = (uint32_t)parts.size();
        return it;
    }
};

int cases = 0, mismatches = 0;

void expect(const char* name, const std::vector<tt_blas_refit_item>& items, const std::vector<tt_mesh_data>& md, uint32_t scene_tris,
            uint32_t flags, tt_status want, const char* word) {
    std::string why;
    const tt_status got = tt_refit_items::check(items.empty() ? nullptr : items.data(), (uint32_t)items.size(), md.data(),
                                                (uint32_t)md.size(), scene_tris, flags, why);
    cases++;
    if (got != want || why.find(word) == std::string::npos) {
        mismatches++;
        std::printf("MISMATCH %s: status %d (want %d), why \"%s\" (want \"%s\")\n", name, (int)got, (int)want, why.c_str(), word);
    }
}

}  // namespace

int main() {
    // records 0..3: three BLASes, records 2 and 3 over the same one
    std::vector<tt_mesh_data> md(4);
    std::memset(md.data(), 0, sizeof(tt_mesh_data) * md.size());
    const int node[4] = {8, 20, 40, 40}, tri[4] = {0, 100, 400, 400};
    for (int i = 0; i < 4; i++) {
        md[i].NodeOffset = node[i];
        md[i].TriOffset = tri[i];
        md[i].mesh_data_bvh_offsets = node[i];
    }
    const uint32_t scene_tris = 1000;
    Mesh a(100, {0, 100}), b(300, {0, 1, 257, 300}), c(600, {0, 299, 600});
    const tt_status INV = TT_ERR_INVALID_ARG;
    expect("good", {a.item(0), b.item(1), c.item(2)}, md, scene_tris, 0, TT_OK, "");
    expect("good, device flag", {c.item(3), a.item(0)}, md, scene_tris, TT_TRACE_DEVICE_PTRS, TT_OK, "");
    expect("empty", {}, md, scene_tris, 0, INV, "no items");
    expect("mesh index", {a.item(4)}, md, scene_tris, 0, INV, "out of range");
    expect("twice", {a.item(0), b.item(1), a.item(0)}, md, scene_tris, 0, INV, "item 0 too");
    expect("shared BLAS", {c.item(2), a.item(0), c.item(3)}, md, scene_tris, 0, INV, "shares NodeOffset");
    expect("beyond the scene", {c.item(2)}, md, 999, 0, INV, "exceeds the scene");
    {
        std::vector<tt_mesh_data> m2 = md;
        m2[1].mesh_data_bvh_offsets = 21;
        expect("root", {b.item(1)}, m2, scene_tris, 0, TT_ERR_UNSUPPORTED, "root is not its first node");
    }
    {
        Mesh g(300, {0, 1, 257, 300});
        g.parts[1].vertex_stride = 5;
        expect("stride", {g.item(1)}, md, scene_tris, 0, INV, "part 1: vertex_stride < 6");
    }
    {
        Mesh g(300, {0, 1, 257, 300});
        g.parts.erase(g.parts.begin() + 1);
        expect("gap", {g.item(1)}, md, scene_tris, 0, INV, "gap: triangles [1, 257)");
    }
    {
        Mesh g(300, {0, 1, 257, 300});
        g.parts[2].first_tri = 256;  // overlaps part 1; its indices pointer moves with it
        g.parts[2].indices = g.idx.data() + 3 * 256;
        g.parts[2].n_tris = 44;
        expect("overlap", {g.item(1)}, md, scene_tris, 0, INV, "overlaps");
    }
    {
        Mesh g(300, {0, 1, 257, 300});
        g.parts.pop_back();
        expect("gap at the end", {g.item(1)}, md, scene_tris, 0, INV, "gap: triangles [257, 300)");
    }
    {
        Mesh g(100, {0, 100});
        g.idx[299] = 300;
        expect("index", {g.item(0)}, md, scene_tris, 0, INV, "index 300 out of range");
        expect("index, device flag", {g.item(0)}, md, scene_tris, TT_TRACE_DEVICE_PTRS, TT_OK, "");
    }
    {
        Mesh g(100, {0, 100});
        g.leaf[99] = 100;
        expect("leaf", {g.item(0)}, md, scene_tris, 0, INV, "leaf_of_triangle[99]");
    }
    {
        Mesh g(100, {0, 100});
        tt_blas_refit_item it = g.item(0);
        it.leaf_of_triangle = nullptr;
        expect("null leaf", {it}, md, scene_tris, 0, INV, "null");
        g.parts[0].vertices = nullptr;
        expect("null vertices", {g.item(0)}, md, scene_tris, 0, INV, "part 0: null");
    }
    std::printf("%d cases, %d mismatches\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
