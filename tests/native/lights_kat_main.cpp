// lights_kat_main.cpp — the light validator, the mesh-tree builder and the scalar NEE reference as a stand-alone
// program (its own main, no Python in the run), for the host sanitizers. tests/test_lights_host.py writes one
// blob per scene: counts, then the arrays, then what the library answered in the test's own process; this
// program runs the same calls again and compares bytes.
//   blob: uint32 n[12] = {n_nodes, n_ltris, n_lmeshes, n_tris, n_mesh, n_rays, bounce, width, height, frames,
//         max_bounce, n_shadow}; float far; uint32 n_parent_tris; then LightNodes, LightTriangles, _LightMeshes,
//         AggTris, _MeshData, RayData[2 W H], samples[n_rays], shadow[n_shadow], the first parent's LightTriData
//         and normals (n_parent_tris) and its 2 n_parent_tris nodes.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/truetrace_scene.h"

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    int mismatches = 0;
    for (int a = 1; a < argc; a++) {
        FILE* f = std::fopen(argv[a], "rb");
        if (!f) return 2;
        uint32_t n[12], npt;
        float far_plane;
        if (std::fread(n, 4, 12, f) != 12 || std::fread(&far_plane, 4, 1, f) != 1 || std::fread(&npt, 4, 1, f) != 1) return 2;
        std::vector<tt_light_node> nodes, pnodes;
        std::vector<tt_light_tri> ltris, ptris;
        std::vector<tt_light_mesh> lmeshes;
        std::vector<tt_cuda_triangle> tris;
        std::vector<tt_mesh_data> md;
        std::vector<tt_ray_data> rays;
        std::vector<tt_light_sample> want_s;
        std::vector<tt_shadow_ray> want_r;
        std::vector<float> pnormals;
        const size_t wh = (size_t)n[7] * n[8];
        if (!read_vec(f, nodes, n[0]) || !read_vec(f, ltris, n[1]) || !read_vec(f, lmeshes, n[2]) || !read_vec(f, tris, n[3]) ||
            !read_vec(f, md, n[4]) || !read_vec(f, rays, 2 * wh) || !read_vec(f, want_s, n[5]) || !read_vec(f, want_r, n[11]) ||
            !read_vec(f, ptris, npt) || !read_vec(f, pnormals, 3 * (size_t)npt) || !read_vec(f, pnodes, 2 * (size_t)npt))
            return 2;
        std::fclose(f);
        tt_trace_params p{};
        p.n_rays = n[5];
        p.bounce = (int32_t)n[6];
        p.far_plane = far_plane;
        p.screen_width = n[7];
        p.screen_height = n[8];
        std::vector<tt_light_sample> got_s(n[5] ? n[5] : 1);
        std::vector<tt_shadow_ray> got_r(n[5] ? n[5] : 1);
        uint32_t cnt = 0;
        const tt_status st = tt_emit_nee_host(nodes.data(), n[0], ltris.data(), n[1], lmeshes.data(), n[2], tris.data(), n[3],
                                              md.data(), n[4], &p, rays.data(), (int32_t)n[9], (int32_t)n[10], 0, 0, got_s.data(),
                                              got_r.data(), &cnt);
        if (st != TT_OK || cnt != n[11]) mismatches++;
        if (n[5] && std::memcmp(got_s.data(), want_s.data(), sizeof(tt_light_sample) * n[5])) mismatches++;
        if (cnt == n[11] && cnt && std::memcmp(got_r.data(), want_r.data(), sizeof(tt_shadow_ray) * cnt)) mismatches++;
        // a refusal: the root's children behind it
        std::vector<tt_light_node> bad = nodes;
        bad[0].left = bad[0].left >= 0 ? 0 : bad[0].left;
        if (nodes[0].left >= 0 && tt_emit_nee_host(bad.data(), n[0], ltris.data(), n[1], lmeshes.data(), n[2], tris.data(), n[3],
                                                   md.data(), n[4], &p, rays.data(), 0, 1, 0, 0, nullptr, nullptr, &cnt) != TT_ERR_INVALID_ARG)
            mismatches++;
        // the first parent's tree, built again
        std::vector<tt_light_node> built(2 * (size_t)npt);
        tt_light_bounds root;
        if (tt_light_bvh_build_mesh(ptris.data(), pnormals.data(), npt, built.data(), &root) != TT_OK ||
            std::memcmp(built.data(), pnodes.data(), sizeof(tt_light_node) * built.size()))
            mismatches++;
        std::printf("%s: %u rays, %u emitted\n", argv[a], n[5], n[11]);
    }
    std::printf("%d scenes, %d mismatches\n", argc - 1, mismatches);
    return mismatches ? 1 : 0;
}
