// Stand-alone known-answer program for the walk tt_object_build_device runs on its host node mirror
// (csrc/tt_assemble_host.h, walk_object with no host triangles): on the cases tests/test_object_build_host.py writes
// to a file, the walk without triangles must reach what the walk with triangles reaches, refuse what it refuses,
// leave max_matdat alone, and count the triangles the leaves name (a built BLAS names each of its n once).
// Built with -fsanitize=address,undefined: every array is a heap vector of exactly the stated size, and the
// triangle-less walk is handed no triangle array at all. No GPU, no Python in the run.
//
// File (little endian u32 words): n_cases, then per case: n_nodes, n_tris, root, expect_ok, nodes (80 B each),
// tris (88 B each).
#include <cstdio>
#include <string>
#include <vector>

#include "tt_assemble_host.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t n_cases = 0, bad = 0;
    if (!rd(f, &n_cases, 4)) return 2;
    for (uint32_t c = 0; c < n_cases; c++) {
        uint32_t h[4];
        if (!rd(f, h, sizeof(h))) return 2;
        std::vector<tt_cwbvh_node> nodes(h[0]);
        std::vector<tt_cuda_triangle> tris(h[1]);
        if (!rd(f, nodes.data(), nodes.size() * sizeof(tt_cwbvh_node)) ||
            !rd(f, tris.data(), tris.size() * sizeof(tt_cuda_triangle)))
            return 2;
        tt_asm::ObjectWalk with, without;
        const bool ok_with = tt_asm::walk_object(nodes.data(), h[0], tris.data(), h[1], h[2], with);
        const bool ok = tt_asm::walk_object(nodes.data(), h[0], nullptr, h[1], h[2], without);
        bool good = ok == (h[3] != 0) && ok == ok_with && without.why == with.why && (ok || !without.why.empty());
        if (ok) {
            good = good && without.reach == with.reach && without.leaf_tris == with.leaf_tris && without.max_matdat == 0;
            good = good && (h[2] != 0 || without.leaf_tris == h[1]);  // from root 0 a built BLAS names every triangle
        }
        if (!good) {
            bad++;
            std::printf("case %u: ok %d / %d (%s), leaf triangles %llu of %u\n", c, (int)ok, (int)ok_with, without.why.c_str(),
                        (unsigned long long)without.leaf_tris, h[1]);
        }
    }
    std::fclose(f);
    std::printf("%u cases, %u mismatches\n", n_cases, bad);
    return bad ? 1 : 0;
}
