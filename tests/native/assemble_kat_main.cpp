// Stand-alone known-answer program for the host half of the GPU-resident objects (csrc/tt_assemble_host.h): the
// object validator and AccumulateData's layout sums on the cases tests/test_assemble_host.py writes to a file.
// Built with -fsanitize=address,undefined: every array is a heap vector of exactly the stated size, so a walk that
// reads one node or triangle too far is reported. No GPU, no Python in the run.
//
// File (little endian u32 words unless noted):
//   n_cases, then per case: n_nodes, n_tris, root, expect_ok, nodes (80 B each), tris (88 B each)
//   n_objects, tlas_region, then per object: n_nodes, n_tris, want_node_offset, want_tri_offset
//   want_n_nodes_total, want_n_tris_total
#include <cstdio>
#include <cstring>
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
        tt_asm::ObjectWalk w;
        const tt_status st = tt_asm::validate_object(nodes.data(), h[0], tris.data(), h[1], h[2], w);
        const bool ok = st == TT_OK;
        // a refusal carries a reason; an accepted object reaches its root, and its largest MatDat is one it holds
        bool good = ok == (h[3] != 0) && (ok || (st == TT_ERR_INVALID_ARG && !w.why.empty()));
        if (ok) {
            good = good && w.reach.size() == h[0] && w.reach[h[2]] == 1;
            bool seen = false;
            for (const tt_cuda_triangle& t : tris) seen = seen || t.MatDat == w.max_matdat;
            good = good && seen;
        }
        if (!good) {
            bad++;
            std::printf("case %u: status %d (%s), expected %s\n", c, st, w.why.c_str(), h[3] ? "TT_OK" : "a refusal");
        }
    }
    uint32_t n_obj = 0, region = 0;
    if (!rd(f, &n_obj, 4) || !rd(f, &region, 4)) return 2;
    std::vector<uint32_t> nn(n_obj), nt(n_obj), wn(n_obj), wt(n_obj), on(n_obj), ot(n_obj);
    for (uint32_t i = 0; i < n_obj; i++) {
        uint32_t r[4];
        if (!rd(f, r, sizeof(r))) return 2;
        nn[i] = r[0], nt[i] = r[1], wn[i] = r[2], wt[i] = r[3];
    }
    uint32_t want_total[2], tn = 0, tt = 0;
    if (!rd(f, want_total, sizeof(want_total))) return 2;
    std::fclose(f);
    std::string why;
    if (tt_asm::layout_counts(nn.data(), nt.data(), n_obj, region, on.data(), ot.data(), &tn, &tt, why) != TT_OK || on != wn ||
        ot != wt || tn != want_total[0] || tt != want_total[1]) {
        bad++;
        std::printf("layout differs (%s)\n", why.c_str());
    }
    // refusals of the arithmetic: an empty list, sums beyond 32 bits
    const uint32_t big[2] = {0xfffffff0u, 0x20u};
    if (tt_asm::layout_counts(nn.data(), nt.data(), 0, region, nullptr, nullptr, nullptr, nullptr, why) != TT_ERR_INVALID_ARG) bad++;
    if (tt_asm::layout_counts(big, big, 2, 0, nullptr, nullptr, &tn, &tt, why) != TT_ERR_INVALID_ARG || why.empty()) bad++;
    if (tt_asm::layout_counts(big, big, 1, 0x10u, on.data(), ot.data(), &tn, &tt, why) != TT_ERR_INVALID_ARG) bad++;
    std::printf("%u cases + layout, %u mismatches\n", n_cases, bad);
    return bad ? 1 : 0;
}
