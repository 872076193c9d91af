// Stand-alone known-answer program for the host scene checks (csrc/tt_scene_check_host.h, and the object walk of
// csrc/tt_assemble_host.h on the same corpus): the cases tests/test_scene_check_host.py writes to a file, each with
// the status and the message it must give. Built with -fsanitize=address,undefined: every array is a heap vector
// of exactly the stated size and an absent array is null, so a walk that reads one element too far is reported.
// No GPU, no Python in the run.
//
// File (little endian u32 words unless noted): n_cases, then per case
//   mode, separate_tl, n_tl, n_bl, n_tris, n_tlas, n_mesh, expect_ok, msg_len, then msg_len bytes of message,
//   separate_tl ? n_tl TLAS-level nodes (80 B each) : nothing (the TLAS level reads the first n_tl of the next array)
//   n_bl BLAS-level nodes, n_tlas int32 TLASBVH8Indices, n_mesh mesh records (88 B each)
//   mode 2 only: the one mesh record to walk
// mode 0: Validator::run; 1: the TLAS-level walk alone; 2: walk_mesh alone; 3: tt_asm::walk_object from root 0
// (the triangles are n_tris zeroed records: only their count matters to the answer).
// What an accepted case reached goes to the second file, one line per case:
//   <case> T <tlas_visit in order> B <BLAS-reached nodes, sorted> K <root NodeOffset TriOffset of each key>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tt_assemble_host.h"
#include "tt_scene_check_host.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
template <class T>
static const T* ptr(const std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s cases.bin reached.txt\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "w");
    if (!f || !out) return 2;
    uint32_t n_cases = 0, bad = 0;
    if (!rd(f, &n_cases, 4)) return 2;
    for (uint32_t c = 0; c < n_cases; c++) {
        uint32_t h[9];
        if (!rd(f, h, sizeof(h))) return 2;
        const uint32_t mode = h[0], n_tl = h[2], n_bl = h[3], n_tris = h[4], n_tlas = h[5], n_mesh = h[6];
        std::string want(h[8], '\0');
        std::vector<tt_cwbvh_node> tl(h[1] ? n_tl : 0u), bl(n_bl);
        std::vector<int32_t> tlas(n_tlas);
        std::vector<tt_mesh_data> mesh(n_mesh), one(mode == 2u ? 1u : 0u);
        if (!rd(f, &want[0], want.size()) || !rd(f, tl.data(), tl.size() * sizeof(tt_cwbvh_node)) ||
            !rd(f, bl.data(), bl.size() * sizeof(tt_cwbvh_node)) || !rd(f, tlas.data(), tlas.size() * 4u) ||
            !rd(f, mesh.data(), mesh.size() * sizeof(tt_mesh_data)) || !rd(f, one.data(), one.size() * sizeof(tt_mesh_data)))
            return 2;
        bool ok;
        std::string why;
        if (mode == 3u) {
            const std::vector<tt_cuda_triangle> tris(n_tris);
            tt_asm::ObjectWalk w;
            ok = tt_asm::validate_object(ptr(bl), n_bl, ptr(tris), n_tris, 0u, w) == TT_OK;
            why = w.why;
            if (ok && (w.reach.size() != n_bl || !w.reach[0] || w.max_matdat != 0u)) why = "(walk record)";
        } else {
            const tt_check::SceneView s{h[1] ? ptr(tl) : ptr(bl), n_tl, ptr(bl), n_bl, ptr(tlas), n_tlas, ptr(mesh), n_mesh, n_tris};
            tt_check::Validator v(s);
            ok = mode == 0u ? v.run() : mode == 1u ? v.walk_tlas() : v.walk_mesh(one[0]);
            why = v.why;
            if (ok) {
                std::vector<uint32_t> b = v.blas_visit;
                std::sort(b.begin(), b.end());
                b.erase(std::unique(b.begin(), b.end()), b.end());
                std::fprintf(out, "%u T", c);
                for (uint32_t n : v.tlas_visit) std::fprintf(out, " %u", n);
                std::fprintf(out, " B");
                for (uint32_t n : b) std::fprintf(out, " %u", n);
                std::fprintf(out, " K");
                for (const tt_check::BlasKey& k : v.keys) std::fprintf(out, " %u %u %u", k.root, k.node_offset, k.tri_offset);
                std::fprintf(out, "\n");
            }
        }
        if (ok != (h[7] != 0u) || why != want) {
            bad++;
            std::printf("case %u (mode %u): %s (%s), expected %s (%s)\n", c, mode, ok ? "accepted" : "refused", why.c_str(),
                        h[7] ? "accepted" : "refused", want.c_str());
        }
    }
    std::fclose(f);
    std::fclose(out);
    std::printf("%u cases, %u mismatches\n", n_cases, bad);
    return bad ? 1 : 0;
}
