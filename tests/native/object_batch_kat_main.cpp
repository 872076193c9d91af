// Stand-alone known-answer program for the host-only half of tt_objects_build_device
// (csrc/tt_object_batch_host.h): the argument checks of a mesh set and their per-mesh status, the concatenated
// triangle ranges, the staging blob's layout and contents, the globalized presort lists and the per-mesh status of a
// failed stage, on the cases tests/test_object_batch_host.py writes to a file. Built with
// -fsanitize=address,undefined: every array is a heap vector of exactly the stated size, absent arrays are null, and
// the blob has exactly the words the plan asks for. No GPU, no Python in the run.
//
// File (little endian u32 words): n_cases, then per case: n_meshes, expect_status, then per mesh: n_vertices,
// n_indices, mask (bit 0 positions, 1 normals, 2 tangents, 3 uvs, 4 indices, 5 matdat, 6 presorted),
// expect_mesh_status, then the present arrays in that order (3 nv, 3 nv, 4 nv, 2 nv, n_indices, n_indices / 3 and
// 3 * (n_indices / 3) words).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tt_object_batch_host.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

struct Mesh {
    std::vector<uint32_t> a[7];
    uint32_t nv = 0, ni = 0, mask = 0, expect = 0;
};

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
        uint32_t h[2];
        if (!rd(f, h, sizeof(h))) return 2;
        const uint32_t M = h[0];
        std::vector<Mesh> ms(M);
        std::vector<tt_mesh_input> in(M);
        std::vector<const int32_t*> pre(M, nullptr);
        for (uint32_t m = 0; m < M; m++) {
            Mesh& x = ms[m];
            uint32_t w[4];
            if (!rd(f, w, sizeof(w))) return 2;
            x.nv = w[0], x.ni = w[1], x.mask = w[2], x.expect = w[3];
            const size_t n = x.ni / 3, count[7] = {3 * (size_t)x.nv, 3 * (size_t)x.nv, 4 * (size_t)x.nv, 2 * (size_t)x.nv, x.ni, n, 3 * n};
            for (int k = 0; k < 7; k++)
                if (x.mask & (1u << k)) {
                    x.a[k].resize(count[k]);
                    if (!rd(f, x.a[k].data(), count[k] * 4)) return 2;
                }
            auto fp = [&](int k) { return (x.mask & (1u << k)) ? reinterpret_cast<const float*>(x.a[k].data()) : nullptr; };
            auto ip = [&](int k) { return (x.mask & (1u << k)) ? reinterpret_cast<const int32_t*>(x.a[k].data()) : nullptr; };
            in[m] = tt_mesh_input{fp(0), x.nv, fp(1), fp(2), fp(3), ip(4), x.ni, ip(5), {1.0f, 1.0f, 1.0f}};
            pre[m] = ip(6);
        }
        bool good = true;
        std::vector<tt_status> status(M, TT_OK);
        std::string why;
        const tt_status st = tt_batch::check_meshes(M ? in.data() : nullptr, M, M ? pre.data() : nullptr, status.data(), why);
        good = good && (uint32_t)st == h[1] && (st == TT_OK) == why.empty();
        int first = -1;
        for (uint32_t m = 0; m < M; m++) {
            good = good && (uint32_t)status[m] == ms[m].expect;
            if (first < 0 && status[m] != TT_OK) first = (int)m;
        }
        if (first >= 0) good = good && why.find("mesh " + std::to_string(first) + ":") != std::string::npos;
        std::string why2;  // the same without a status array
        good = good && tt_batch::check_meshes(M ? in.data() : nullptr, M, M ? pre.data() : nullptr, nullptr, why2) == st && why2 == why;
        if (st == TT_OK) {
            tt_batch::Plan p, q;
            tt_batch::make_plan(in.data(), M, true, p);
            tt_batch::make_plan(in.data(), M, false, q);
            good = good && q.words == 0 && q.off.empty() && q.start == p.start && p.start.size() == (size_t)M + 1 && p.start[0] == 0;
            std::vector<uint32_t> blob(p.words, 0xA5A5A5A5u);  // exactly the plan's words
            tt_batch::fill_blob(in.data(), M, p, blob.data());
            uint64_t at = 0;  // the arrays follow each other, 16-byte aligned, in mesh and field order
            for (uint32_t m = 0; m < M; m++) {
                const Mesh& x = ms[m];
                good = good && p.start[m + 1] - p.start[m] == x.ni / 3;
                const uint64_t off[6] = {p.off[m].pos, p.off[m].nrm, p.off[m].tan, p.off[m].uv, p.off[m].idx, p.off[m].mat};
                for (int k = 0; k < 6; k++) {
                    if (!(x.mask & (1u << k))) {
                        good = good && off[k] == tt_batch::kAbsent;
                        continue;
                    }
                    const size_t cnt = k == 5 ? x.ni / 3 : x.a[k].size();  // (matdat: n words)
                    good = good && off[k] == at && off[k] % 4 == 0 && off[k] + cnt <= p.words;
                    good = good && std::memcmp(blob.data() + off[k], x.a[k].data(), cnt * 4) == 0;
                    at += (cnt + 3) / 4 * 4;
                    for (uint64_t g = off[k] + cnt; g < at; g++) good = good && blob[g] == 0u;
                }
                if (pre[m]) {  // the list as the forest takes it
                    const uint32_t n = x.ni / 3;
                    std::vector<int32_t> g(3 * (size_t)n);
                    tt_batch::globalize_presort(pre[m], n, p.start[m], g.data());
                    for (size_t i = 0; i < g.size(); i++)
                        good = good && g[i] == pre[m][i] + (int32_t)p.start[m] && (uint32_t)g[i] >= p.start[m] && (uint32_t)g[i] < p.start[m + 1];
                }
            }
            good = good && at == p.words;
            // the staging copies, small meshes composed and large ones direct, must leave every array where the full
            // composition has it, for a threshold that sends nothing, some and every mesh directly
            for (uint64_t direct : {(uint64_t)~0ull, (uint64_t)200, (uint64_t)0}) {
                std::vector<uint32_t> staging(p.words, 0x5A5A5A5Au), devblob(p.words, 0xC3C3C3C3u);
                std::vector<tt_batch::Copy> copies;
                tt_batch::stage_copies(in.data(), M, p, direct, staging.data(), copies);
                uint64_t sent = 0;
                for (const tt_batch::Copy& k : copies) {
                    good = good && k.at + k.words <= p.words && k.words > 0;
                    if (k.at + k.words > p.words) break;
                    std::memcpy(devblob.data() + k.at, k.src, k.words * 4);
                    sent += k.words;
                }
                good = good && sent <= p.words && (direct != ~0ull || copies.size() == 1);
                for (uint32_t m = 0; m < M; m++) {
                    const Mesh& x = ms[m];
                    const uint64_t off[6] = {p.off[m].pos, p.off[m].nrm, p.off[m].tan, p.off[m].uv, p.off[m].idx, p.off[m].mat};
                    for (int k = 0; k < 6; k++)
                        if (x.mask & (1u << k)) {
                            const size_t cnt = k == 5 ? x.ni / 3 : x.a[k].size();
                            good = good && std::memcmp(devblob.data() + off[k], blob.data() + off[k], cnt * 4) == 0;
                        }
                }
            }
            // a failed stage's flags: every third mesh from the second
            std::vector<int> flags(M, 0);
            std::vector<tt_status> s2(M, TT_OK);
            for (uint32_t m = 1; m < M; m += 3) flags[m] = 1 + (int)m;
            const int lowest = tt_batch::mark_failed(flags.data(), M, TT_ERR_UNSUPPORTED, s2.data());
            good = good && lowest == (M > 1 ? 1 : -1) && tt_batch::mark_failed(flags.data(), M, TT_ERR_UNSUPPORTED, nullptr) == lowest;
            for (uint32_t m = 0; m < M; m++) good = good && s2[m] == (flags[m] ? TT_ERR_UNSUPPORTED : TT_OK);
        }
        if (!good) {
            bad++;
            std::printf("case %u: status %d (expected %u): %s\n", c, (int)st, h[1], why.c_str());
        }
    }
    std::fclose(f);
    std::printf("%u cases, %u mismatches\n", n_cases, bad);
    return bad ? 1 : 0;
}
