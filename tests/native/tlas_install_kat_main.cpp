// Stand-alone known-answer program for the host-only half of a TLAS installation (csrc/tt_tlas_host.h): the checks
// of tt_scene_update_tlas, the shape of the install launch, the staging blob and the host mirror's update, on the
// cases tests/test_tlas_build_host.py writes to a file. Built with -fsanitize=address,undefined: every array is a
// heap vector of exactly the stated size and absent arrays are null, so a check that reads past what the caller
// supplied, or a plan that writes past the region, is reported. No GPU, no Python in the run.
//
// File (little endian u32 words): n_cases, then per case: capacity, n_idx_scene, n_mesh, prev_nodes, n_nodes, n_idx,
// mask (bit 0 nodes present, 1 indices present), expect_status, then n_nodes x 20 words of nodes and n_idx indices
// (each only when present).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tt_tlas_host.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

// tt_install_tlas_kernel's stores, thread by thread, into exactly sized arrays
static void run_plan(const tt_tlas::Plan& p, const std::vector<uint8_t>& stage, std::vector<tt_cwbvh_node>& region,
                     std::vector<int32_t>& tlas) {
    const size_t unit = 16;
    for (uint32_t i = 0; i < p.blocks * tt_tlas::kInstallBlock; i++) {
        if (i < p.units) {
            uint8_t v[16] = {0};
            if (i < p.copy_units) std::memcpy(v, stage.data() + (size_t)i * unit, unit);
            std::memcpy(reinterpret_cast<uint8_t*>(region.data()) + (size_t)i * unit, v, unit);
        }
        if (i < p.n_idx) std::memcpy(&tlas[i], stage.data() + p.idx_offset + (size_t)i * 4, 4);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t n_cases = 0, bad = 0;
    if (!rd(f, &n_cases, 4)) return 2;
    static_assert(sizeof(tt_cwbvh_node) == 80, "20 words per node");
    for (uint32_t c = 0; c < n_cases; c++) {
        uint32_t h[8];
        if (!rd(f, h, sizeof(h))) return 2;
        const uint32_t capacity = h[0], n_idx_scene = h[1], n_mesh = h[2], prev = h[3], n_nodes = h[4], n_idx = h[5], mask = h[6];
        std::vector<tt_cwbvh_node> nodes((mask & 1u) ? n_nodes : 0);
        std::vector<int32_t> idx((mask & 2u) ? n_idx : 0);
        if (!rd(f, nodes.data(), nodes.size() * sizeof(tt_cwbvh_node)) || !rd(f, idx.data(), idx.size() * 4)) return 2;
        tt_tlas::Check k;
        const tt_status st = tt_tlas::check_install((mask & 1u) && n_nodes ? nodes.data() : nullptr, n_nodes, capacity,
                                                    (mask & 2u) && n_idx ? idx.data() : nullptr, n_idx, n_idx_scene, n_mesh, k);
        bool good = (uint32_t)st == h[7] && (st == TT_OK) == k.why.empty();
        if (st == TT_OK && good) {
            good = good && !k.visit.empty() && k.visit[0] == 0 && k.visit.size() <= n_nodes;
            const tt_tlas::Plan p = tt_tlas::plan_install(n_nodes, prev, n_idx);
            good = good && p.n_nodes + p.n_clear == (prev > n_nodes ? prev : n_nodes) && p.n_nodes + p.n_clear <= capacity;
            good = good && p.units == 5u * (p.n_nodes + p.n_clear) && p.copy_units == 5u * n_nodes;
            good = good && (uint64_t)p.blocks * tt_tlas::kInstallBlock >= p.threads && p.threads >= p.units && p.threads >= n_idx;
            std::vector<uint8_t> stage(p.stage_bytes, 0xA5);  // exactly the plan's bytes
            tt_tlas::fill_stage(p, nodes.data(), idx.data(), stage.data());
            // the device side: the region as it was (prev nodes of another TLAS, zeros behind), the old indices
            tt_cwbvh_node old_node;
            std::memset(&old_node, 0x5A, sizeof(old_node));
            tt_cwbvh_node zero;
            std::memset(&zero, 0, sizeof(zero));
            std::vector<tt_cwbvh_node> region(capacity, zero);
            for (uint32_t i = 0; i < prev; i++) region[i] = old_node;
            std::vector<int32_t> tlas(n_idx_scene, -7);
            run_plan(p, stage, region, tlas);
            for (uint32_t i = 0; i < capacity; i++)
                good = good && std::memcmp(&region[i], i < n_nodes ? &nodes[i] : &zero, sizeof(zero)) == 0;
            good = good && tlas == idx;
            good = good && tt_tlas::used_nodes(region.data(), capacity) <= n_nodes;
            // the mirror of a scene of its own: BLAS nodes behind the region stay, the flags follow the walk
            {
                std::vector<tt_cwbvh_node> mirror(capacity + 3, old_node);
                for (uint32_t i = prev; i < capacity; i++) mirror[i] = zero;
                good = good && tt_tlas::used_nodes(mirror.data(), capacity) == prev;
                std::vector<int32_t> mt(n_idx_scene, -7);
                std::vector<uint8_t> flags(capacity + 3, 0u);
                std::vector<uint32_t> list;
                for (uint32_t i = 0; i < prev; i += 2) {
                    flags[i] = 1u;
                    list.push_back(i);
                }
                tt_tlas::apply_mirror(p, nodes.data(), idx.data(), k, false, mirror, mt, flags, list);
                for (uint32_t i = 0; i < capacity + 3; i++) {
                    const tt_cwbvh_node* want = i < n_nodes ? &nodes[i] : i < capacity ? &zero : &old_node;
                    good = good && std::memcmp(&mirror[i], want, sizeof(zero)) == 0;
                }
                std::vector<uint8_t> wantf(capacity + 3, 0u);
                for (uint32_t n : k.visit) wantf[n] = 1u;
                good = good && flags == wantf && list == k.visit && mt == idx;
                std::vector<uint8_t> blas(capacity + 3, 0u);
                blas[capacity] = 1u;
                good = good && tt_tlas::region_capacity(blas, capacity + 3) == capacity &&
                       tt_tlas::region_capacity(blas, capacity ? capacity - 1 : 0) == (capacity ? capacity - 1 : 0);
            }
            // the mirror of a frame slot: its TLAS nodes alone
            {
                std::vector<tt_cwbvh_node> mirror(prev, old_node);
                std::vector<int32_t> mt(n_idx_scene, -7);
                std::vector<uint8_t> flags(prev, 1u);
                std::vector<uint32_t> list;
                tt_tlas::apply_mirror(p, nodes.data(), idx.data(), k, true, mirror, mt, flags, list);
                good = good && mirror.size() == n_nodes && flags.size() == n_nodes && list == k.visit && mt == idx &&
                       std::memcmp(mirror.data(), nodes.data(), (size_t)n_nodes * sizeof(zero)) == 0;
            }
        }
        if (!good) {
            bad++;
            std::printf("case %u: status %d (expected %u): %s\n", c, (int)st, h[7], k.why.c_str());
        }
    }
    std::fclose(f);
    std::printf("%u cases, %u mismatches\n", n_cases, bad);
    return bad ? 1 : 0;
}
