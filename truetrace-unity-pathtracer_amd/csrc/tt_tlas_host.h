// tt_tlas_host.h — the host-only half of a TLAS installation (tt_scene_update_tlas, tt_tlas_rebuild): the checks
// that keep a malformed TLAS from reaching a kernel, the capacity of a scene's TLAS region, the shape of the one
// install launch, and the host mirror's update. Plain C++ with no HIP in it, so a stand-alone program can run it
// under the host sanitizers (tests/native/tlas_install_kat_main.cpp).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/truetrace_hip.h"

namespace tt_tlas {

struct Check {
    std::vector<uint32_t> visit;  // the nodes the TLAS-level walk reached
    std::string why;
};

// Validator::walk(0, 0, 0, true) (tt_scene_api.hip) over the supplied nodes alone: IntersectBVH's index arithmetic
// at TLAS level (IntersectionKernels.compute:157-196). A child index must stay inside [0, n_nodes) -- the nodes
// behind them are zeroed by the installation, never read from the caller -- and a leaf slot inside [0, n_idx).
inline bool walk_tlas(const tt_cwbvh_node* nodes, uint32_t n_nodes, uint32_t n_idx, Check& k) {
    k.visit.clear();
    std::vector<uint8_t> seen(n_nodes, 0u);
    std::vector<uint32_t> work{0u};
    while (!work.empty()) {
        const uint32_t ni = work.back();
        work.pop_back();
        if (ni >= n_nodes) {
            k.why = "node index " + std::to_string(ni) + " out of range of the " + std::to_string(n_nodes) + " TLAS nodes";
            return false;
        }
        if (seen[ni]) continue;
        seen[ni] = 1u;
        k.visit.push_back(ni);
        const tt_cwbvh_node& n = nodes[ni];
        const uint32_t imask = n.e_imask >> 24;
        for (int c = 0; c < 8; c++) {
            const uint32_t meta = (n.meta[c >> 2] >> ((c & 3) * 8)) & 0xffu;
            const uint32_t low5 = meta & 0x1fu, bits = (meta >> 5) & 7u;
            if ((meta & 0x18u) == 0x18u) {
                if (bits != 1u) {
                    k.why = "inner meta with child bits != 1";
                    return false;
                }
                const uint32_t slot = low5 - 24u;
                const uint64_t child = (uint64_t)n.base_child + (uint32_t)__builtin_popcount(imask & ((1u << slot) - 1u));
                if (child >= n_nodes) {
                    k.why = "node index " + std::to_string(child) + " out of range of the " + std::to_string(n_nodes) + " TLAS nodes";
                    return false;
                }
                work.push_back((uint32_t)child);
            } else if (bits) {
                const uint32_t top = low5 + (31u - (uint32_t)__builtin_clz(bits));
                if (top >= 24u) {
                    k.why = "leaf meta spills into the internal-child bits";
                    return false;
                }
                for (uint32_t b = 0; b < 3; b++) {
                    if (!((bits >> b) & 1u)) continue;
                    const uint64_t t = (uint64_t)n.base_tri + low5 + b;
                    if (t >= n_idx) {
                        k.why = "TLAS leaf slot out of range";
                        return false;
                    }
                }
            }
        }
    }
    return true;
}

// Everything tt_scene_update_tlas checks before anything is enqueued. n_idx_scene, n_mesh: the scene's current
// TLASBVH8Indices and _MeshData counts; capacity: the nodes its TLAS region holds.
// check_counts: the part that reads no array (what is refused before the arrays are staged).
inline tt_status check_counts(const tt_cwbvh_node* nodes, uint32_t n_nodes, uint32_t capacity, const int32_t* idx,
                              uint32_t n_idx, uint32_t n_idx_scene, Check& k) {
    k.visit.clear();
    if (!nodes || !n_nodes || !idx || !n_idx) {
        k.why = "null or empty array";
        return TT_ERR_INVALID_ARG;
    }
    if (n_idx != n_idx_scene) {
        k.why = "n_tlas_indices " + std::to_string(n_idx) + " differs from the scene's " + std::to_string(n_idx_scene) +
                " (the number of mesh records cannot change)";
        return TT_ERR_INVALID_ARG;
    }
    if (n_nodes > capacity) {
        k.why = "n_tlas_nodes " + std::to_string(n_nodes) + " exceeds the TLAS region's capacity " + std::to_string(capacity);
        return TT_ERR_INVALID_ARG;
    }
    return TT_OK;
}
inline tt_status check_install(const tt_cwbvh_node* nodes, uint32_t n_nodes, uint32_t capacity, const int32_t* idx,
                               uint32_t n_idx, uint32_t n_idx_scene, uint32_t n_mesh, Check& k) {
    if (check_counts(nodes, n_nodes, capacity, idx, n_idx, n_idx_scene, k) != TT_OK) return TT_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n_idx; i++)
        if (idx[i] < 0 || (uint32_t)idx[i] >= n_mesh) {
            k.why = "TLASBVH8Indices entry " + std::to_string(i) + " (" + std::to_string(idx[i]) + ") out of range";
            return TT_ERR_INVALID_ARG;
        }
    return walk_tlas(nodes, n_nodes, n_idx, k) ? TT_OK : TT_ERR_INVALID_ARG;
}

// A scene's own TLAS capacity: the leading nodes that no validated BLAS walk reaches, at most `limit` (the
// assembled scene's tlas_region, or the node count).
inline uint32_t region_capacity(const std::vector<uint8_t>& is_blas_node, uint32_t limit) {
    uint32_t n = 0;
    while (n < limit && n < is_blas_node.size() && !is_blas_node[n]) n++;
    return n;
}

// The nodes of mirror[0, capacity) up to the last one that is not all zero: what an installation has to clear
// behind a shorter TLAS (a refit rewrites reachable nodes only, so a zero node of the mirror is zero on the device).
inline uint32_t used_nodes(const tt_cwbvh_node* mirror, uint32_t capacity) {
    static const tt_cwbvh_node zero{};
    uint32_t n = capacity;
    while (n > 0 && std::memcmp(mirror + (n - 1), &zero, sizeof(zero)) == 0) n--;
    return n;
}

// The one install launch. The staged source is [nodes: n_nodes x 80 B][indices: n_idx x 4 B]; the kernel moves
// nodes in 16-B units (5 per node), clears nodes [n_nodes, n_nodes + n_clear), and handles one index (and its
// LeafMesh) per thread.
struct Plan {
    uint32_t n_nodes = 0, n_clear = 0, n_idx = 0;
    uint32_t copy_units = 0, units = 0;  // 16-B units copied; copied + cleared
    uint32_t threads = 0, blocks = 0;
    size_t idx_offset = 0, stage_bytes = 0;
};
constexpr uint32_t kInstallBlock = 256;
inline Plan plan_install(uint32_t n_nodes, uint32_t prev_nodes, uint32_t n_idx) {
    Plan p;
    p.n_nodes = n_nodes;
    p.n_clear = prev_nodes > n_nodes ? prev_nodes - n_nodes : 0u;
    p.n_idx = n_idx;
    p.copy_units = 5u * n_nodes;
    p.units = 5u * (n_nodes + p.n_clear);
    p.threads = p.units > n_idx ? p.units : n_idx;
    p.blocks = (p.threads + kInstallBlock - 1u) / kInstallBlock;
    p.idx_offset = (size_t)n_nodes * sizeof(tt_cwbvh_node);
    p.stage_bytes = p.idx_offset + (size_t)n_idx * sizeof(int32_t);
    return p;
}
inline void fill_stage(const Plan& p, const tt_cwbvh_node* nodes, const int32_t* idx, void* stage) {
    std::memcpy(stage, nodes, p.idx_offset);
    std::memcpy(static_cast<uint8_t*>(stage) + p.idx_offset, idx, (size_t)p.n_idx * sizeof(int32_t));
}

// The host mirror after the installation. A scene of its own: mirror[0, n) = nodes, [n, n + n_clear) zero, the
// rest (the BLASes) untouched. A frame slot's mirror holds its TLAS nodes alone and takes the new count.
// is_tlas_node / tlas_nodes follow the walk.
inline void apply_mirror(const Plan& p, const tt_cwbvh_node* nodes, const int32_t* idx, const Check& k, bool slot,
                         std::vector<tt_cwbvh_node>& mirror, std::vector<int32_t>& tlas, std::vector<uint8_t>& is_tlas_node,
                         std::vector<uint32_t>& tlas_nodes) {
    if (slot) {
        mirror.assign(nodes, nodes + p.n_nodes);
        is_tlas_node.assign(p.n_nodes, 0u);
    } else {
        std::memcpy(mirror.data(), nodes, (size_t)p.n_nodes * sizeof(tt_cwbvh_node));
        if (p.n_clear) std::memset(mirror.data() + p.n_nodes, 0, (size_t)p.n_clear * sizeof(tt_cwbvh_node));
        for (uint32_t n : tlas_nodes)
            if (n < is_tlas_node.size()) is_tlas_node[n] = 0u;
    }
    tlas.assign(idx, idx + p.n_idx);
    tlas_nodes = k.visit;
    for (uint32_t n : tlas_nodes) is_tlas_node[n] = 1u;
}

}  // namespace tt_tlas
