// tt_tlas_host.h — the host-only half of a TLAS installation (tt_scene_update_tlas, tt_tlas_rebuild): the checks
// that keep a malformed TLAS from reaching a kernel, the capacity of a scene's TLAS region, the shape of the one
// install launch, and the host mirror's update. Its walk is the shared one of tt_scene_check_host.h, with this
// installation's bounds and messages. Plain C++ with no HIP in it, so a stand-alone program can run it
// under the host sanitizers (tests/native/tlas_install_kat_main.cpp).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/truetrace_hip.h"
#include "tt_scene_check_host.h"

namespace tt_tlas {

struct Check {
    std::vector<uint32_t> visit;  // the nodes the TLAS-level walk reached
    std::string why;
};

// The shared walk (tt_scene_check_host.h) from node 0 over the supplied nodes alone: IntersectBVH's index arithmetic
// at TLAS level (IntersectionKernels.compute:157-196). A child index must stay inside [0, n_nodes) -- the nodes
// behind them are zeroed by the installation, never read from the caller -- and a leaf slot inside [0, n_idx).
struct TlasWalk {
    const tt_cwbvh_node* nodes;
    const uint32_t n_nodes, n_idx;
    Check& k;
    std::vector<uint8_t> seen = std::vector<uint8_t>(n_nodes, 0u);
    bool refuse(const std::string& what) {
        k.why = what;
        return false;
    }
    TT_CHECK_INLINE bool node_in_range(uint64_t ni) {
        return ni < n_nodes ||
               refuse("node index " + std::to_string(ni) + " out of range of the " + std::to_string(n_nodes) + " TLAS nodes");
    }
    TT_CHECK_INLINE tt_check::Enter enter(uint32_t ni) {
        if (!node_in_range(ni)) return tt_check::Enter::refused;
        if (seen[ni]) return tt_check::Enter::seen;
        seen[ni] = 1u;
        k.visit.push_back(ni);
        return tt_check::Enter::fresh;
    }
    const tt_cwbvh_node& node(uint32_t ni) const { return nodes[ni]; }
    TT_CHECK_INLINE bool child(uint32_t, const tt_cwbvh_node& n, uint32_t rank, uint32_t& out) {
        const uint64_t child = (uint64_t)n.base_child + rank;
        out = (uint32_t)child;
        return node_in_range(child);
    }
    TT_CHECK_INLINE bool leaf(uint32_t, uint64_t t) { return t < n_idx || refuse("TLAS leaf slot out of range"); }
    bool bad_meta(uint32_t, const char* what) { return refuse(what); }
};
inline bool walk_tlas(const tt_cwbvh_node* nodes, uint32_t n_nodes, uint32_t n_idx, Check& k) {
    k.visit.clear();
    TlasWalk p{nodes, n_nodes, n_idx, k};
    return tt_check::walk(0u, p);
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
    } else {
        std::memcpy(mirror.data(), nodes, (size_t)p.n_nodes * sizeof(tt_cwbvh_node));
        if (p.n_clear) std::memset(mirror.data() + p.n_nodes, 0, (size_t)p.n_clear * sizeof(tt_cwbvh_node));
    }
    tlas.assign(idx, idx + p.n_idx);
    tt_check::replace_tlas_reach(is_tlas_node, tlas_nodes, k.visit, slot ? p.n_nodes : 0u);
}

}  // namespace tt_tlas
