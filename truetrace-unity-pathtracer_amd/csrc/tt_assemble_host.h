// tt_assemble_host.h — the host-only half of the GPU-resident objects (tt_object_*, tt_scene_layout_*):
// the BLAS-level walk that validates one object against its own counts (the shared loop of
// tt_scene_check_host.h, with the object's bounds and messages), and AccumulateData's running sums. Plain C++ with no HIP in it, so a stand-alone program can run it under the host sanitizers
// (tests/native/assemble_kat_main.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/truetrace_hip.h"
#include "tt_scene_check_host.h"

namespace tt_asm {

// What the walk of one object establishes, kept with the object for the scene-level checks of
// tt_scene_assemble_objects (which never walks a BLAS again).
struct ObjectWalk {
    std::vector<uint8_t> reach;  // per node: reached from the root (so valid as a mesh record's root too)
    uint32_t max_matdat = 0;     // largest MatDat of a reachable triangle
    uint64_t leaf_tris = 0;      // triangles the reached leaves name (a built BLAS names each of its n once)
    std::string why;
};

// The shared walk (tt_scene_check_host.h) at BLAS level with NodeOffset = TriOffset = 0 (IntersectBVH's index
// arithmetic, IntersectionKernels.compute:157-213), bounded by the object's own counts: stricter than the whole-scene
// check, where a BLAS may reach into its neighbours. tris == nullptr (the triangles exist on the device only,
// tt_object_build_device): every index is checked as before, max_matdat is left at 0 for the caller to supply.
struct ObjectLevel {
    const uint32_t n_nodes;
    const tt_cwbvh_node* nodes;
    const tt_cuda_triangle* tris;
    const uint32_t n_tris;
    ObjectWalk& w;
    static std::string of_node(uint32_t ni) { return " of node " + std::to_string(ni); }
    TT_CHECK_INLINE tt_check::Enter enter(uint32_t ni) {  // (in range: the root and every child were checked before they were pushed)
        if (w.reach[ni]) return tt_check::Enter::seen;
        w.reach[ni] = 1u;
        return tt_check::Enter::fresh;
    }
    const tt_cwbvh_node& node(uint32_t ni) const { return nodes[ni]; }
    TT_CHECK_INLINE bool child(uint32_t ni, const tt_cwbvh_node& n, uint32_t rank, uint32_t& out) {
        const uint64_t child = (uint64_t)n.base_child + rank;
        out = (uint32_t)child;
        if (child < n_nodes) return true;
        w.why = "child index " + std::to_string(child) + of_node(ni) + " outside the object's " + std::to_string(n_nodes) + " nodes";
        return false;
    }
    TT_CHECK_INLINE bool leaf(uint32_t ni, uint64_t t) {
        if (t >= n_tris) {
            w.why = "triangle index " + std::to_string(t) + of_node(ni) + " outside the object's " + std::to_string(n_tris) +
                    " triangles";
            return false;
        }
        w.leaf_tris++;
        if (tris && tris[t].MatDat > w.max_matdat) w.max_matdat = tris[t].MatDat;
        return true;
    }
    bool bad_meta(uint32_t ni, const char* what) {
        w.why = std::string(what) + " (node " + std::to_string(ni) + ")";
        return false;
    }
};
inline bool walk_object(const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris, uint32_t n_tris,
                        uint32_t root, ObjectWalk& w) {
    w.reach.assign(n_nodes, 0u);
    w.max_matdat = 0;
    w.leaf_tris = 0;
    if (root >= n_nodes) {
        w.why = "root " + std::to_string(root) + " outside the object's " + std::to_string(n_nodes) + " nodes";
        return false;
    }
    ObjectLevel p{n_nodes, nodes, tris, n_tris, w};
    return tt_check::walk(root, p);
}

inline tt_status validate_object(const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris,
                                 uint32_t n_tris, uint32_t root, ObjectWalk& w) {
    if (!nodes || !n_nodes || !tris || !n_tris) {
        w.why = "null or empty buffer";
        return TT_ERR_INVALID_ARG;
    }
    return walk_object(nodes, n_nodes, tris, n_tris, root, w) ? TT_OK : TT_ERR_INVALID_ARG;
}

// AssetManager.AccumulateData's running sums (AssetManager.cs:995, :1133-1136, :1178-1181): the TLAS region
// first, then every object's nodes; triangles from 0. Totals beyond 32 bits are refused.
inline tt_status layout_counts(const uint32_t* n_nodes, const uint32_t* n_tris, uint32_t n, uint32_t tlas_region,
                               uint32_t* node_offsets, uint32_t* tri_offsets, uint32_t* n_nodes_total,
                               uint32_t* n_tris_total, std::string& why) {
    if (!n_nodes || !n_tris || !n) {
        why = "null or empty object list";
        return TT_ERR_INVALID_ARG;
    }
    uint64_t nn = tlas_region, nt = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (nn > 0xffffffffull || nt > 0xffffffffull) break;
        if (node_offsets) node_offsets[i] = (uint32_t)nn;
        if (tri_offsets) tri_offsets[i] = (uint32_t)nt;
        nn += n_nodes[i];
        nt += n_tris[i];
    }
    if (nn > 0xffffffffull || nt > 0xffffffffull) {
        why = "the objects' node or triangle counts sum beyond 32 bits";
        return TT_ERR_INVALID_ARG;
    }
    if (n_nodes_total) *n_nodes_total = (uint32_t)nn;
    if (n_tris_total) *n_tris_total = (uint32_t)nt;
    return TT_OK;
}

}  // namespace tt_asm
