// tt_assemble_host.h — the host-only half of the GPU-resident objects (tt_object_*, tt_scene_layout_*):
// the BLAS-level walk that validates one object against its own counts, and AccumulateData's running
// sums. Plain C++ with no HIP in it, so a stand-alone program can run it under the host sanitizers
// (tests/native/assemble_kat_main.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/truetrace_hip.h"

namespace tt_asm {

// What the walk of one object establishes, kept with the object for the scene-level checks of
// tt_scene_assemble_objects (which never walks a BLAS again).
struct ObjectWalk {
    std::vector<uint8_t> reach;  // per node: reached from the root (so valid as a mesh record's root too)
    uint32_t max_matdat = 0;     // largest MatDat of a reachable triangle
    uint64_t leaf_tris = 0;      // triangles the reached leaves name (a built BLAS names each of its n once)
    std::string why;
};

// Validator::walk at BLAS level with NodeOffset = TriOffset = 0 (IntersectBVH's index arithmetic,
// IntersectionKernels.compute:157-213), bounded by the object's own counts: stricter than the whole-scene
// check, where a BLAS may reach into its neighbours. tris == nullptr (the triangles exist on the device only,
// tt_object_build_device): every index is checked as before, max_matdat is left at 0 for the caller to supply.
inline bool walk_object(const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris, uint32_t n_tris,
                        uint32_t root, ObjectWalk& w) {
    w.reach.assign(n_nodes, 0u);
    w.max_matdat = 0;
    w.leaf_tris = 0;
    if (root >= n_nodes) {
        w.why = "root " + std::to_string(root) + " outside the object's " + std::to_string(n_nodes) + " nodes";
        return false;
    }
    std::vector<uint32_t> work{root};
    while (!work.empty()) {
        const uint32_t ni = work.back();
        work.pop_back();
        if (w.reach[ni]) continue;
        w.reach[ni] = 1u;
        const tt_cwbvh_node& n = nodes[ni];
        const uint32_t imask = n.e_imask >> 24;
        for (int k = 0; k < 8; k++) {
            const uint32_t meta = (n.meta[k >> 2] >> ((k & 3) * 8)) & 0xffu;
            const uint32_t low5 = meta & 0x1fu, bits = (meta >> 5) & 7u;
            if ((meta & 0x18u) == 0x18u) {
                if (bits != 1u) {
                    w.why = "inner meta with child bits != 1 (node " + std::to_string(ni) + ")";
                    return false;
                }
                const uint32_t slot = low5 - 24u;
                const uint64_t child = (uint64_t)n.base_child + (uint32_t)__builtin_popcount(imask & ((1u << slot) - 1u));
                if (child >= n_nodes) {
                    w.why = "child index " + std::to_string(child) + " of node " + std::to_string(ni) +
                            " outside the object's " + std::to_string(n_nodes) + " nodes";
                    return false;
                }
                work.push_back((uint32_t)child);
            } else if (bits) {
                const uint32_t top = low5 + (31u - (uint32_t)__builtin_clz(bits));
                if (top >= 24u) {
                    w.why = "leaf meta spills into the internal-child bits (node " + std::to_string(ni) + ")";
                    return false;
                }
                for (uint32_t b = 0; b < 3; b++) {
                    if (!((bits >> b) & 1u)) continue;
                    const uint64_t t = (uint64_t)n.base_tri + low5 + b;
                    if (t >= n_tris) {
                        w.why = "triangle index " + std::to_string(t) + " of node " + std::to_string(ni) +
                                " outside the object's " + std::to_string(n_tris) + " triangles";
                        return false;
                    }
                    w.leaf_tris++;
                    if (tris && tris[t].MatDat > w.max_matdat) w.max_matdat = tris[t].MatDat;
                }
            }
        }
    }
    return true;
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
