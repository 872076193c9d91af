// tt_light_refit_plan_host.h — what the light refit climbs, built on the host from validated lights
// (tt_lights_check_host.h's rules; no HIP: tt_lights.hip and host/tt_lights.cpp both build it). Per tree -- the
// TLAS, and each distinct LightNodeOffset a light mesh's _MeshData record names -- the parent of every reachable
// node, the reachable nodes in breadth-first order and the reachable leaves. Slot 1 of every tree is unreachable
// (the builder starts children at 2), and so are unused tail slots: they have no parent here, are in no list and
// keep their bytes. Also the checks of a refit call's arguments, shared by tt_lights_refit and its host reference.
#ifndef TT_LIGHT_REFIT_PLAN_HOST_H
#define TT_LIGHT_REFIT_PLAN_HOST_H
#include <map>
#include <string>
#include <vector>

#include "tt_lights_check_host.h"

namespace tt_lplan {

struct Tree {
    uint32_t base = 0;         // the tree's first node
    int32_t start_index = 0;   // mesh trees: the first LightTriangles row (LightMeshData.StartIndex)
    int32_t tri_offset = 0;    // mesh trees: TriOffset of a _MeshData record that owns the tree
    uint32_t bfs_first = 0, bfs_count = 0;    // its reachable nodes in Plan::bfs, the root first
    uint32_t leaf_first = 0, leaf_count = 0;  // its reachable leaves in Plan::leaf_node
};

struct Plan {
    std::vector<int32_t> parent;     // per node (absolute indices): its parent; -1: a root or unreachable
    std::vector<int32_t> base;       // per node: its tree's first node (0 where unreachable)
    std::vector<int32_t> bfs;        // reachable nodes, tree after tree
    std::vector<int32_t> leaf_node;  // reachable leaves, tree after tree: the node ...
    std::vector<int32_t> leaf_row;   // ... and, in a mesh tree, its LightTriangles row
    Tree tlas;
    std::map<uint32_t, Tree> trees;  // mesh trees by LightNodeOffset
    std::vector<uint8_t> reached;    // per node: some tree's walk reached it
    // Not empty: the lights pass tt_lcheck::validate, which looks at each light mesh alone, but cannot be refitted: a
    // node lies in two trees (the later walk would take over its parent and its counter would never return to
    // zero), or two light meshes name one tree with different StartIndex. A refit refuses with this text.
    std::string unusable;
};

inline void walk(const tt_light_node* nodes, Plan& P, Tree& T) {
    T.bfs_first = (uint32_t)P.bfs.size();
    T.leaf_first = (uint32_t)P.leaf_node.size();
    P.bfs.push_back((int32_t)T.base);
    P.parent[T.base] = -1;
    P.reached[T.base] = 1;
    for (size_t at = T.bfs_first; at < P.bfs.size(); at++) {
        const int32_t n = P.bfs[at];
        P.base[n] = (int32_t)T.base;
        const int32_t left = nodes[n].left;
        if (left < 0) {
            P.leaf_node.push_back(n);
            P.leaf_row.push_back(T.start_index + (-(left + 1)));
            continue;
        }
        for (int32_t k = 0; k < 2; k++) {
            const int32_t ch = (int32_t)T.base + left + k;
            if (P.reached[ch]) {  // (not walked again: the plan is unusable)
                if (P.unusable.empty())
                    P.unusable = tt_lcheck::fmt("light node %lld lies in the tree at %lld and in another tree", ch, T.base);
                continue;
            }
            P.reached[ch] = 1;
            P.parent[ch] = n;
            P.bfs.push_back(ch);
        }
    }
    T.bfs_count = (uint32_t)P.bfs.size() - T.bfs_first;
    T.leaf_count = (uint32_t)P.leaf_node.size() - T.leaf_first;
}

// L must have passed tt_lcheck::validate against md
inline void build(const tt_lcheck::Lights& L, const tt_mesh_data* md, Plan& P) {
    P = Plan();
    P.parent.assign(L.n_nodes, -1);
    P.base.assign(L.n_nodes, 0);
    P.reached.assign(L.n_nodes, 0);
    P.tlas.base = 0;
    walk(L.nodes, P, P.tlas);
    for (uint32_t m = 0; m < L.n_meshes; m++) {
        const tt_mesh_data& M = md[L.meshes[m].LockedMeshIndex];
        const uint32_t off = (uint32_t)M.LightNodeOffset;
        const auto have = P.trees.find(off);
        if (have != P.trees.end()) {
            if (have->second.start_index != L.meshes[m].StartIndex && P.unusable.empty())
                P.unusable = tt_lcheck::fmt("light mesh %lld names the tree at %lld with StartIndex %lld, another light mesh with another",
                                            m, off, L.meshes[m].StartIndex);
            continue;
        }
        if (P.reached[off]) {
            if (P.unusable.empty()) P.unusable = tt_lcheck::fmt("light mesh %lld: its tree's root %lld lies inside another tree", m, off);
            continue;
        }
        Tree T;
        T.base = off;
        T.start_index = L.meshes[m].StartIndex;
        T.tri_offset = M.TriOffset;
        walk(L.nodes, P, T);
        P.trees[off] = T;
    }
}

inline bool same_structure(const tt_light_node* a, const tt_light_node* b, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (a[i].left != b[i].left) return false;
    return true;
}

// The refusals of a refit call that need no device: an unusable plan, a listed record with no light triangles or no
// tree, two listed records with one LightNodeOffset, a transform count that is not the light-mesh count, a host-side
// SolidOffset that is not the root of a mesh tree (transforms null: not checked -- no TLAS pass, or device memory).
inline tt_status check_call(const Plan& P, const tt_mesh_data* md, uint32_t n_mesh, uint32_t n_lmeshes, uint32_t n_nodes,
                            const uint32_t* mesh_indices, uint32_t n_mesh_indices, bool tlas_pass,
                            const tt_light_transform* transforms, uint32_t n_transforms, std::string& why) {
    using tt_lcheck::fmt;
    if (!P.unusable.empty()) {
        why = "these lights cannot be refitted: " + P.unusable;
        return TT_ERR_INVALID_ARG;
    }
    if (n_mesh_indices && !mesh_indices) {
        why = "null mesh_indices";
        return TT_ERR_INVALID_ARG;
    }
    std::map<uint32_t, uint32_t> seen;  // LightNodeOffset -> position in the list
    for (uint32_t i = 0; i < n_mesh_indices; i++) {
        const uint32_t m = mesh_indices[i];
        if (m >= n_mesh) {
            why = fmt("mesh_indices[%lld] = %lld outside the %lld mesh records", i, m, n_mesh);
            return TT_ERR_INVALID_ARG;
        }
        if (md[m].LightTriCount == 0) {
            why = fmt("mesh_indices[%lld]: mesh record %lld has LightTriCount 0", i, m);
            return TT_ERR_INVALID_ARG;
        }
        const uint32_t off = (uint32_t)md[m].LightNodeOffset;
        if (!P.trees.count(off)) {
            why = fmt("mesh_indices[%lld]: no light mesh uses the LightNodeOffset %lld of mesh record %lld", i, off, m);
            return TT_ERR_INVALID_ARG;
        }
        const auto it = seen.find(off);
        if (it != seen.end()) {
            why = fmt("mesh_indices[%lld] and mesh_indices[%lld] share the light tree at LightNodeOffset %lld", it->second, i, off);
            return TT_ERR_INVALID_ARG;
        }
        seen[off] = i;
    }
    if (tlas_pass && n_transforms != n_lmeshes) {
        why = fmt("%lld transforms for %lld light meshes", n_transforms, n_lmeshes);
        return TT_ERR_INVALID_ARG;
    }
    if (tlas_pass && transforms)
        for (uint32_t i = 0; i < n_transforms; i++)
            if (transforms[i].SolidOffset < 0 || (uint32_t)transforms[i].SolidOffset >= n_nodes ||
                !P.trees.count((uint32_t)transforms[i].SolidOffset)) {
                why = fmt("transforms[%lld]: SolidOffset %lld is not the root of a mesh tree (a LightNodeOffset) of the %lld light nodes", i,
                          transforms[i].SolidOffset, n_nodes);
                return TT_ERR_INVALID_ARG;
            }
    return TT_OK;
}

}  // namespace tt_lplan
#endif
