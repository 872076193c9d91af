// tt_lights_check_host.h — what SampleLightBVH (CommonData.cginc:1126-1166) and its caller (:1913-1920) may
// reach, checked on the host (no HIP: tt_lights_validate, tt_emit_nee_host and tests/native/lights_kat_main.cpp
// build it with a host compiler). The kernel indexes LightNodes, LightTriangles, _LightMeshes, _MeshData and
// AggTris with no bounds checks of its own; this walk is why it may.
//
// Termination: every interior `left` must exceed its node's own index (relative to the tree's first node), so
// a descent visits strictly increasing indices and cannot cycle; its length is then bounded by the depth this
// walk measures, which must fit TT_LIGHT_MAX_REPS.
#ifndef TT_LIGHTS_CHECK_HOST_H
#define TT_LIGHTS_CHECK_HOST_H
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/truetrace_hip.h"

namespace tt_lcheck {

struct Lights {
    const tt_light_node* nodes;
    uint32_t n_nodes;
    const tt_light_tri* tris;
    uint32_t n_tris;
    const tt_light_mesh* meshes;
    uint32_t n_meshes;
};

inline std::string fmt(const char* f, long long a = 0, long long b = 0, long long c = 0) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), f, a, b, c);
    return buf;
}

// Walks the tree whose first node is `base` and whose nodes lie in [base, end). leaf(k, node) checks a leaf
// holding k. depth: the largest number of interior nodes on a root-to-leaf path.
template <class Leaf>
bool walk_tree(const Lights& L, uint32_t base, uint32_t end, const char* what, Leaf&& leaf, uint32_t& depth,
               std::string& why) {
    std::vector<std::pair<uint32_t, uint32_t>> stack;  // (node relative to base, interior nodes above it)
    stack.push_back({0u, 0u});
    depth = 0;
    uint64_t visits = 0;
    while (!stack.empty()) {
        const uint32_t rel = stack.back().first, d = stack.back().second;
        stack.pop_back();
        if (++visits > (uint64_t)end - base) {  // a tree visits each of its nodes once
            why = std::string(what) + fmt(" at node %lld: a node has two parents", base);
            return false;
        }
        const tt_light_node& nd = L.nodes[base + rel];
        if (nd.left < 0) {
            depth = std::max(depth, d);
            if (!leaf((uint32_t)(-(nd.left + 1)), base + rel, why)) return false;
            continue;
        }
        const uint32_t left = (uint32_t)nd.left;
        if (left & 1u) {
            why = std::string(what) + fmt(" node %lld: left %lld is odd", base + rel, left);
            return false;
        }
        if (left <= rel) {
            why = std::string(what) + fmt(" node %lld: left %lld is not greater than the node's own index %lld", base + rel, left, rel);
            return false;
        }
        if ((uint64_t)base + left + 1u >= end) {
            why = std::string(what) + fmt(" node %lld: children %lld, %lld outside the tree's nodes", base + rel,
                                          (long long)base + left, (long long)base + left + 1);
            return false;
        }
        if (d + 1u > TT_LIGHT_MAX_REPS) {
            why = std::string(what) + fmt(" node %lld: deeper than %lld steps", base + rel, TT_LIGHT_MAX_REPS);
            return false;
        }
        stack.push_back({left, d + 1u});
        stack.push_back({left + 1u, d + 1u});
    }
    return true;
}

// first triangle index past mesh `m`'s triangles: the next larger TriOffset, or the scene's count
inline uint32_t mesh_tri_end(const tt_mesh_data* md, uint32_t n_mesh, uint32_t m, uint32_t n_scene_tris) {
    uint32_t end = n_scene_tris;
    for (uint32_t k = 0; k < n_mesh; k++)
        if (md[k].TriOffset > md[m].TriOffset && (uint32_t)md[k].TriOffset < end) end = (uint32_t)md[k].TriOffset;
    return end;
}

inline tt_status validate(const Lights& L, const tt_mesh_data* md, uint32_t n_mesh, uint32_t n_scene_tris,
                          std::string& why) {
    if (!L.nodes || !L.tris || !L.meshes || !md || !L.n_tris || !L.n_meshes || !n_mesh) {
        why = "null or empty light buffer";
        return TT_ERR_INVALID_ARG;
    }
    if (L.n_meshes > 0x3fffffffu || L.n_nodes > 0x7fffffffu || L.n_tris > 0x7fffffffu) {
        why = "light buffer too large";
        return TT_ERR_INVALID_ARG;
    }
    const uint32_t tlas_end = 2u * L.n_meshes;
    if (L.n_nodes < tlas_end) {
        why = fmt("%lld light nodes cannot hold the TLAS part of %lld light meshes", L.n_nodes, L.n_meshes);
        return TT_ERR_INVALID_ARG;
    }
    uint32_t tlas_depth = 0;
    auto tlas_leaf = [&](uint32_t k, uint32_t node, std::string& w) {
        if (k >= L.n_meshes) {
            w = fmt("TLAS node %lld: light mesh %lld >= %lld", node, k, L.n_meshes);
            return false;
        }
        return true;
    };
    if (!walk_tree(L, 0u, tlas_end, "TLAS", tlas_leaf, tlas_depth, why)) return TT_ERR_INVALID_ARG;
    uint32_t mesh_depth = 0;
    for (uint32_t m = 0; m < L.n_meshes; m++) {
        const tt_light_mesh& lm = L.meshes[m];
        if (lm.LockedMeshIndex < 0 || (uint32_t)lm.LockedMeshIndex >= n_mesh) {
            why = fmt("light mesh %lld: LockedMeshIndex %lld outside the %lld mesh records", m, lm.LockedMeshIndex, n_mesh);
            return TT_ERR_INVALID_ARG;
        }
        const tt_mesh_data& M = md[lm.LockedMeshIndex];
        const int64_t off = M.LightNodeOffset;
        if (off < (int64_t)tlas_end || (off & 1) || off >= (int64_t)L.n_nodes) {
            why = fmt("light mesh %lld: LightNodeOffset %lld of mesh record %lld is odd, below the TLAS part or past the nodes",
                      m, off, lm.LockedMeshIndex);
            return TT_ERR_INVALID_ARG;
        }
        if (lm.StartIndex < 0 || lm.IndexEnd <= lm.StartIndex || (uint32_t)lm.IndexEnd > L.n_tris) {
            why = fmt("light mesh %lld: [StartIndex %lld, IndexEnd %lld) outside the light triangles", m, lm.StartIndex, lm.IndexEnd);
            return TT_ERR_INVALID_ARG;
        }
        if (M.TriOffset < 0 || (uint32_t)M.TriOffset >= n_scene_tris) {
            why = fmt("light mesh %lld: TriOffset %lld of mesh record %lld outside the triangles", m, M.TriOffset, lm.LockedMeshIndex);
            return TT_ERR_INVALID_ARG;
        }
        const uint32_t tri_end = mesh_tri_end(md, n_mesh, (uint32_t)lm.LockedMeshIndex, n_scene_tris);
        auto mesh_leaf = [&](uint32_t k, uint32_t node, std::string& w) {
            const uint64_t t = (uint64_t)lm.StartIndex + k;
            if (t >= (uint64_t)lm.IndexEnd) {
                w = fmt("light mesh %lld, node %lld: light triangle %lld outside [StartIndex, IndexEnd)", m, node, (long long)t);
                return false;
            }
            if ((uint64_t)L.tris[t].TriTarget + (uint64_t)M.TriOffset >= tri_end) {
                w = fmt("light triangle %lld: TriTarget %lld outside the triangles of mesh record %lld", (long long)t,
                        L.tris[t].TriTarget, lm.LockedMeshIndex);
                return false;
            }
            return true;
        };
        uint32_t d = 0;
        if (!walk_tree(L, (uint32_t)off, L.n_nodes, "mesh-tree", mesh_leaf, d, why)) return TT_ERR_INVALID_ARG;
        mesh_depth = std::max(mesh_depth, d);
    }
    // interior steps of both levels, the TLAS -> mesh transition and the returning step
    if ((uint64_t)tlas_depth + mesh_depth + 2u > TT_LIGHT_MAX_REPS) {
        why = fmt("a descent of %lld TLAS and %lld mesh-tree steps exceeds the %lld-step bound", tlas_depth, mesh_depth,
                  TT_LIGHT_MAX_REPS);
        return TT_ERR_INVALID_ARG;
    }
    return TT_OK;
}

}  // namespace tt_lcheck
#endif
