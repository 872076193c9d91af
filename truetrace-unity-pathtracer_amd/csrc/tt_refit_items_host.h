// tt_refit_items_host.h — the host-only half of tt_blas_refit_many (tt_scene_api.hip): the checks of an item list
// against the scene's _MeshData records that need neither node data nor a device. Plain C++ with no HIP in it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/truetrace_hip.h"

namespace tt_refit_items {

// why receives the first violation, in list order (item by item, part by part); the pairwise checks of an item
// against the earlier ones come with that item.
inline tt_status check(const tt_blas_refit_item* items, uint32_t n_items, const tt_mesh_data* md, uint32_t n_mesh,
                       uint32_t n_scene_tris, uint32_t flags, std::string& why) {
    if (!items || n_items == 0) {
        why = "no items";
        return TT_ERR_INVALID_ARG;
    }
    if (!md || n_mesh == 0) {
        why = "no _MeshData records";
        return TT_ERR_INVALID_ARG;
    }
    const bool host_arrays = !(flags & TT_TRACE_DEVICE_PTRS);
    auto item_why = [&](uint32_t i, const std::string& reason) {
        why = "item " + std::to_string(i) + ": " + reason;
        return TT_ERR_INVALID_ARG;
    };
    std::vector<std::pair<uint32_t, uint32_t>> seen_mesh, seen_node;  // (value, item), kept sorted
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_items; i++) {
        const tt_blas_refit_item& it = items[i];
        if (!it.leaf_of_triangle || !it.parts) return item_why(i, "null leaf_of_triangle or parts");
        if (it.n_tris == 0 || it.n_parts == 0) return item_why(i, "no triangles or no parts");
        if (it.mesh_index >= n_mesh)
            return item_why(i, "mesh_index " + std::to_string(it.mesh_index) + " out of range (" + std::to_string(n_mesh) + " records)");
        const tt_mesh_data& r = md[it.mesh_index];
        const auto sm = std::lower_bound(seen_mesh.begin(), seen_mesh.end(), std::make_pair(it.mesh_index, 0u));
        if (sm != seen_mesh.end() && sm->first == it.mesh_index)
            return item_why(i, "mesh_index " + std::to_string(it.mesh_index) + " was given by item " + std::to_string(sm->second) + " too");
        if (r.NodeOffset < 0 || r.TriOffset < 0) return item_why(i, "negative mesh offsets");
        const auto sn = std::lower_bound(seen_node.begin(), seen_node.end(), std::make_pair((uint32_t)r.NodeOffset, 0u));
        if (sn != seen_node.end() && sn->first == (uint32_t)r.NodeOffset)
            return item_why(i, "its record shares NodeOffset " + std::to_string(r.NodeOffset) + " with item " +
                                   std::to_string(sn->second) + "'s: one BLAS, refit it once");
        if ((uint32_t)(r.mesh_data_bvh_offsets & 0x7fffffff) != (uint32_t)r.NodeOffset) {
            why = "item " + std::to_string(i) + ": the mesh's BLAS root is not its first node";
            return TT_ERR_UNSUPPORTED;
        }
        if ((uint64_t)r.TriOffset + it.n_tris > n_scene_tris) return item_why(i, "TriOffset + n_tris exceeds the scene's triangles");
        total += it.n_tris;
        if (total > TT_BLAS_REFIT_MANY_MAX_TRIS)
            return item_why(i, "more than " + std::to_string(TT_BLAS_REFIT_MANY_MAX_TRIS) + " triangles in all");
        ranges.clear();
        for (uint32_t k = 0; k < it.n_parts; k++) {
            const tt_blas_refit_part& p = it.parts[k];
            auto pk = [&] { return "part " + std::to_string(k) + ": "; };  // (built only for a refusal)
            if (!p.vertices || !p.indices) return item_why(i, pk() + "null vertices or indices");
            if (p.n_tris == 0 || p.n_vertices == 0) return item_why(i, pk() + "no triangles or no vertices");
            if (p.vertex_stride < 6) return item_why(i, pk() + "vertex_stride < 6");
            if ((uint64_t)p.first_tri + p.n_tris > it.n_tris)
                return item_why(i, pk() + "triangles [" + std::to_string(p.first_tri) + ", " +
                                       std::to_string((uint64_t)p.first_tri + p.n_tris) + ") leave the mesh's " + std::to_string(it.n_tris));
            ranges.emplace_back(p.first_tri, k);
        }
        std::sort(ranges.begin(), ranges.end());
        uint64_t next = 0;
        for (const auto& rg : ranges) {
            const tt_blas_refit_part& p = it.parts[rg.second];
            if (p.first_tri < next) return item_why(i, "part " + std::to_string(rg.second) + " overlaps another part at triangle " + std::to_string(p.first_tri));
            if (p.first_tri > next)
                return item_why(i, "the parts leave a gap: triangles [" + std::to_string(next) + ", " + std::to_string(p.first_tri) + ")");
            next = (uint64_t)p.first_tri + p.n_tris;
        }
        if (next != it.n_tris)
            return item_why(i, "the parts leave a gap: triangles [" + std::to_string(next) + ", " + std::to_string(it.n_tris) + ")");
        if (host_arrays) {
            for (uint32_t k = 0; k < it.n_parts; k++) {
                const tt_blas_refit_part& p = it.parts[k];
                for (uint64_t j = 0; j < 3ull * p.n_tris; j++)
                    if (p.indices[j] < 0 || (uint32_t)p.indices[j] >= p.n_vertices)
                        return item_why(i, "part " + std::to_string(k) + ": index " + std::to_string(p.indices[j]) + " out of range");
            }
            for (uint32_t t = 0; t < it.n_tris; t++)
                if (it.leaf_of_triangle[t] < 0 || (uint32_t)it.leaf_of_triangle[t] >= it.n_tris)
                    return item_why(i, "leaf_of_triangle[" + std::to_string(t) + "] out of range");
        }
        seen_mesh.insert(sm, std::make_pair(it.mesh_index, i));  // (both stay sorted by value)
        seen_node.insert(std::lower_bound(seen_node.begin(), seen_node.end(), std::make_pair((uint32_t)r.NodeOffset, 0u)),
                         std::make_pair((uint32_t)r.NodeOffset, i));
    }
    return TT_OK;
}

}  // namespace tt_refit_items
