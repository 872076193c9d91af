// tt_light_refit.h — the two launches of tt_lights_refit (tt_light_refit.hip), as tt_lights.hip calls them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/truetrace_hip.h"

// One 256-thread block of the mesh-forest launch: leaves [first, first + count) of the plan's leaf list (one
// tree's: no block straddles two trees) and the TriOffset of the listed record that owns the tree.
struct LightRefitBlock {
    uint32_t first, count;
    int32_t tri_offset;
    uint32_t pad;
};

// The plan on the device (tt_light_refit_plan_host.h), shared by both launches.
struct LightRefitPlanDev {
    const int2* up;            // per node: {parent (-1: a root), its tree's first node}
    uint32_t* arrive;          // per node: arrivals at an interior node (0 between refits)
    const int32_t* leaf_node;  // the plan's leaf list: the node ...
    const int32_t* leaf_row;   // ... and its LightTriangles row (mesh trees)
    tt_light_node* nodes;
    uint32_t n_nodes;
};

hipError_t tt_light_refit_forest(const LightRefitPlanDev& p, const LightRefitBlock* blocks, uint32_t n_blocks,
                                 tt_light_tri* ltris, const tt_cuda_triangle* tris, uint32_t n_tris, bool conservative,
                                 hipStream_t st);
hipError_t tt_light_refit_tlas(const LightRefitPlanDev& p, uint32_t leaf_first, uint32_t n_leaves,
                               const tt_light_transform* transforms, uint32_t n_transforms, bool conservative,
                               hipStream_t st);
