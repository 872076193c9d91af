// tt_build.h — the BLAS builder's device-resident forms (tt_build.hip), for the translation units that keep a
// build on the GPU from end to end (tt_object_build.hip). The exported tt_bvh2_presort_device /
// tt_blas_build_device are wrappers that upload and download around these.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "tt_ctx.h"

// A built BLAS left on the device.
struct tt_blas_dev {
    DevBuf<tt_cwbvh_node> nodes;      // n_nodes, BLAS-local indices
    DevBuf<int32_t> cwbvh_indices;    // n: leaf position -> source triangle
    uint32_t n_nodes = 0, bvh2_depth = 0;
    float root_box[6] = {0, 0, 0, 0, 0, 0};  // {BBMax, BBMin}: the Extend union of the primitives in index order
};

// M BLASes built together over one concatenated primitive range (mesh m owns [start[m], start[m + 1])), left on
// the device. Every level of every stage runs all meshes at once, so the host waits once per level of the deepest
// mesh, not once per level of every mesh.
struct tt_forest_dev {
    DevBuf<tt_cwbvh_node> nodes;        // node_base[M]: mesh m's at [node_base[m], node_base[m + 1]), BLAS-local indices
    DevBuf<int32_t> cwbvh_indices;      // start[M]: global leaf position -> global primitive (mesh m's: minus start[m])
    std::vector<uint32_t> node_base;    // M + 1
    std::vector<uint32_t> bvh2_depth;   // M: the levels at which the mesh still had a live segment
    std::vector<float> root_box;        // 6 per mesh, as tt_blas_dev::root_box
};

// aabbs_dev: n x {BBMax[3], BBMin[3]}; presorted_dev: 3 x n. Both synchronize `st` before they return; on
// failure the reason is in tt_build_error() (thread-local). The caller has set the device.
tt_status tt_build_presort_dev(hipStream_t st, const float* aabbs_dev, uint32_t n, int32_t* presorted_dev);
tt_status tt_build_blas_dev(hipStream_t st, const float* aabbs_dev, uint32_t n, const int32_t* presorted_dev,
                            tt_blas_dev& out);
// The forest forms (the two above are their M = 1 case). start: a HOST array of n_meshes + 1 offsets, n = start[M].
// presorted_dev is axis-major over n (axis d at d * n) and holds GLOBAL primitive indices. sorted (host, nullable:
// every mesh): the meshes the presort sorts; the others' lists are already in presorted_dev. Unlike the single
// presort, meshes of at most 16 primitives are sorted too. mesh_status (host, nullable, n_meshes, preset by the
// caller) receives the failing status of every mesh the failing stage flagged; the message names the lowest.
tt_status tt_build_presort_forest(hipStream_t st, const float* aabbs_dev, const uint32_t* start, uint32_t n_meshes,
                                  const unsigned char* sorted, int32_t* presorted_dev, tt_status* mesh_status);
tt_status tt_build_blas_forest(hipStream_t st, const float* aabbs_dev, const uint32_t* start, uint32_t n_meshes,
                               const int32_t* presorted_dev, tt_forest_dev& out, tt_status* mesh_status);
const char* tt_build_error();
