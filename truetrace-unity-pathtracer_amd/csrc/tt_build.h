// tt_build.h — the BLAS builder's device-resident forms (tt_build.hip), for the translation units that keep a
// build on the GPU from end to end (tt_object_build.hip). The exported tt_bvh2_presort_device /
// tt_blas_build_device are wrappers that upload and download around these.
#pragma once
#include <hip/hip_runtime.h>

#include "tt_ctx.h"

// A built BLAS left on the device.
struct tt_blas_dev {
    DevBuf<tt_cwbvh_node> nodes;      // n_nodes, BLAS-local indices
    DevBuf<int32_t> cwbvh_indices;    // n: leaf position -> source triangle
    uint32_t n_nodes = 0, bvh2_depth = 0;
    float root_box[6] = {0, 0, 0, 0, 0, 0};  // {BBMax, BBMin}: the Extend union of the primitives in index order
};

// aabbs_dev: n x {BBMax[3], BBMin[3]}; presorted_dev: 3 x n. Both synchronize `st` before they return; on
// failure the reason is in tt_build_error() (thread-local). The caller has set the device.
tt_status tt_build_presort_dev(hipStream_t st, const float* aabbs_dev, uint32_t n, int32_t* presorted_dev);
tt_status tt_build_blas_dev(hipStream_t st, const float* aabbs_dev, uint32_t n, const int32_t* presorted_dev,
                            tt_blas_dev& out);
const char* tt_build_error();
