// tt_refit.h — refit plans (host) and device state shared by tt_refit.hip and tt_scene_api.hip: the TLAS
// refit (AssetManager.RefitTLAS) and the BLAS refit of deforming / skinned meshes
// (ParentObject.RefitMesh), which share NodeInitializer / layer refit / NodeUpdate / NodeCompress.
#ifndef TT_REFIT_H
#define TT_REFIT_H
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "tt_device.h"

// DocumentNodes (AssetManager.cs:1257-1297, ParentObject.cs:638-677 — the same walk) and the
// ForwardStack / LayerStack construction (AssetManager.cs:1364-1390, ParentObject.cs:706-730),
// from a node array whose root is node 0 and whose child indices are local to it (the TLAS
// region, or one BLAS). Returned as flat arrays.
struct RefitPlan {
    bool ok = true;          // false: a child index points outside [0, n_nodes) or the tree is too deep
    uint32_t n_tlas = 0;     // node count bound (TLAS nodes, or the BLAS's nodes)
    int32_t leaf_end = 0;    // largest leaf range end (primitive boxes the refit reads)
    std::vector<int32_t> pair_bvh, pair_slot, leaf, depth, parent, to_bvh, fwd;
    std::vector<std::vector<int32_t>> layers;  // NodePair indices per depth
};

// Device state of a prepared refit (one launch per refit: tt_refit.hip refit_tree).
struct RefitDev {
    int32_t *starts = nullptr, *fwd = nullptr, *parent = nullptr, *node_of = nullptr;
    uint32_t* arrive = nullptr;
    float* bb = nullptr;
    uint32_t n_pairs = 0, n_nodes = 0, n_starts = 0;
};

bool tt_refit_build_plan(const tt_cwbvh_node* nodes, uint32_t n_tlas_nodes, RefitPlan& R);
hipError_t tt_refit_prepare(const RefitPlan& R, const tt_cwbvh_node* host_nodes, uint32_t n_tlas_nodes, RefitDev& d);
// box_index: TLASCWBVHIndices for the TLAS (RefitBVHLayer), nullptr for a BLAS (RefitLayer reads
// the triangle boxes in leaf order directly)
hipError_t tt_refit_run(RefitDev& d, const float* boxes, const int32_t* box_index, tt_cwbvh_node* nodes, hipStream_t st);

// Construct (BVHRefitter.compute:72-120): one thread per triangle of the deformed mesh; writes the
// triangle's AABB (leaf order) and its positions / edges / packed normals into AggTris and the
// derived 48-B traversal layout.
struct BlasConstructArgs {
    const float* vertices;        // vertex_stride floats per vertex: position at +0, normal at +3
    const int32_t* indices;       // 3 per triangle (Unity order; the triangle is (i0, i2, i1))
    const int32_t* leaf_of;       // CWBVHIndicesBufferInverted: source triangle -> leaf-order index
    uint32_t n_tris, n_vertices, vertex_stride;
    float m[16];                  // Transform, column-major
    float* boxes;                 // n_tris x {BBMax, BBMin}
    tt_cuda_triangle* tris88;     // AggTris + TriOffset
    TriPos* tripos;               // traversal layout + TriOffset
};
hipError_t tt_blas_construct(const BlasConstructArgs& a, hipStream_t st);
void tt_refit_free(RefitDev& d);

// tt_blas_refit_many: Construct over all parts of all items in one launch, then one refit launch over the
// composed forest of the items' plans. The three descriptor arrays are rewritten every call (pointers and
// matrices are the frame's) and read by the kernels from one device buffer.
struct RefitManyPart {        // one renderer: block-uniform in blas_construct_many
    const float* vertices;
    const int32_t* indices;
    const int32_t* leaf_of;   // the item's leaf_of_triangle + first_tri
    float* boxes;             // the item's boxes in the pool
    tt_cuda_triangle* tris88; // AggTris + the item's TriOffset
    TriPos* tripos;           // traversal layout + the item's TriOffset
    uint32_t n_tris, n_vertices, vertex_stride;
    uint32_t leaf_bound;      // the item's triangle count
    float m[16];
};
struct RefitManyBlock {       // block b of the Construct launch: triangles [first, first + 256) of part `part`
    uint32_t part, first;
};
struct RefitManyItem {        // what the thread completing the item's root needs
    float l2w[16];
    uint32_t mesh_index, has_l2w, pad[2];
};
static_assert(sizeof(RefitManyPart) == 128 && sizeof(RefitManyItem) == 80 && sizeof(RefitManyBlock) == 8, "descriptor layout");
struct RefitForestItem {
    const RefitPlan* plan;
    uint32_t node_base;  // the BLAS's first node in the scene's node array
    uint32_t n_nodes;    // nodes the plan covers
    uint32_t box_base;   // the item's first box in the pool (in boxes)
};
hipError_t tt_refit_prepare_forest(const std::vector<RefitForestItem>& items, RefitDev& d);
// items: the device array, one per tree; or null and `one` (host): a forest of one tree, its item in the kernel arguments
hipError_t tt_refit_run_forest(RefitDev& d, const float* boxes, tt_cwbvh_node* nodes, const RefitManyItem* items,
                               const RefitManyItem* one, float* bounds_out, float* mesh_aabbs, hipStream_t st);
hipError_t tt_blas_construct_many(const RefitManyPart* parts, const RefitManyBlock* blocks, uint32_t n_blocks, hipStream_t st);

#endif  // TT_REFIT_H
