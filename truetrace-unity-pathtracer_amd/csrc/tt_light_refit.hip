// tt_light_refit.hip — the per-frame refit of the light BVH on the GPU: LightBVHRefitter.compute's
// LightRefitKernel (:183-209) behind BVHRefitter.compute's TransferKernel (:135-147) for the light trees of
// deforming meshes (ParentObject.RefitMesh, ParentObject.cs:881-905), and RefitKernel (:136-157) for the light
// TLAS (AssetManager.RefitTLAS, AssetManager.cs:1585-1605). The arithmetic is tt_light_refit_core.h, the text the
// host reference builds too.
//
// MI355X shape: tt_refit.hip's problem again -- a few thousand 40-byte records per frame, latency- not
// bandwidth-bound -- so not the reference's one dispatch per depth level but two launches, each a thread per leaf
// that computes its leaf and then climbs:
//   A  the mesh forest, every listed mesh in one launch: the transfer of the leaf's triangle, the leaf, the climb;
//   B  the TLAS: the leaf from Transfers[i] and the node at SolidOffset (a root launch A refitted: the stream
//      orders the two), the climb.
// Each interior node has an arrival counter. The second arriver computes Union(left, left + 1) and writes the whole
// node; the first exits. No thread waits or spins. Nodes are handed between threads (workgroups, XCDs) exactly as
// refit_climb hands boxes: write-through sc1 stores, a vmcnt(0) drain, an agent-scope atomic arrive; the
// completing thread makes one agent-scope acquire (several workgroups per CU: outside the measured sc1-loads-only
// table of MI355X_MICROARCH.md, so it stays) and reads both children with L1-bypassing sc1 loads. It also resets the
// counter, so consecutive refits need no memset. A node is a pure function of its two children, so the bytes do
// not depend on who arrives first.
//
// The reference's `if (id.x > SetCount)` lets one thread per dispatch read past the working set; in D3D it reads
// index 0 and recomputes the tree's root early, and the root's own dispatch writes it again last. The final bytes
// are the same, and this one-launch form has no such thread.
#include "tt_light_refit.h"

#include "tt_light_refit_core.h"

namespace {

constexpr int kBlock = 256;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// a 40-byte node at byte 40 * id is 8-byte aligned: five write-through (sc1, aux 16) 8-byte stores
__device__ __forceinline__ void st_node(__amdgpu_buffer_rsrc_t nb, int32_t id, const tt_light_node& nd) {
    uint32_t w[10];
    __builtin_memcpy(w, &nd, 40);
    const uint32_t off = (uint32_t)id * 40u;
#pragma unroll
    for (int k = 0; k < 5; k++) __builtin_amdgcn_raw_buffer_store_b64(u32x2{w[2 * k], w[2 * k + 1]}, nb, off + 8u * k, 0, 16);
}
// two children: `first` is even, so the pair is one 80-byte, 16-byte-aligned block: five L1-bypassing (sc1) loads
__device__ __forceinline__ void ld_pair(__amdgpu_buffer_rsrc_t nb, int32_t first, tt_light_node& a, tt_light_node& b) {
    const uint32_t off = (uint32_t)first * 40u;
    u32x4 w[5];
#pragma unroll
    for (int k = 0; k < 5; k++) w[k] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(nb, off + 16u * k, 0, 16));
    __builtin_memcpy(&a, &w[0], 40);
    __builtin_memcpy(&b, reinterpret_cast<const char*>(&w[0]) + 40, 40);
}

// Writes leaf `id` and climbs: see the file comment. Ends at the tree's root (parent -1) or as a first arriver.
template <bool kCons>
__device__ __forceinline__ void climb(const LightRefitPlanDev& p, int32_t id, tt_light_node nd) {
    const __amdgpu_buffer_rsrc_t nb = __builtin_amdgcn_make_buffer_rsrc(p.nodes, 0, (int)(p.n_nodes * 40u), 0x00020000);
    for (;;) {
        st_node(nb, id, nd);
        const int2 u = p.up[id];
        if (u.x < 0) return;  // the root completes the tree
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the node has left this CU before the arrival
        const uint32_t prev = __hip_atomic_fetch_add(p.arrive + u.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev != 1u) return;  // the first of the parent's two children
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(p.arrive + u.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        id = u.x;
        // the parent's own `left` never changes: no refit writes another value there
        const int32_t left = __hip_atomic_load(&p.nodes[id].left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tt_light_node a, b;
        ld_pair(nb, u.y + left, a, b);
        nd = tt_lr::union_node<kCons>(a, b, left);
    }
}

template <bool kCons>
__global__ __launch_bounds__(kBlock) void light_refit_forest(LightRefitPlanDev p, const LightRefitBlock* __restrict__ blocks,
                                                             tt_light_tri* __restrict__ ltris,
                                                             const tt_cuda_triangle* __restrict__ tris, uint32_t n_tris) {
    const LightRefitBlock b = blocks[blockIdx.x];
    if (threadIdx.x >= b.count) return;
    const uint32_t leaf = b.first + threadIdx.x;
    const int32_t id = p.leaf_node[leaf];
    tt_light_tri& row = ltris[p.leaf_row[leaf]];
    // TransferKernel: TriTarget + TriOffset was checked at upload; past the triangles D3D reads zeros
    tt_light_tri T;
    T.TriTarget = row.TriTarget;
    const uint64_t agg = (uint64_t)T.TriTarget + (uint64_t)(uint32_t)b.tri_offset;
    if (agg < n_tris) {
        tt_lr::transfer_tri(tris[agg], T);
    } else {
        for (int k = 0; k < 3; k++) T.pos0[k] = T.posedge1[k] = T.posedge2[k] = 0.0f;
    }
    for (int k = 0; k < 3; k++) {
        row.pos0[k] = T.pos0[k];
        row.posedge1[k] = T.posedge1[k];
        row.posedge2[k] = T.posedge2[k];
    }
    tt_light_node nd = p.nodes[id];
    tt_lr::mesh_leaf(T, nd);
    climb<kCons>(p, id, nd);
}

template <bool kCons>
__global__ __launch_bounds__(kBlock) void light_refit_tlas(LightRefitPlanDev p, uint32_t leaf_first, uint32_t n_leaves,
                                                           const tt_light_transform* __restrict__ transforms, uint32_t n_transforms) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_leaves) return;
    const int32_t id = p.leaf_node[leaf_first + i];
    tt_light_node nd = p.nodes[id];
    const uint32_t t = (uint32_t)(-(nd.left + 1));
    tt_light_transform X;
    __builtin_memset(&X, 0, sizeof X);  // (past the transforms: zeros, D3D; the host refuses a wrong count)
    if (t < n_transforms) X = transforms[t];
    tt_light_node root;
    __builtin_memset(&root, 0, sizeof root);
    if ((uint32_t)X.SolidOffset < p.n_nodes) root = p.nodes[X.SolidOffset];
    tt_lr::tlas_leaf<kCons>(X.Transform, root, nd);
    climb<kCons>(p, id, nd);
}

}  // namespace

hipError_t tt_light_refit_forest(const LightRefitPlanDev& p, const LightRefitBlock* blocks, uint32_t n_blocks,
                                 tt_light_tri* ltris, const tt_cuda_triangle* tris, uint32_t n_tris, bool conservative,
                                 hipStream_t st) {
    if (!n_blocks) return hipSuccess;
    if (conservative)
        hipLaunchKernelGGL(light_refit_forest<true>, dim3(n_blocks), dim3(kBlock), 0, st, p, blocks, ltris, tris, n_tris);
    else
        hipLaunchKernelGGL(light_refit_forest<false>, dim3(n_blocks), dim3(kBlock), 0, st, p, blocks, ltris, tris, n_tris);
    return hipGetLastError();
}

hipError_t tt_light_refit_tlas(const LightRefitPlanDev& p, uint32_t leaf_first, uint32_t n_leaves,
                               const tt_light_transform* transforms, uint32_t n_transforms, bool conservative, hipStream_t st) {
    if (!n_leaves) return hipSuccess;
    const uint32_t grid = (n_leaves + kBlock - 1) / kBlock;
    if (conservative)
        hipLaunchKernelGGL(light_refit_tlas<true>, dim3(grid), dim3(kBlock), 0, st, p, leaf_first, n_leaves, transforms, n_transforms);
    else
        hipLaunchKernelGGL(light_refit_tlas<false>, dim3(grid), dim3(kBlock), 0, st, p, leaf_first, n_leaves, transforms, n_transforms);
    return hipGetLastError();
}
