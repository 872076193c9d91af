// tt_object_build.hip — a mesh built into a GPU-resident object without leaving the device
// (tt_object_build_device): ParentObject.BuildTotal (ParentObject.cs:973-1111) for one merged child with identity
// child->parent transform, as host/tt_scene.cpp's blas_prepare restates it, split in two passes around the
// device builder of tt_build.hip.
//
// Pass 1, one thread per source triangle: the three positions through the Unity index order (i0, i2, i1),
// AABB.Create / Extend / Validate (CommonVars.cs:304-402) with ParentScale = 0.001 / lossyScale, the 24-byte
// {BBMax, BBMin} box. The same pass checks every index against n_vertices and raises an error word: nothing is
// read through a bad index, and the host never loops over triangles.
//
// Pass 2, one thread per LEAF position i: s = cwbvh_indices[i], that triangle's vertices gathered again, the
// 88-byte CudaTriangle written at i, its 48-byte traversal record at i, leaf_of[s] = i. A record is a pure function
// of its source triangle, so no source-ordered AggTriangles array ever exists: one write instead of write, scattered
// read and write again. The stores are whole records at a per-lane stride (11 x 8 bytes, 3 x 16 bytes), as
// tt_blas_refit's Construct writes them.
//
// Numerics are the C# host's, not the HLSL's: normalized(v) = v / sqrt(x*x + y*y + z*z) with a correctly rounded
// square root (taken in double, as the host takes it) and three IEEE divisions when the magnitude exceeds 1e-5,
// else zero; PackOctahedral as tt_pack_octahedral (host/tt_scene.cpp) with its NaN / non-positive -> 0 conversions.
// The library is built -ffp-contract=off. Every byte equals the host build's.
//
// tt_objects_build_device does the same for M meshes in one call: both passes as one launch over all N triangles,
// driven by a device table of per-mesh arrays, scale and destinations, around the forest forms of the builder
// (tt_build.h), which run every level of every stage for all meshes together. Every object still owns its buffers:
// pass 2 and a node scatter write into them through the table.
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "tt_assemble.h"
#include "tt_build.h"
#include "tt_ctx.h"
#include "tt_object_batch_host.h"

namespace {

struct MeshDev {  // the mesh's arrays on the device; the nullable ones stay nullable
    const float* pos;
    const float* nrm;
    const float* tan;
    const float* uv;
    const int32_t* idx;
    const int32_t* matdat;
    uint32_t n_vertices, n_tris;
};

struct V3 {
    float x, y, z;
};

__device__ inline V3 load3(const float* __restrict__ p, uint32_t stride, uint32_t i) {
    const float* q = p + (size_t)stride * i;
    return V3{q[0], q[1], q[2]};
}

// Pass 1 for triangle t of mesh m: its box at o. false (and a zero box): an index outside the mesh's vertices.
__device__ inline bool triangle_box(const MeshDev& m, float sx, float sy, float sz, uint32_t t, float* __restrict__ o) {
    const int32_t* ip = m.idx + 3 * (size_t)t;
    const uint32_t i1 = (uint32_t)ip[0], i2 = (uint32_t)ip[2], i3 = (uint32_t)ip[1];
    if (i1 >= m.n_vertices || i2 >= m.n_vertices || i3 >= m.n_vertices) {  // (a negative index is a large one)
#pragma unroll
        for (int k = 0; k < 6; k++) o[k] = 0.0f;
        return false;
    }
    const V3 a = load3(m.pos, 3, i1), b = load3(m.pos, 3, i2), c = load3(m.pos, 3, i3);
    float mx[3] = {a.x, a.y, a.z}, mn[3] = {a.x, a.y, a.z};  // Create(V1, V2): both corners V1, then Extend(V2)
    const float pb[3] = {b.x, b.y, b.z}, pc[3] = {c.x, c.y, c.z}, s[3] = {sx, sy, sz};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (pb[k] < mn[k]) mn[k] = pb[k];
        if (pb[k] > mx[k]) mx[k] = pb[k];
        if (pc[k] < mn[k]) mn[k] = pc[k];
        if (pc[k] > mx[k]) mx[k] = pc[k];
        if (mx[k] - mn[k] < s[k]) {  // Validate(ParentScale)
            mn[k] -= s[k];
            mx[k] += s[k];
        }
    }
    o[0] = mx[0];
    o[1] = mx[1];
    o[2] = mx[2];
    o[3] = mn[0];
    o[4] = mn[1];
    o[5] = mn[2];
    return true;
}

__global__ __launch_bounds__(256) void tt_object_boxes_kernel(MeshDev m, float sx, float sy, float sz,
                                                              float* __restrict__ boxes, int* __restrict__ err) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= m.n_tris) return;
    if (!triangle_box(m, sx, sy, sz, t, boxes + 6 * (size_t)t)) atomicOr(err, 1);
}

// Vector3.normalized (UnityEngine): mag = (float)Math.Sqrt(x*x + y*y + z*z); mag > 1e-5 ? v / mag : zero. The
// square root goes through double as the host's does (the float intrinsics of the HIP headers map to the native,
// not correctly rounded, instruction); `/` is IEEE division in this build.
__device__ inline V3 normalized(V3 v) {
    const float mag = (float)sqrt((double)(v.x * v.x + v.y * v.y + v.z * v.z));
    if (mag > 1e-5f) return V3{v.x / mag, v.y / mag, v.z / mag};
    return V3{0.0f, 0.0f, 0.0f};
}

// CommonFunctions.PackOctahedral (CommonVars.cs:816-833), as tt_pack_octahedral states it
__device__ inline uint32_t pack_octahedral(V3 v) {
    const float halfMaxUInt16 = 32767.5f;
    const float sx = (v.x >= 0.0f) ? 1.0f : -1.0f, sy = (v.y >= 0.0f) ? 1.0f : -1.0f;
    const float absX = v.x * sx, absY = v.y * sy;
    const float Tot = absX + absY + fabsf(v.z);
    float tx = absX / Tot, ty = absY / Tot;
    if (v.z < 0.0f) {
        const float ox = tx;
        tx = 1.0f - ty;
        ty = 1.0f - ox;
    }
    const float fx = halfMaxUInt16 + tx * halfMaxUInt16 * sx;
    const float fy = halfMaxUInt16 + ty * halfMaxUInt16 * sy;
    const uint32_t ux = (fx == fx && fx > 0.0f) ? (uint32_t)fx : 0u;
    const uint32_t uy = (fy == fy && fy > 0.0f) ? (uint32_t)fy : 0u;
    return ux | (uy << 16);
}

// The bits of `a - b` as the host's subtraction leaves them. They differ from the GPU's only where the result is a
// NaN: the host returns a NaN operand as it is (quieted; the minuend's first) and a negative default NaN for
// inf - inf, the GPU returns the subtrahend's NaN with its sign flipped (tri 54, words 4 and 7 of the mesh with a NaN
// y coordinate in tests/test_gpu_object_batch.py: 0xffc00000 against the host's 0x7fc00000) and a positive default.
__device__ inline uint32_t host_sub_bits(float a, float b) {
    const float d = a - b;
    if (d == d) return __float_as_uint(d);
    if (a != a) return __float_as_uint(a) | 0x00400000u;
    if (b != b) return __float_as_uint(b) | 0x00400000u;
    return 0xffc00000u;
}

// Pass 2 for leaf position i of mesh m, whose source triangle is s (< n_tris): the 88-byte record and the traversal
// record at i, leaf_of[s] = i. Returns the triangle's MatDat.
__device__ inline uint32_t triangle_records(const MeshDev& m, uint32_t s, uint32_t i, tt_cuda_triangle* __restrict__ tris,
                                            TriPos* __restrict__ tripos, int32_t* __restrict__ leaf_of) {
    const int32_t* ip = m.idx + 3 * (size_t)s;  // pass 1 checked every index
    const uint32_t vi[3] = {(uint32_t)ip[0], (uint32_t)ip[2], (uint32_t)ip[1]};
    const V3 a = load3(m.pos, 3, vi[0]), b = load3(m.pos, 3, vi[1]), c = load3(m.pos, 3, vi[2]);
    uint32_t w[22];
    w[0] = __float_as_uint(a.x);
    w[1] = __float_as_uint(a.y);
    w[2] = __float_as_uint(a.z);
    w[3] = host_sub_bits(b.x, a.x);
    w[4] = host_sub_bits(b.y, a.y);
    w[5] = host_sub_bits(b.z, a.z);
    w[6] = host_sub_bits(c.x, a.x);
    w[7] = host_sub_bits(c.y, a.y);
    w[8] = host_sub_bits(c.z, a.z);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const V3 n = m.nrm ? load3(m.nrm, 3, vi[k]) : V3{0.0f, 1.0f, 0.0f};
        const V3 t = m.tan ? load3(m.tan, 4, vi[k]) : V3{1.0f, 0.0f, 0.0f};
        w[9 + k] = pack_octahedral(normalized(n));
        w[12 + k] = pack_octahedral(normalized(t));
        w[15 + 2 * k] = m.uv ? __float_as_uint(m.uv[2 * (size_t)vi[k]]) : 0u;
        w[16 + 2 * k] = m.uv ? __float_as_uint(m.uv[2 * (size_t)vi[k] + 1]) : 0u;
    }
    const uint32_t md = m.matdat ? (uint32_t)m.matdat[s] : 0u;
    w[21] = md;
    uint2* o = reinterpret_cast<uint2*>(tris + i);  // 88-byte records: 8-byte aligned
#pragma unroll
    for (int k = 0; k < 11; k++) o[k] = make_uint2(w[2 * k], w[2 * k + 1]);
    uint4* p = reinterpret_cast<uint4*>(tripos + i);  // tt_derive_tripos_kernel's bytes
    p[0] = make_uint4(w[0], w[1], w[2], w[3]);
    p[1] = make_uint4(w[4], w[5], w[6], w[7]);
    p[2] = make_uint4(w[8], md, 0u, 0u);
    leaf_of[s] = (int32_t)i;
    return md;
}

__global__ __launch_bounds__(256) void tt_object_records_kernel(MeshDev m, const int32_t* __restrict__ cwbvh_indices,
                                                                tt_cuda_triangle* __restrict__ tris,
                                                                TriPos* __restrict__ tripos, int32_t* __restrict__ leaf_of,
                                                                uint32_t* __restrict__ max_matdat, int* __restrict__ err) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t md = 0u;
    if (i < m.n_tris) {
        const uint32_t s = (uint32_t)cwbvh_indices[i];
        if (s >= m.n_tris) atomicOr(err, 2);  // not a permutation: the builder's own output, checked all the same
        else md = triangle_records(m, s, i, tris, tripos, leaf_of);
    }
    // the largest MatDat: one atomic per wave that saw a non-zero one
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)md, off, 64);
        md = o > md ? o : md;
    }
    if ((threadIdx.x & 63u) == 0u && md) atomicMax(max_matdat, md);
}

// ---- the batched forms (tt_objects_build_device): one launch over the N triangles of M meshes, driven by a device
// table of per-mesh arrays, scale and destinations, in the manner of tt_assemble_kernel's object table. Mesh k owns
// the batch's triangles [starts[k], starts[k + 1]); a thread finds its mesh by bisection of starts.
struct MeshTab {
    MeshDev m;
    float sx, sy, sz;          // ParentScale of this mesh
    tt_cwbvh_node* nodes;      // the object's own buffers (set before pass 2)
    tt_cuda_triangle* tris;
    TriPos* tripos;
    int32_t* leaf_of;
};

__device__ inline uint32_t range_of(const uint32_t* __restrict__ starts, uint32_t M, uint32_t t) {
    uint32_t lo = 0, hi = M - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void tt_objects_boxes_kernel(const MeshTab* __restrict__ tab,
                                                               const uint32_t* __restrict__ starts, uint32_t M, uint32_t N,
                                                               float* __restrict__ boxes, int* __restrict__ err,
                                                               int* __restrict__ mesh_err) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= N) return;
    const uint32_t k = range_of(starts, M, t);
    const MeshTab& e = tab[k];
    if (!triangle_box(e.m, e.sx, e.sy, e.sz, t - starts[k], boxes + 6 * (size_t)t)) {
        atomicOr(err, 1);
        atomicOr(mesh_err + k, 1);
    }
}

// cwbvh_indices: global leaf position -> global source triangle, as the forest builder leaves it
__global__ __launch_bounds__(256) void tt_objects_records_kernel(const MeshTab* __restrict__ tab,
                                                                 const uint32_t* __restrict__ starts, uint32_t M, uint32_t N,
                                                                 const int32_t* __restrict__ cwbvh_indices,
                                                                 uint32_t* __restrict__ max_matdat, int* __restrict__ err,
                                                                 int* __restrict__ mesh_err) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t md = 0u, k = M;  // k = M: a lane past the last triangle
    if (i < N) {
        k = range_of(starts, M, i);
        const MeshTab& e = tab[k];
        const uint32_t s = (uint32_t)cwbvh_indices[i] - starts[k];
        if (s >= e.m.n_tris) {
            atomicOr(err, 2);  // not a permutation of the mesh's triangles
            atomicOr(mesh_err + k, 1);
        } else {
            md = triangle_records(e.m, s, i - starts[k], e.tris, e.tripos, e.leaf_of);
        }
    }
    // the largest MatDat per mesh: one atomic per wave inside one mesh, else one per lane that saw a non-zero one
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
    if (__ballot(k != k0) == 0ull) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)md, off, 64);
            md = o > md ? o : md;
        }
        if ((threadIdx.x & 63u) == 0u && md && k0 < M) atomicMax(max_matdat + k0, md);
    } else if (md) {
        atomicMax(max_matdat + k, md);
    }
}

// the forest's nodes (mesh after mesh, node_base[M] = total) into every object's own node buffer
__global__ __launch_bounds__(256) void tt_objects_nodes_kernel(const MeshTab* __restrict__ tab,
                                                               const uint32_t* __restrict__ node_base, uint32_t M,
                                                               uint32_t total, const tt_cwbvh_node* __restrict__ src) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= total) return;
    const uint32_t k = range_of(node_base, M, x);
    static_assert(sizeof(tt_cwbvh_node) == 5 * sizeof(uint4), "a node is five 16-byte words");
    const uint4* s = reinterpret_cast<const uint4*>(src + x);
    uint4* d = reinterpret_cast<uint4*>(tab[k].nodes + (x - node_base[k]));
#pragma unroll
    for (int w = 0; w < 5; w++) d[w] = s[w];
}

// One nullable mesh array: staged from the host, or checked to be device memory.
template <class T>
tt_status mesh_array(tt_ctx* c, bool dev, const T* src, size_t count, DevBuf<T>& stage, const T*& out, const char* name) {
    out = nullptr;
    if (!src) return TT_OK;
    if (dev) {
        if (!is_device_ptr(src)) return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but %s is not device memory", name);
        out = src;
        return TT_OK;
    }
    TT_HIP(c, stage.alloc(count));
    TT_HIP(c, hipMemcpyAsync(stage.p, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    out = stage.p;
    return TT_OK;
}

struct RingEntry {  // one tt_timing_read entry around a stage
    tt_ctx* c;
    uint32_t slot = 0;
    hipError_t open() { return ring_open(c, c->timing, slot); }
    hipError_t close() { return ring_close(c, c->timing, slot); }
};

tt_status build_object(tt_ctx* c, const tt_mesh_input* mesh, const int32_t* presorted, uint32_t flags, tt_object** out,
                       tt_object_build_info* info) {
    if (flags & ~(uint32_t)TT_TRACE_DEVICE_PTRS) return fail(c, TT_ERR_INVALID_ARG, "tt_object_build_device: unknown flag");
    if (!mesh || !mesh->positions || !mesh->indices || !mesh->n_vertices)
        return fail(c, TT_ERR_INVALID_ARG, "tt_object_build_device: null mesh, positions or indices");
    if (mesh->n_indices < 3 || mesh->n_indices % 3)
        return fail(c, TT_ERR_INVALID_ARG, "tt_object_build_device: n_indices (%u) is not a positive multiple of 3", mesh->n_indices);
    const uint32_t n = mesh->n_indices / 3, nv = mesh->n_vertices;
    if (n >= (1u << 29) || (uint64_t)n * 48u >= (1ull << 32))
        return fail(c, TT_ERR_INVALID_ARG, "tt_object_build_device: triangle array of 4 GiB or more (the trace kernel addresses it with 32-bit offsets)");
    const bool dev = (flags & TT_TRACE_DEVICE_PTRS) != 0;
    const float scale[3] = {0.001f / mesh->lossy_scale[0], 0.001f / mesh->lossy_scale[1], 0.001f / mesh->lossy_scale[2]};
    if (presorted)  // the caller's lists index the boxes on the device: range-checked like tt_blas_build_device's
        for (size_t i = 0; i < 3 * (size_t)n; i++)
            if (presorted[i] < 0 || (uint32_t)presorted[i] >= n)
                return fail(c, TT_ERR_INVALID_ARG, "tt_object_build_device: presorted[%zu] out of range", i);
    TT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;

    DevBuf<float> s_pos, s_nrm, s_tan, s_uv;
    DevBuf<int32_t> s_idx, s_mat;
    MeshDev m{};
    m.n_vertices = nv;
    m.n_tris = n;
    tt_status s;
    if ((s = mesh_array(c, dev, mesh->positions, 3 * (size_t)nv, s_pos, m.pos, "positions")) != TT_OK) return s;
    if ((s = mesh_array(c, dev, mesh->normals, 3 * (size_t)nv, s_nrm, m.nrm, "normals")) != TT_OK) return s;
    if ((s = mesh_array(c, dev, mesh->tangents, 4 * (size_t)nv, s_tan, m.tan, "tangents")) != TT_OK) return s;
    if ((s = mesh_array(c, dev, mesh->uvs, 2 * (size_t)nv, s_uv, m.uv, "uvs")) != TT_OK) return s;
    if ((s = mesh_array(c, dev, mesh->indices, 3 * (size_t)n, s_idx, m.idx, "indices")) != TT_OK) return s;
    if ((s = mesh_array(c, dev, mesh->matdat, (size_t)n, s_mat, m.matdat, "matdat")) != TT_OK) return s;

    // ---- pass 1: boxes and the index check
    DevBuf<float> boxes;
    DevBuf<int> err;
    DevBuf<uint32_t> maxmat;
    TT_HIP(c, boxes.alloc(6 * (size_t)n));
    TT_HIP(c, err.alloc(1));
    TT_HIP(c, maxmat.alloc(1));
    TT_HIP(c, hipMemsetAsync(err.p, 0, sizeof(int), st));
    TT_HIP(c, hipMemsetAsync(maxmat.p, 0, sizeof(uint32_t), st));
    const unsigned grid = (n + 255u) / 256u;
    RingEntry ring{c};
    int e = 0;
    TT_HIP(c, ring.open());
    hipLaunchKernelGGL(tt_object_boxes_kernel, dim3(grid), dim3(256), 0, st, m, scale[0], scale[1], scale[2], boxes.p, err.p);
    TT_HIP(c, hipGetLastError());
    TT_HIP(c, ring.close());
    TT_HIP(c, hipMemcpyAsync(&e, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    TT_HIP(c, hipStreamSynchronize(st));
    if (e) return fail(c, TT_ERR_INVALID_ARG, "tt_object_build_device: an index is outside the mesh's %u vertices", nv);

    // ---- presort: the caller's, or on the device
    DevBuf<int32_t> pre;
    TT_HIP(c, pre.alloc(3 * (size_t)n));
    TT_HIP(c, ring.open());
    if (presorted) {
        TT_HIP(c, hipMemcpyAsync(pre.p, presorted, 3 * (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    } else if ((s = tt_build_presort_dev(st, boxes.p, n, pre.p)) != TT_OK) {
        return fail(c, s, "tt_object_build_device: %s", tt_build_error());
    }
    TT_HIP(c, ring.close());

    // ---- BVH2 + BVH8 + Aggregate
    tt_blas_dev B;
    TT_HIP(c, ring.open());
    if ((s = tt_build_blas_dev(st, boxes.p, n, pre.p, B)) != TT_OK)
        return fail(c, s, "tt_object_build_device: %s", tt_build_error());
    TT_HIP(c, ring.close());
    if ((uint64_t)B.n_nodes * std::max<uint64_t>(sizeof(tt_cwbvh_node), TT_NODE_STRIDE) >= (1ull << 32))
        return fail(c, TT_ERR_INVALID_ARG, "tt_object_build_device: node array of 4 GiB or more");
    boxes.release();
    pre.release();

    // ---- pass 2: leaf-ordered records, traversal records, the inverted leaf order
    std::unique_ptr<tt_object> o(new tt_object);
    TT_HIP(c, o->d_tris.alloc(n));
    TT_HIP(c, o->d_tripos.alloc(n));
    TT_HIP(c, o->d_leaf_of.alloc(n));
    TT_HIP(c, ring.open());
    hipLaunchKernelGGL(tt_object_records_kernel, dim3(grid), dim3(256), 0, st, m, B.cwbvh_indices.p, o->d_tris.p,
                       o->d_tripos.p, o->d_leaf_of.p, maxmat.p, err.p);
    TT_HIP(c, hipGetLastError());
    TT_HIP(c, ring.close());

    // ---- the host node mirror and the walk tt_object_create would have run on the same bytes
    uint32_t mm = 0;
    o->nodes.resize(B.n_nodes);
    TT_HIP(c, ring.open());
    TT_HIP(c, hipMemcpyAsync(o->nodes.data(), B.nodes.p, (size_t)B.n_nodes * sizeof(tt_cwbvh_node), hipMemcpyDeviceToHost, st));
    TT_HIP(c, ring.close());
    TT_HIP(c, hipMemcpyAsync(&mm, maxmat.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    TT_HIP(c, hipMemcpyAsync(&e, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    TT_HIP(c, hipStreamSynchronize(st));  // any context's stream may read the object from here on
    if (e) return fail(c, TT_ERR_UNSUPPORTED, "tt_object_build_device: cwbvh_indices is not a permutation");
    if (!tt_asm::walk_object(o->nodes.data(), B.n_nodes, nullptr, n, 0, o->walk))
        return fail(c, TT_ERR_UNSUPPORTED, "tt_object_build_device: the built BLAS fails validation: %s", o->walk.why.c_str());
    if (o->walk.leaf_tris != n)
        return fail(c, TT_ERR_UNSUPPORTED, "tt_object_build_device: the built BLAS names %llu triangles, the mesh has %u",
                    (unsigned long long)o->walk.leaf_tris, n);
    o->walk.max_matdat = mm;  // a built BLAS reaches every triangle: the device reduction over all of them
    o->d_nodes = std::move(B.nodes);
    o->device = c->device;
    o->n_nodes = B.n_nodes;
    o->n_tris = n;
    o->root = 0;
    o->built = true;
    tt_object_build_info& bi = o->build_info;
    bi.n_nodes = B.n_nodes;
    bi.n_tris = n;
    bi.bvh2_depth = B.bvh2_depth;
    bi.max_matdat = mm;
    for (int k = 0; k < 3; k++) {
        bi.aabb_max[k] = B.root_box[k];
        bi.aabb_min[k] = B.root_box[3 + k];
    }
    bi.presorted_on_host = presorted ? 1u : 0u;
    bi.pad = 0;
    if (info) *info = bi;
    *out = o.release();
    return TT_OK;
}

// A failed stage of the batch: the meshes its per-mesh flags name get `code`, the message names the lowest.
tt_status fail_meshes(tt_ctx* c, const int* mesh_err_dev, uint32_t M, tt_status code, tt_status* mesh_status, const char* what) {
    std::vector<int> flags(M, 0);
    TT_HIP(c, hipMemcpyAsync(flags.data(), mesh_err_dev, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    TT_HIP(c, hipStreamSynchronize(c->stream));
    const int first = tt_batch::mark_failed(flags.data(), M, code, mesh_status);
    return fail(c, code, "tt_objects_build_device: %s (mesh %d)", what, first);
}

// M meshes into M objects: the two mesh passes as one launch each around the forest builder (tt_build.hip), the
// objects' own buffers filled through the table. Nothing is handed out before everything has succeeded.
tt_status build_objects(tt_ctx* c, const tt_mesh_input* meshes, uint32_t M, const int32_t* const* presorted, uint32_t flags,
                        tt_object** out, tt_object_build_info* infos, tt_status* mesh_status) {
    if (flags & ~(uint32_t)TT_TRACE_DEVICE_PTRS) return fail(c, TT_ERR_INVALID_ARG, "tt_objects_build_device: unknown flag");
    std::string why;
    tt_status s = tt_batch::check_meshes(meshes, M, presorted, mesh_status, why);
    if (s != TT_OK) return fail(c, s, "tt_objects_build_device: %s", why.c_str());
    const bool dev = (flags & TT_TRACE_DEVICE_PTRS) != 0;
    if (dev)
        for (uint32_t m = 0; m < M; m++) {
            const tt_mesh_input& in = meshes[m];
            const void* arrays[6] = {in.positions, in.normals, in.tangents, in.uvs, in.indices, in.matdat};
            for (const void* a : arrays)
                if (a && !is_device_ptr(a)) {
                    tt_batch::set_status(mesh_status, m, TT_ERR_INVALID_ARG);
                    return fail(c, TT_ERR_INVALID_ARG,
                                "tt_objects_build_device: argument checks: TT_TRACE_DEVICE_PTRS set but an array of mesh %u is not device memory", m);
                }
        }
    tt_batch::Plan plan;
    tt_batch::make_plan(meshes, M, !dev, plan);
    const uint32_t N = plan.start[M];
    TT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;

    // ---- the meshes' arrays: read in place, or every host array in one device blob: the small meshes composed on
    // the host and sent a run at a time, the large ones (1 MiB and up) straight from the caller's arrays
    DevBuf<uint32_t> blob;
    std::unique_ptr<uint32_t[]> staging;  // (not zero-filled: only the small meshes' parts are ever touched)
    if (!dev) {
        std::vector<tt_batch::Copy> copies;
        staging.reset(new uint32_t[std::max<uint64_t>(plan.words, 1)]);
        tt_batch::stage_copies(meshes, M, plan, 1u << 18, staging.get(), copies);
        TT_HIP(c, blob.alloc(plan.words));
        for (const tt_batch::Copy& k : copies)
            TT_HIP(c, hipMemcpyAsync(blob.p + k.at, k.src, k.words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    std::vector<MeshTab> tab(M);
    for (uint32_t m = 0; m < M; m++) {
        const tt_mesh_input& in = meshes[m];
        MeshTab& e = tab[m];
        e = MeshTab{};
        if (dev) {
            e.m = MeshDev{in.positions, in.normals, in.tangents, in.uvs, in.indices, in.matdat, 0u, 0u};
        } else {
            const tt_batch::MeshOffsets& o = plan.off[m];
            auto f = [&](uint64_t at) { return at == tt_batch::kAbsent ? nullptr : reinterpret_cast<const float*>(blob.p + at); };
            auto i = [&](uint64_t at) { return at == tt_batch::kAbsent ? nullptr : reinterpret_cast<const int32_t*>(blob.p + at); };
            e.m = MeshDev{f(o.pos), f(o.nrm), f(o.tan), f(o.uv), i(o.idx), i(o.mat), 0u, 0u};
        }
        e.m.n_vertices = in.n_vertices;
        e.m.n_tris = in.n_indices / 3;
        e.sx = 0.001f / in.lossy_scale[0];
        e.sy = 0.001f / in.lossy_scale[1];
        e.sz = 0.001f / in.lossy_scale[2];
    }
    DevBuf<MeshTab> d_tab;
    DevBuf<uint32_t> d_starts, d_node_base, maxmat;
    DevBuf<float> boxes;
    DevBuf<int> err, mesh_err;
    TT_HIP(c, d_tab.alloc(M));
    TT_HIP(c, d_starts.alloc((size_t)M + 1));
    TT_HIP(c, boxes.alloc(6 * (size_t)N));
    TT_HIP(c, err.alloc(1));
    TT_HIP(c, mesh_err.alloc(M));
    TT_HIP(c, maxmat.alloc(M));
    TT_HIP(c, hipMemcpyAsync(d_tab.p, tab.data(), (size_t)M * sizeof(MeshTab), hipMemcpyHostToDevice, st));
    TT_HIP(c, hipMemcpyAsync(d_starts.p, plan.start.data(), ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    TT_HIP(c, hipMemsetAsync(err.p, 0, sizeof(int), st));
    TT_HIP(c, hipMemsetAsync(mesh_err.p, 0, (size_t)M * sizeof(int), st));
    TT_HIP(c, hipMemsetAsync(maxmat.p, 0, (size_t)M * sizeof(uint32_t), st));

    // ---- pass 1: boxes and the index check
    const unsigned grid = (N + 255u) / 256u;
    RingEntry ring{c};
    int e = 0;
    TT_HIP(c, ring.open());
    hipLaunchKernelGGL(tt_objects_boxes_kernel, dim3(grid), dim3(256), 0, st, d_tab.p, d_starts.p, M, N, boxes.p, err.p, mesh_err.p);
    TT_HIP(c, hipGetLastError());
    TT_HIP(c, ring.close());
    TT_HIP(c, hipMemcpyAsync(&e, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    TT_HIP(c, hipStreamSynchronize(st));
    if (e) return fail_meshes(c, mesh_err.p, M, TT_ERR_INVALID_ARG, mesh_status, "pass 1: an index is outside the mesh's vertices");

    // ---- presort: the callers' lists (made global) where supplied, the device's for the rest
    DevBuf<int32_t> pre;
    TT_HIP(c, pre.alloc(3 * (size_t)N));
    std::vector<unsigned char> sorted(M, 1);
    std::vector<std::vector<int32_t>> lists;  // alive until the copies have run
    uint32_t n_sorted = 0;
    TT_HIP(c, ring.open());
    for (uint32_t m = 0; m < M; m++) {
        const int32_t* list = presorted ? presorted[m] : nullptr;
        if (!list) {
            n_sorted++;
            continue;
        }
        sorted[m] = 0;
        const uint32_t s0 = plan.start[m], n = plan.start[m + 1] - s0;
        if (s0) {
            lists.emplace_back(3 * (size_t)n);
            tt_batch::globalize_presort(list, n, s0, lists.back().data());
            list = lists.back().data();
        }
        for (int d = 0; d < 3; d++)
            TT_HIP(c, hipMemcpyAsync(pre.p + (size_t)d * N + s0, list + (size_t)d * n, (size_t)n * sizeof(int32_t),
                                     hipMemcpyHostToDevice, st));
    }
    if (n_sorted && (s = tt_build_presort_forest(st, boxes.p, plan.start.data(), M, n_sorted == M ? nullptr : sorted.data(),
                                                 pre.p, mesh_status)) != TT_OK)
        return fail(c, s, "tt_objects_build_device: %s", tt_build_error());
    TT_HIP(c, ring.close());

    // ---- BVH2 + BVH8 + Aggregate, all meshes level by level together
    tt_forest_dev B;
    TT_HIP(c, ring.open());
    if ((s = tt_build_blas_forest(st, boxes.p, plan.start.data(), M, pre.p, B, mesh_status)) != TT_OK)
        return fail(c, s, "tt_objects_build_device: %s", tt_build_error());
    TT_HIP(c, ring.close());
    for (uint32_t m = 0; m < M; m++)
        if ((uint64_t)(B.node_base[m + 1] - B.node_base[m]) * std::max<uint64_t>(sizeof(tt_cwbvh_node), TT_NODE_STRIDE) >= (1ull << 32)) {
            tt_batch::set_status(mesh_status, m, TT_ERR_INVALID_ARG);
            return fail(c, TT_ERR_INVALID_ARG, "tt_objects_build_device: BVH8: node array of 4 GiB or more (mesh %u)", m);
        }
    boxes.release();
    pre.release();

    // ---- pass 2: every object's own buffers, written through the table
    std::vector<std::unique_ptr<tt_object>> objs(M);
    for (uint32_t m = 0; m < M; m++) {
        const uint32_t n = plan.start[m + 1] - plan.start[m], nn = B.node_base[m + 1] - B.node_base[m];
        objs[m].reset(new tt_object);
        tt_object& o = *objs[m];
        TT_HIP(c, o.d_nodes.alloc(nn));
        TT_HIP(c, o.d_tris.alloc(n));
        TT_HIP(c, o.d_tripos.alloc(n));
        TT_HIP(c, o.d_leaf_of.alloc(n));
        tab[m].nodes = o.d_nodes.p;
        tab[m].tris = o.d_tris.p;
        tab[m].tripos = o.d_tripos.p;
        tab[m].leaf_of = o.d_leaf_of.p;
    }
    const uint32_t total = B.node_base[M];
    TT_HIP(c, d_node_base.alloc((size_t)M + 1));
    TT_HIP(c, hipMemcpyAsync(d_tab.p, tab.data(), (size_t)M * sizeof(MeshTab), hipMemcpyHostToDevice, st));
    TT_HIP(c, hipMemcpyAsync(d_node_base.p, B.node_base.data(), ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    TT_HIP(c, ring.open());
    hipLaunchKernelGGL(tt_objects_records_kernel, dim3(grid), dim3(256), 0, st, d_tab.p, d_starts.p, M, N, B.cwbvh_indices.p,
                       maxmat.p, err.p, mesh_err.p);
    hipLaunchKernelGGL(tt_objects_nodes_kernel, dim3((total + 255u) / 256u), dim3(256), 0, st, d_tab.p, d_node_base.p, M, total,
                       B.nodes.p);
    TT_HIP(c, hipGetLastError());
    TT_HIP(c, ring.close());

    // ---- every node mirror in one copy, then the walk tt_object_create would have run, per object
    std::unique_ptr<tt_cwbvh_node[]> mirror(new tt_cwbvh_node[total]);  // (not zero-filled: the copy writes all of it)
    std::vector<uint32_t> mm(M, 0u);
    TT_HIP(c, ring.open());
    TT_HIP(c, hipMemcpyAsync(mirror.get(), B.nodes.p, (size_t)total * sizeof(tt_cwbvh_node), hipMemcpyDeviceToHost, st));
    TT_HIP(c, ring.close());
    TT_HIP(c, hipMemcpyAsync(mm.data(), maxmat.p, (size_t)M * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    TT_HIP(c, hipMemcpyAsync(&e, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    TT_HIP(c, hipStreamSynchronize(st));  // any context's stream may read the objects from here on
    if (e) return fail_meshes(c, mesh_err.p, M, TT_ERR_UNSUPPORTED, mesh_status, "pass 2: cwbvh_indices is not a permutation");
    int first_bad = -1;
    std::string first_why;
    for (uint32_t m = 0; m < M; m++) {
        tt_object& o = *objs[m];
        const uint32_t n = plan.start[m + 1] - plan.start[m], nn = B.node_base[m + 1] - B.node_base[m];
        o.nodes.assign(mirror.get() + B.node_base[m], mirror.get() + B.node_base[m + 1]);
        std::string w;
        if (!tt_asm::walk_object(o.nodes.data(), nn, nullptr, n, 0, o.walk)) w = "the built BLAS fails validation: " + o.walk.why;
        else if (o.walk.leaf_tris != n) w = "the built BLAS names " + std::to_string(o.walk.leaf_tris) + " triangles, the mesh has " + std::to_string(n);
        if (!w.empty()) {
            tt_batch::set_status(mesh_status, m, TT_ERR_UNSUPPORTED);
            if (first_bad < 0) {
                first_bad = (int)m;
                first_why = w;
            }
            continue;
        }
        o.walk.max_matdat = mm[m];  // a built BLAS reaches every triangle: the device reduction over all of them
        o.device = c->device;
        o.n_nodes = nn;
        o.n_tris = n;
        o.root = 0;
        o.built = true;
        tt_object_build_info& bi = o.build_info;
        bi.n_nodes = nn;
        bi.n_tris = n;
        bi.bvh2_depth = B.bvh2_depth[m];
        bi.max_matdat = mm[m];
        for (int k = 0; k < 3; k++) {
            bi.aabb_max[k] = B.root_box[6 * (size_t)m + k];
            bi.aabb_min[k] = B.root_box[6 * (size_t)m + 3 + k];
        }
        bi.presorted_on_host = sorted[m] ? 0u : 1u;
        bi.pad = 0;
    }
    if (first_bad >= 0)
        return fail(c, TT_ERR_UNSUPPORTED, "tt_objects_build_device: walk: %s (mesh %d)", first_why.c_str(), first_bad);
    for (uint32_t m = 0; m < M; m++) {
        if (infos) infos[m] = objs[m]->build_info;
        out[m] = objs[m].release();
    }
    return TT_OK;
}

}  // namespace

extern "C" {

tt_status tt_object_build_device(tt_ctx* c, const tt_mesh_input* mesh, const int32_t* presorted, uint32_t flags,
                                 tt_object** out, tt_object_build_info* info) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (!out) return fail(c, TT_ERR_INVALID_ARG, "tt_object_build_device: null output handle");
    *out = nullptr;
    TT_REFUSE_DEAD_STREAM(c);
    const tt_status s = build_object(c, mesh, presorted, flags, out, info);
    if (s != TT_OK) (void)hipStreamSynchronize(c->stream);  // nothing of the failed build is still in flight
    return s;
}

tt_status tt_objects_build_device(tt_ctx* c, const tt_mesh_input* meshes, uint32_t n_meshes, const int32_t* const* presorted,
                                  uint32_t flags, tt_object** out, tt_object_build_info* infos, tt_status* mesh_status) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (!out) return fail(c, TT_ERR_INVALID_ARG, "tt_objects_build_device: null output handles");
    for (uint32_t m = 0; m < n_meshes; m++) {
        out[m] = nullptr;
        if (mesh_status) mesh_status[m] = TT_OK;
    }
    TT_REFUSE_DEAD_STREAM(c);
    const tt_status s = build_objects(c, meshes, n_meshes, presorted, flags, out, infos, mesh_status);
    if (s != TT_OK) (void)hipStreamSynchronize(c->stream);  // nothing of the failed build is still in flight
    return s;
}

tt_status tt_object_read(tt_ctx* c, const tt_object* o, tt_cwbvh_node* nodes, tt_cuda_triangle* tris,
                         int32_t* leaf_of_triangle) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (!o) return fail(c, TT_ERR_INVALID_ARG, "tt_object_read: null object");
    TT_REFUSE_DEAD_STREAM(c);
    if (o->device != c->device) return fail(c, TT_ERR_INVALID_ARG, "tt_object_read: the object lives on device %d", o->device);
    TT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (nodes) TT_HIP(c, hipMemcpyAsync(nodes, o->d_nodes.p, (size_t)o->n_nodes * sizeof(tt_cwbvh_node), hipMemcpyDeviceToHost, st));
    if (tris) TT_HIP(c, hipMemcpyAsync(tris, o->d_tris.p, (size_t)o->n_tris * sizeof(tt_cuda_triangle), hipMemcpyDeviceToHost, st));
    if (leaf_of_triangle && o->built)
        TT_HIP(c, hipMemcpyAsync(leaf_of_triangle, o->d_leaf_of.p, (size_t)o->n_tris * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TT_HIP(c, hipStreamSynchronize(st));
    if (leaf_of_triangle && !o->built)
        return fail(c, TT_ERR_INVALID_ARG, "tt_object_read: an object of tt_object_create has no leaf order");
    return TT_OK;
}

tt_status tt_object_leaf_order_device(const tt_object* o, const int32_t** leaf_of_triangle_dev) {
    if (!o || !leaf_of_triangle_dev) return TT_ERR_INVALID_ARG;
    *leaf_of_triangle_dev = nullptr;
    if (!o->built) return TT_ERR_INVALID_ARG;
    *leaf_of_triangle_dev = o->d_leaf_of.p;
    return TT_OK;
}

}  // extern "C"
