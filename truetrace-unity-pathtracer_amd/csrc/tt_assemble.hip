// tt_assemble.hip — the scene-change path on the GPU: what AssetManager.AccumulateData dispatches per
// ParentObject (CombineNodeBuffers / CombineTriBuffers, GeneralMeshFunctions.compute:26-73, 372 threads per
// group and one record per thread) as ONE launch over all objects, plus the TriPos derivation of
// tt_object_create.
//
// The gather. Every object contributes three byte ranges (AsmSegment, tt_assemble.h): its 80-byte nodes, its
// 88-byte triangles and its 48-byte TriPos records. The ranges are laid end to end in a flat space of 16-byte
// units; the grid strides over fixed tiles of TT_ASM_TILE units (16 KiB), each block finds the segment of its
// tile's first unit by binary search once per tile, and a lane whose unit lies beyond that segment's end steps
// forward (a tile may straddle any number of small objects). Consecutive lanes take consecutive units, so every
// wave instruction moves 1 KiB of contiguous bytes whatever the record size: the record structure is ignored on
// purpose, a per-field or per-record copy of 88-byte records cannot coalesce.
//
// Alignment. Sources start their own allocations and node / TriPos destinations sit at multiples of 80 / 48
// bytes, so they always take 16-byte accesses. An 88-byte triangle destination is 16-byte aligned only at an
// even TriOffset: there the 16-byte load is regrouped into two 8-byte stores (`wide` = 0). A segment of an odd
// number of triangles ends in one 8-byte unit.
//
// TriPos is NOT derived again from the 88-byte read: it is a third copy stream from the records the object
// derived once. Fusing would save the 48-byte read per triangle (224 instead of 272 bytes of traffic) but needs
// record-granular work -- 22 dwords per triangle at 8-byte alignment, staged through LDS to stay coalesced --
// for a pass that runs when the object set changes, not per frame. The uniform unit copy keeps one code path
// for all three streams.
#include "tt_assemble.h"

namespace {

__global__ __launch_bounds__(TT_ASM_BLOCK) void tt_assemble_kernel(const AsmSegment* __restrict__ seg, uint32_t n_seg,
                                                                   uint64_t total_units, uint64_t n_tiles) {
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t base = tile * TT_ASM_TILE;
        // the first segment whose end lies beyond the tile's first unit (base < total_units: it exists)
        uint32_t lo = 0, hi = n_seg - 1u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (seg[mid].unit_end > base) hi = mid;
            else lo = mid + 1u;
        }
        uint32_t s = lo;
        uint64_t begin = s ? seg[s - 1u].unit_end : 0ull;
        AsmSegment cur = seg[s];
        // A tile of full units inside one 16-byte aligned segment (nearly every tile of a large object): all
        // loads are issued before the first store, four in flight per lane. Block-uniform condition.
        const uint64_t local = base - begin;
        if (cur.wide && !cur.dst_k && (local + TT_ASM_TILE) * 16u <= cur.bytes) {
            const uint4* __restrict__ src = reinterpret_cast<const uint4*>(cur.src) + local + threadIdx.x;
            uint4* __restrict__ dst = reinterpret_cast<uint4*>(cur.dst) + local + threadIdx.x;
            uint4 v[TT_ASM_UNITS_PER_THREAD];
#pragma unroll
            for (uint32_t k = 0; k < TT_ASM_UNITS_PER_THREAD; k++) v[k] = src[k * TT_ASM_BLOCK];
#pragma unroll
            for (uint32_t k = 0; k < TT_ASM_UNITS_PER_THREAD; k++) dst[k * TT_ASM_BLOCK] = v[k];
            continue;
        }
        // The general tile (segment ends, 8-byte aligned destinations, tails, the strided node copy): again every
        // load before the first store; what a lane stores where is kept per unit, lanes may sit in different
        // segments.
        uint4 v[TT_ASM_UNITS_PER_THREAD];
        uint8_t* dst[TT_ASM_UNITS_PER_THREAD];
        uint8_t* dst_k[TT_ASM_UNITS_PER_THREAD];
        uint32_t mode[TT_ASM_UNITS_PER_THREAD];  // 0 nothing, 1 one 16-byte store, 2 two 8-byte stores, 3 the 8-byte tail
#pragma unroll
        for (uint32_t k = 0; k < TT_ASM_UNITS_PER_THREAD; k++) {
            const uint64_t u = base + k * TT_ASM_BLOCK + threadIdx.x;
            mode[k] = 0u;
            dst[k] = dst_k[k] = nullptr;
            if (u >= total_units) continue;
            while (u >= cur.unit_end) {  // (u < total_units = the last segment's end: s stays in range)
                begin = cur.unit_end;
                cur = seg[++s];
            }
            const uint64_t lu = u - begin, off = lu * 16u;
            dst[k] = cur.dst + off;
            if (off + 16u <= cur.bytes) {
                v[k] = *reinterpret_cast<const uint4*>(cur.src + off);
                mode[k] = cur.wide ? 1u : 2u;
                if (cur.dst_k)  // the strided node copy: 5 units per node, the slot's padding was zeroed before
                    dst_k[k] = cur.dst_k + (size_t)(lu / 5u) * TT_NODE_STRIDE + (lu % 5u) * 16u;
            } else {  // the 8-byte tail of an odd number of 88-byte records
                const uint2 t = *reinterpret_cast<const uint2*>(cur.src + off);
                v[k] = make_uint4(t.x, t.y, 0u, 0u);
                mode[k] = 3u;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < TT_ASM_UNITS_PER_THREAD; k++) {
            if (mode[k] == 1u) {
                *reinterpret_cast<uint4*>(dst[k]) = v[k];
            } else if (mode[k] == 2u) {
                *reinterpret_cast<uint2*>(dst[k]) = make_uint2(v[k].x, v[k].y);
                *reinterpret_cast<uint2*>(dst[k] + 8) = make_uint2(v[k].z, v[k].w);
            } else if (mode[k] == 3u) {
                *reinterpret_cast<uint2*>(dst[k]) = make_uint2(v[k].x, v[k].y);
            }
            if (dst_k[k]) *reinterpret_cast<uint4*>(dst_k[k]) = v[k];
        }
    }
}

// one thread per triangle: dwords 0..8 (pos0, posedge1, posedge2) and 21 (MatDat) of the 88-byte record, read as
// 8-byte pairs (the records are 8-byte aligned), written as three 16-byte stores
__global__ __launch_bounds__(256) void tt_derive_tripos_kernel(const tt_cuda_triangle* __restrict__ tris,
                                                               TriPos* __restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint2* p = reinterpret_cast<const uint2*>(tris + t);
    const uint2 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4], m = p[10];
    uint4* o = reinterpret_cast<uint4*>(out + t);
    o[0] = make_uint4(a.x, a.y, b.x, b.y);
    o[1] = make_uint4(c.x, c.y, d.x, d.y);
    o[2] = make_uint4(e.x, m.y, 0u, 0u);
}

}  // namespace

hipError_t tt_launch_derive_tripos(const tt_cuda_triangle* tris, TriPos* out, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(tt_derive_tripos_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, tris, out, n);
    return hipGetLastError();
}

hipError_t tt_launch_assemble(const AsmSegment* seg, uint32_t n_seg, uint64_t total_units, hipStream_t st) {
    if (n_seg == 0 || total_units == 0) return hipSuccess;
    const uint64_t n_tiles = (total_units + TT_ASM_TILE - 1u) / TT_ASM_TILE;
    // memory-bound: at most 8 blocks per CU of a 256-CU part, the rest by the grid stride
    const uint32_t grid = (uint32_t)(n_tiles < 2048u ? n_tiles : 2048u);
    hipLaunchKernelGGL(tt_assemble_kernel, dim3(grid), dim3(TT_ASM_BLOCK), 0, st, seg, n_seg, total_units, n_tiles);
    return hipGetLastError();
}
