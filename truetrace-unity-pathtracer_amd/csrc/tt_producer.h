// tt_producer.h — device code the ray producers share (tt_raygen.hip: Generate and the bounce enqueue;
// tt_lights.hip: the NEE emit): the pinned vector helpers, random(), the octahedral codecs, the frame of a hit,
// and the decoupled look-back of the stable compaction. Each including file wraps it in its own unnamed namespace.
#pragma once
#include "tt_device.h"
#include "tt_terrain.h"

namespace {

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

__device__ __forceinline__ float3 normalize3(float3 v) {
    const float inv = 1.0f / sqrtf(fma_(v.z, v.z, fma_(v.y, v.y, v.x * v.x)));
    return make_float3(v.x * inv, v.y * inv, v.z * inv);
}
__device__ __forceinline__ float3 cross3(float3 a, float3 b) {
    return make_float3(fma_(a.y, b.z, -(a.z * b.y)), fma_(a.z, b.x, -(a.x * b.z)), fma_(a.x, b.y, -(a.y * b.x)));
}
__device__ __forceinline__ float dot3(float3 a, float3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }

// pcg_hash / hash_with / random() (non-ASVGF branch) — CommonData.cginc:374-389, :413-426
__device__ __forceinline__ uint32_t pcg_hash(uint32_t seed) {
    const uint32_t state = seed * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
__device__ __forceinline__ uint32_t hash_with(uint32_t seed, uint32_t hash) {
    seed = (seed ^ 61u) ^ hash;
    seed += seed << 3;
    seed ^= seed >> 4;
    seed *= 0x27d4eb2du;
    return seed;
}
__device__ __forceinline__ float2 random2(uint32_t samdim, uint32_t pixel_index, int32_t frames, int32_t max_bounce,
                                          int32_t cur_bounce) {
    const uint32_t hash = pcg_hash((pixel_index * 258u + samdim) * (uint32_t)(max_bounce + 1) + (uint32_t)cur_bounce);
    const float k = __uint_as_float(0x2f7fffffu);
    return make_float2((float)hash_with((uint32_t)frames, hash) * k, (float)hash_with((uint32_t)frames + 0xdeadbeefu, hash) * k);
}

__device__ __forceinline__ float3 i_octahedral_32(uint32_t data) {
    const uint32_t ix = data & 65535u, iy = (data >> 16) & 65535u;
    const float vx = (float)ix / 32767.5f - 1.0f, vy = (float)iy / 32767.5f - 1.0f;
    float3 nor = make_float3(vx, vy, 1.0f - fabsf(vx) - fabsf(vy));
    const float t = fmaxf(-nor.z, 0.0f);
    nor.x += (nor.x > 0.0f) ? -t : t;
    nor.y += (nor.y > 0.0f) ? -t : t;
    return normalize3(nor);
}
// octahedral_32 — CommonData.cginc:840-846 (round = round-half-even, DXIL Round_ne)
__device__ __forceinline__ uint32_t octahedral_32(float3 nor) {
    const float sx = nor.x >= 0.0f ? 1.0f : -1.0f, sy = nor.y >= 0.0f ? 1.0f : -1.0f;
    const float den = nor.x * sx + nor.y * sy + fabsf(nor.z);
    float x = nor.x / den, y = nor.y / den;
    if (!(nor.z >= 0.0f)) {
        const float ox = x;
        x = (1.0f - (y * sy)) * sx;
        y = (1.0f - (ox * sx)) * sy;
    }
    const uint32_t dx = (uint32_t)rintf(32767.5f + x * 32767.5f), dy = (uint32_t)rintf(32767.5f + y * 32767.5f);
    return dx | (dy << 16u);
}

__device__ __forceinline__ float3 mul_inv(const float* W, float3 x) {
    auto M = [&](int r, int c) { return W[c * 4 + r]; };
    return make_float3(fma_(M(2, 0), x.z, fma_(M(1, 0), x.y, M(0, 0) * x.x)),
                       fma_(M(2, 1), x.z, fma_(M(1, 1), x.y, M(0, 1) * x.x)),
                       fma_(M(2, 2), x.z, fma_(M(1, 2), x.y, M(0, 2) * x.x)));
}

// RayData as three 16-B words: (origin, PixelIndex), (direction, last_pdf), hits
struct Ray3 {
    uint4 a, b, h;
};
// The terrain set as the TERRAIN instantiation of the enqueue reads it (TerrainData array, Heightmap atlas).
struct TerrainSet {
    const tt_terrain* terrains;
    uint32_t n;
    tt_ter::HeightView hmap;
};
// a record the TERRAIN instantiation treats as a terrain hit; one with triangle_id >= n ends its path
__device__ __forceinline__ bool terrain_record(const uint4& h) { return h.x == TT_TERRAIN_MESH_ID; }

// The frame of a hit as kernel_shade derives it (RayTracingShader.compute:99-122, 293): pos, Geomnorm g and
// the unsmoothed normal us, both flipped for a backfacing hit. The enqueue (tt_raygen.hip) and the NEE emit
// (tt_lights.hip) share it, so their pos / norm / origin are the same bits.
struct HitFrame {
    float3 dir, pos, g, us;
};
template <bool TERRAIN>
__device__ __forceinline__ HitFrame hit_frame(const Ray3& R, const tt_cuda_triangle* tris, const tt_mesh_data* md,
                                              const TerrainSet& ter) {
    HitFrame H;
    const float t = __uint_as_float(R.h.z);
    const float3 dir = make_float3(__uint_as_float(R.b.x), __uint_as_float(R.b.y), __uint_as_float(R.b.z));
    const float3 org = make_float3(__uint_as_float(R.a.x), __uint_as_float(R.a.y), __uint_as_float(R.a.z));
    const float3 pos = make_float3(dir.x * t + org.x, dir.y * t + org.y, dir.z * t + org.z);
    float3 g, us;
    if (TERRAIN && terrain_record(R.h)) {
        // RayTracingShader.compute:109-111: Geomnorm = USGNorm = GetHeightmapNormal(pos, triangle_id); _MeshData and
        // AggTris are not read (the record's mesh_id indexes nothing). triangle_id < ter.n: pass 1 checked it.
        g = us = tt_ter::heightmap_normal(ter.hmap, ter.terrains[R.h.y], pos);
    } else {
        const int32_t mesh_id = (int32_t)R.h.x, tri = (int32_t)R.h.y;
        const float u = (float)(R.h.w & 0xffffu) / 65535.0f, v = (float)(R.h.w >> 16) / 65535.0f;
        const float* W = md[mesh_id].W2L;
        const tt_cuda_triangle& T = tris[tri];
        // Geomnorm (GetTriangleNormal) and USGNorm (RayTracingShader.compute:111-118)
        const float3 n0 = i_octahedral_32(T.norms[0]), n1 = i_octahedral_32(T.norms[1]), n2 = i_octahedral_32(T.norms[2]);
        const float w0 = 1.0f - u - v;
        g = mul_inv(W, make_float3(n0.x * w0 + u * n1.x + v * n2.x, n0.y * w0 + u * n1.y + v * n2.y,
                                   n0.z * w0 + u * n1.z + v * n2.z));
        g = normalize3(g);
        us = mul_inv(W, cross3(normalize3(make_float3(T.posedge1[0], T.posedge1[1], T.posedge1[2])),
                               normalize3(make_float3(T.posedge2[0], T.posedge2[1], T.posedge2[2]))));
        us = normalize3(us);
        us = make_float3(-us.x, -us.y, -us.z);
        if (dot3(us, g) < 0) us = make_float3(-us.x, -us.y, -us.z);
    }
    if (dot3(dir, us) > 0.0f) {  // GotFlipped: backfacing
        us = make_float3(-us.x, -us.y, -us.z);
        g = make_float3(-g.x, -g.y, -g.z);
    }
    H.dir = dir;
    H.pos = pos;
    H.g = g;
    H.us = us;
    return H;
}

// Decoupled look-back status word of a tile: bits 0-31 the count, bit 32 "aggregate" (this
// tile's own survivors), bit 33 "inclusive" (survivors of tiles [0, tile]); 0 = not yet published.
// Flag and value travel in one 64-bit word, so relaxed device-scope atomics suffice (no fences).
constexpr uint64_t TT_LB_AGG = 1ull << 32, TT_LB_INC = 2ull << 32;
__device__ __forceinline__ void lb_publish(unsigned long long* st, uint32_t tile, uint64_t flag, uint32_t v) {
    __hip_atomic_store(st + tile, (unsigned long long)(flag | v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Exclusive prefix of tile `tile` (> 0): one wave reads the 64 preceding status words at once
// (lane k reads tile - 1 - k), waits until all are published, sums up to and including the
// nearest inclusive one, and slides the window back when there is none.
__device__ __forceinline__ uint32_t lb_lookback(unsigned long long* st, uint32_t tile, uint32_t lane) {
    uint32_t prefix = 0;
    int32_t j = (int32_t)tile - 1;
    while (true) {
        const int32_t idx = j - (int32_t)lane;
        uint64_t w = TT_LB_INC;  // before tile 0: an inclusive zero
        if (idx >= 0) {
            do {
                w = __hip_atomic_load(st + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } while ((w >> 32) == 0u);
        }
        const uint64_t inc = __ballot((w & TT_LB_INC) != 0u);
        // lanes [0, first inclusive lane] contribute; none inclusive -> all 64, then slide
        const uint32_t stop = inc ? (uint32_t)__builtin_ctzll(inc) : 63u;
        uint32_t v = lane <= stop ? (uint32_t)w : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        prefix += v;
        if (inc) return prefix;
        j -= 64;
    }
}

}  // namespace
