// tt_terrain.h — device-side pieces shared by the heightmap kernels (tt_terrain.hip), the attribute resolve
// (tt_resolve.hip) and the bounce enqueue (tt_raygen.hip): the pinned Heightmap sample, the terrain normal and
// the comparisons the terrain code spells out
// (include/truetrace_hip.h: abs / max(0, q) / all(a < b) are plain IEEE comparisons, min / max NaN-ignoring).
#ifndef TT_TERRAIN_H
#define TT_TERRAIN_H
#include "tt_device.h"

namespace tt_ter {

// g = sin(atan(1.0f / 2.0f)) (IntersectionKernels.compute:511): the fp32 nearest 1/sqrt(5)
constexpr float kG = 0.44721359549995793928f;

__device__ __forceinline__ float min_nn(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }
__device__ __forceinline__ float max_nn(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
__device__ __forceinline__ float max0(float q) { return q > 0.0f ? q : 0.0f; }  // max(0, q): NaN -> 0
__device__ __forceinline__ float min1(float q) { return q < 1.0f ? q : 1.0f; }  // min(q, 1): NaN -> 1
// (uint)f as D3D: NaN -> 0, negative -> 0, saturating
__device__ __forceinline__ uint32_t d3d_f2u(float f) {
    if (!(f > 0.0f)) return 0u;
    if (f >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)f;
}

// The Heightmap atlas: binary16 texels, row-major (2-byte loads the vector L1 / L2 serve; no texture unit).
struct HeightView {
    const uint16_t* texels;
    uint32_t w, h;
};
__device__ __forceinline__ int clamp_texel(float c, uint32_t n) {
    const float hi = (float)(n - 1u);
    return (int)(c > 0.0f ? (c < hi ? c : hi) : 0.0f);
}
__device__ __forceinline__ float texel(const HeightView& M, int x, int y) {
    return (float)__builtin_bit_cast(_Float16, M.texels[(size_t)y * M.w + (size_t)x]);  // exact (v_cvt_f32_f16)
}
// Heightmap.SampleLevel(sampler_trilinear_clamp, uv, 0).x: the linear filter pinned for the alpha atlas
// (tt_traverse.h sample_linear). Every index is clamped into the atlas, whatever uv is (NaN -> texel 0).
__device__ __forceinline__ float sample(const HeightView& M, float u, float v) {
    const float x = u * (float)M.w - 0.5f, y = v * (float)M.h - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    const int ix0 = clamp_texel(x0, M.w), ix1 = clamp_texel(x0 + 1.0f, M.w);
    const int iy0 = clamp_texel(y0, M.h), iy1 = clamp_texel(y0 + 1.0f, M.h);
    const float t00 = texel(M, ix0, iy0), t10 = texel(M, ix1, iy0), t01 = texel(M, ix0, iy1), t11 = texel(M, ix1, iy1);
    const float a = t00 * (1.0f - fx) + t10 * fx;
    const float b = t01 * (1.0f - fx) + t11 * fx;
    return a * (1.0f - fy) + b * fy;
}
// the atlas uv of a terrain's unmapped uv: uv * (HeightMap.xy - HeightMap.zw) + HeightMap.zw
__device__ __forceinline__ float height(const HeightView& M, const tt_terrain& T, float u, float v) {
    return sample(M, u * (T.HeightMap[0] - T.HeightMap[2]) + T.HeightMap[2],
                  v * (T.HeightMap[1] - T.HeightMap[3]) + T.HeightMap[3]);
}

// GetHeightRaw / GetHeightmapNormal — CommonData.cginc:922-938 (normalize(v) = v * (1 / sqrt(dot(v, v)))). One copy
// serves the attribute resolve (tt_resolve.hip) and the bounce enqueue's terrain branch (tt_raygen.hip).
__device__ __forceinline__ float3 normalize_nn(float3 v) {
    const float inv = 1.0f / sqrtf(__builtin_fmaf(v.z, v.z, __builtin_fmaf(v.y, v.y, v.x * v.x)));
    return make_float3(v.x * inv, v.y * inv, v.z * inv);
}
__device__ __forceinline__ float height_raw(const HeightView& M, const tt_terrain& T, float x, float z) {
    x = x - T.PositionOffset[0];
    z = z - T.PositionOffset[2];
    const float dx = T.TerrainDim[0], dz = T.TerrainDim[1];
    const float u = min_nn(x / dx, dx / dx), v = min_nn(z / dz, dz / dz);
    return height(M, T, u, v) * (T.HeightScale * 2.0f);
}
__device__ __forceinline__ float3 heightmap_normal(const HeightView& M, const tt_terrain& T, float3 p) {
    const float3 c = make_float3(p.x, height_raw(M, T, p.x, p.z), p.z);
    const float3 ox = make_float3(p.x + 0.25f, height_raw(M, T, p.x + 0.25f, p.z + 0.0f), p.z);
    const float3 oy = make_float3(p.x, height_raw(M, T, p.x + 0.0f, p.z + 0.25f), p.z + 0.25f);
    const float3 a = normalize_nn(make_float3(ox.x - c.x, ox.y - c.y, ox.z - c.z));
    const float3 b = normalize_nn(make_float3(oy.x - c.x, oy.y - c.y, oy.z - c.z));
    return normalize_nn(make_float3(__builtin_fmaf(a.y, b.z, -(a.z * b.y)), __builtin_fmaf(a.z, b.x, -(a.x * b.z)),
                                    __builtin_fmaf(a.x, b.y, -(a.y * b.x))));
}

}  // namespace tt_ter
#endif
