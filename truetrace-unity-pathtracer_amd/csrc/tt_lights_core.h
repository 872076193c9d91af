// tt_lights_core.h — SampleLightBVH, Importance and the geometric subset of kernel_shade's NEE block
// (CommonData.cginc:1007-1043, :1126-1166, :1911-1920, :824-839; RayTracingShader.compute:391-479), one ray at a
// time. One text, two compilers: the kernel (tt_lights.hip, hipcc for gfx950) and the scalar host reference
// (host/tt_lights.cpp, g++) both build this header, so "bit for bit" between them is a statement about the two
// compilers' arithmetic under the numerics contract (-ffp-contract=off, the explicit fmaf chains, IEEE
// sqrt and divide, the pinned log2 / exp2), not about two restatements agreeing. The independent check of
// what is computed is the float64 model of tests/lights.py.
//
// Pins (Lights): dot(a, b) = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); normalize(v) = v * (1 /
// sqrt(dot(v, v))); length = sqrt(dot); mul(M, v) rows as fmaf chains, + the translation last; rcp(x) = 1 / x;
// pow(x, 2) = exp2(2 * log2(x)) with the pinned log2 / exp2 of tt_encode.h; max / min = IEEE maxNum / minNum;
// everything else is evaluated as written, left to right, unfused.
#ifndef TT_LIGHTS_CORE_H
#define TT_LIGHTS_CORE_H
#include <cstdint>
#include <cstring>

#include "../../include/truetrace_hip.h"

#if defined(__HIPCC__)
#include "tt_encode.h"
#define TT_LT_FN __device__ __forceinline__
#define TT_LT_SQRT(x) sqrtf(x)
#else
#include <cmath>
#define TT_LT_FN inline
#define TT_LT_SQRT(x) std::sqrt(x)
#endif

namespace tt_lt {

struct V3 {
    float x, y, z;
};

TT_LT_FN float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
TT_LT_FN float absf(float a) { return __builtin_fabsf(a); }
TT_LT_FN float maxf(float a, float b) { return __builtin_fmaxf(a, b); }
TT_LT_FN uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
TT_LT_FN float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
TT_LT_FN V3 ld3(const float* p) { return V3{p[0], p[1], p[2]}; }
TT_LT_FN V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
TT_LT_FN float dot(V3 a, V3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
TT_LT_FN float length(V3 a) { return TT_LT_SQRT(dot(a, a)); }
TT_LT_FN V3 normalize(V3 a) {
    const float k = 1.0f / TT_LT_SQRT(dot(a, a));
    return V3{a.x * k, a.y * k, a.z * k};
}
TT_LT_FN V3 cross(V3 a, V3 b) {
    return V3{fma_(a.y, b.z, -(a.z * b.y)), fma_(a.z, b.x, -(a.x * b.z)), fma_(a.x, b.y, -(a.y * b.x))};
}

#if defined(__HIPCC__)
TT_LT_FN float pow_pinned(float x, float y) { return tt_enc::pow_pinned(x, y); }
TT_LT_FN uint32_t pack_rgbe(float r, float g, float b) { return tt_enc::packRGBE(r, g, b); }
#else
// the host's statement of tt_encode.h's log2f_pinned / exp2f_pinned / packRGBE: the same operations in the same order
inline float log2f_pinned(float xf) {
    if (xf != xf || xf < 0.0f) return from_bits(0x7fc00000u);
    if (xf == 0.0f) return -__builtin_inff();
    if (xf == __builtin_inff()) return xf;
    int e;
    double m = std::frexp((double)xf, &e);
    if (m < 0.70710678118654752) {
        m = m * 2.0;
        e = e - 1;
    }
    const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    double p = 1.0 / 21.0;
    p = p * s2 + 1.0 / 19.0;
    p = p * s2 + 1.0 / 17.0;
    p = p * s2 + 1.0 / 15.0;
    p = p * s2 + 1.0 / 13.0;
    p = p * s2 + 1.0 / 11.0;
    p = p * s2 + 1.0 / 9.0;
    p = p * s2 + 1.0 / 7.0;
    p = p * s2 + 1.0 / 5.0;
    p = p * s2 + 1.0 / 3.0;
    p = p * s2 + 1.0;
    const double ln_m = 2.0 * s * p;
    return (float)((double)e + ln_m * 1.4426950408889634);
}
inline float exp2f_pinned(float yf) {
    if (yf != yf) return yf;
    if (yf >= 128.0f) return __builtin_inff();
    if (yf < -160.0f) return 0.0f;
    const double y = (double)yf, k = std::floor(y), f = y - k;
    const double r = f * 0.69314718055994531;
    double t = 1.0, sum = 1.0;
    for (int n = 1; n <= 22; n++) {
        t = t * r / (double)n;
        sum = sum + t;
    }
    return (float)std::ldexp(sum, (int)k);
}
inline float pow_pinned(float x, float y) { return exp2f_pinned(y * log2f_pinned(x)); }
inline uint32_t ftou(float f) {
    if (!(f > 0.0f)) return 0u;
    if (f >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)f;
}
inline uint32_t pack_rgbe(float r, float g, float b) {
    const float va[3] = {std::fmax(0.0f, r), std::fmax(0.0f, g), std::fmax(0.0f, b)};
    const float max_abs = std::fmax(va[0], std::fmax(va[1], va[2]));
    if (max_abs == 0.0f) return 0u;
    int e;
    (void)std::frexp(max_abs, &e);
    const float exponent = max_abs == __builtin_inff() ? __builtin_inff() : (float)(e - 1);
    uint32_t result = ftou(std::fmin(std::fmax(exponent + 20.0f, 0.0f), 31.0f)) << 27;
    const float scale = exp2f_pinned(-exponent) * 256.0f;
    uint32_t vu[3];
    for (int k = 0; k < 3; k++) vu[k] = ftou(std::fmin(511.0f, std::nearbyintf(va[k] * scale)));
    result |= vu[0];
    result |= vu[1] << 9;
    result |= vu[2] << 18;
    return result;
}
#endif

// pcg_hash / hash_with / random() (non-ASVGF branch) — CommonData.cginc:374-386, :417-426
TT_LT_FN uint32_t pcg_hash(uint32_t seed) {
    const uint32_t state = seed * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
TT_LT_FN uint32_t hash_with(uint32_t seed, uint32_t hash) {
    seed = (seed ^ 61u) ^ hash;
    seed += seed << 3;
    seed ^= seed >> 4;
    seed *= 0x27d4eb2du;
    return seed;
}
struct Rng {
    uint32_t pixel;
    int32_t frames, max_bounce, cur_bounce;
};
TT_LT_FN uint32_t rng_hash(const Rng& r, uint32_t samdim) {
    return pcg_hash((r.pixel * 258u + samdim) * (uint32_t)(r.max_bounce + 1) + (uint32_t)r.cur_bounce);
}
TT_LT_FN float random_x(const Rng& r, uint32_t samdim) {
    return (float)hash_with((uint32_t)r.frames, rng_hash(r, samdim)) * from_bits(0x2f7fffffu);
}
TT_LT_FN float random_y(const Rng& r, uint32_t samdim) {
    return (float)hash_with((uint32_t)r.frames + 0xdeadbeefu, rng_hash(r, samdim)) * from_bits(0x2f7fffffu);
}

TT_LT_FN V3 i_octahedral_32(uint32_t data) {
    const uint32_t ix = data & 65535u, iy = (data >> 16) & 65535u;
    const float vx = (float)ix / 32767.5f - 1.0f, vy = (float)iy / 32767.5f - 1.0f;
    V3 nor = {vx, vy, 1.0f - absf(vx) - absf(vy)};
    const float t = maxf(-nor.z, 0.0f);
    nor.x += (nor.x > 0.0f) ? -t : t;
    nor.y += (nor.y > 0.0f) ? -t : t;
    return normalize(nor);
}
// octahedral_32 — CommonData.cginc:841-847 (round = round-half-even)
TT_LT_FN uint32_t octahedral_32(V3 nor) {
    const float sx = nor.x >= 0.0f ? 1.0f : -1.0f, sy = nor.y >= 0.0f ? 1.0f : -1.0f;
    const float den = nor.x * sx + nor.y * sy + absf(nor.z);
    float x = nor.x / den, y = nor.y / den;
    if (!(nor.z >= 0.0f)) {
        const float ox = x;
        x = (1.0f - (y * sy)) * sx;
        y = (1.0f - (ox * sx)) * sy;
    }
    const uint32_t dx = (uint32_t)__builtin_rintf(32767.5f + x * 32767.5f), dy = (uint32_t)__builtin_rintf(32767.5f + y * 32767.5f);
    return dx | (dy << 16u);
}

// Unity column-major matrix: element (r, c) at m[c * 4 + r]
TT_LT_FN float M_(const float* m, int r, int c) { return m[c * 4 + r]; }
TT_LT_FN V3 mul33(const float* m, V3 d) {  // mul((float3x3)W, d)
    return V3{fma_(M_(m, 0, 2), d.z, fma_(M_(m, 0, 1), d.y, M_(m, 0, 0) * d.x)),
              fma_(M_(m, 1, 2), d.z, fma_(M_(m, 1, 1), d.y, M_(m, 1, 0) * d.x)),
              fma_(M_(m, 2, 2), d.z, fma_(M_(m, 2, 1), d.y, M_(m, 2, 0) * d.x))};
}
TT_LT_FN V3 mul34(const float* m, V3 o) {  // mul(W, float4(o, 1)).xyz
    const V3 r = mul33(m, o);
    return V3{r.x + M_(m, 0, 3), r.y + M_(m, 1, 3), r.z + M_(m, 2, 3)};
}
TT_LT_FN V3 mul33_t(const float* m, V3 x) {  // mul(transpose((float3x3)W), x): the enqueue's Inverse
    return V3{fma_(M_(m, 2, 0), x.z, fma_(M_(m, 1, 0), x.y, M_(m, 0, 0) * x.x)),
              fma_(M_(m, 2, 1), x.z, fma_(M_(m, 1, 1), x.y, M_(m, 0, 1) * x.x)),
              fma_(M_(m, 2, 2), x.z, fma_(M_(m, 1, 2), x.y, M_(m, 0, 2) * x.x))};
}

TT_LT_FN float det3(float a, float b, float c, float d, float e, float f, float g, float h, float i) {
    return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
}
// inverse(W) (CommonData.cginc:940-977) by cofactors: inv(i, j) = cof(j, i) * (1 / det), det along row 0.
// Written column-major like W, all 16 elements.
TT_LT_FN void inverse4(const float* W, float* inv) {
    float cof[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            const int r0 = r == 0 ? 1 : 0, r1 = r <= 1 ? 2 : 1, r2 = r <= 2 ? 3 : 2;
            const int c0 = c == 0 ? 1 : 0, c1 = c <= 1 ? 2 : 1, c2 = c <= 2 ? 3 : 2;
            const float m = det3(M_(W, r0, c0), M_(W, r0, c1), M_(W, r0, c2), M_(W, r1, c0), M_(W, r1, c1), M_(W, r1, c2),
                                 M_(W, r2, c0), M_(W, r2, c1), M_(W, r2, c2));
            cof[r * 4 + c] = ((r + c) & 1) ? -m : m;
        }
    const float det = M_(W, 0, 0) * cof[0] + M_(W, 0, 1) * cof[1] + M_(W, 0, 2) * cof[2] + M_(W, 0, 3) * cof[3];
    const float idet = 1.0f / det;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) inv[j * 4 + i] = cof[j * 4 + i] * idet;
}

TT_LT_FN float cos_sub_clamped(float sin_a, float cos_a, float sin_b, float cos_b) {
    if (cos_a > cos_b) return 1.0f;
    return cos_a * cos_b + sin_a * sin_b;
}
TT_LT_FN float sin_sub_clamped(float sin_a, float cos_a, float sin_b, float cos_b) {
    if (cos_a > cos_b) return 0.0f;
    return sin_a * cos_b - cos_a * sin_b;
}

// Importance — CommonData.cginc:1007-1043
TT_LT_FN float importance(V3 p, V3 n, const tt_light_node& nd) {
    const float cos_o = 2.0f * ((float)(nd.cosTheta_oe & 0x0000ffffu) / 32767.0f) - 1.0f;
    const V3 bmax = ld3(nd.BBMax), bmin = ld3(nd.BBMin);
    const V3 pc = {(bmax.x + bmin.x) / 2.0f, (bmax.y + bmin.y) / 2.0f, (bmax.z + bmin.z) / 2.0f};
    const V3 dp = sub(p, pc);
    const float p_diff = dot(dp, dp);
    const float d2 = maxf(p_diff, length(sub(bmax, bmin)) / 2.0f);
    const float s = TT_LT_SQRT(p_diff);
    const V3 wi = {(pc.x - p.x) / s, (pc.y - p.y) / s, (pc.z - p.z) / s};
    const float cos_w = absf(dot(i_octahedral_32(nd.w), wi));
    const float sin_w = TT_LT_SQRT(maxf(1.0f - cos_w * cos_w, 0.0f));
    float cos_b;
    {
        const bool inside = pc.x >= bmin.x && pc.y >= bmin.y && pc.z >= bmin.z && pc.x <= bmax.x && pc.y <= bmax.y && pc.z <= bmax.z;
        const V3 r = sub(bmax, pc);
        const float radius = inside ? dot(r, r) : 0.0f;
        if (p_diff < radius)
            cos_b = -1.0f;
        else
            cos_b = TT_LT_SQRT(maxf(1.0f - radius / p_diff, 0.0f));
    }
    const float sin_b = TT_LT_SQRT(maxf(1.0f - cos_b * cos_b, 0.0f));
    const float sin_o = TT_LT_SQRT(maxf(1.0f - cos_o * cos_o, 0.0f));
    const float cos_x = cos_sub_clamped(sin_w, cos_w, sin_o, cos_o);
    const float sin_x = sin_sub_clamped(sin_w, cos_w, sin_o, cos_o);
    const float cos_p = cos_sub_clamped(sin_x, cos_x, sin_b, cos_b);
    if (cos_p <= (2.0f * ((float)(nd.cosTheta_oe >> 16) / 32767.0f) - 1.0f)) return 0.0f;
    float imp = nd.phi * cos_p / d2;
    const float cos_i = dot(wi, n);
    const float sin_i = TT_LT_SQRT(maxf(1.0f - cos_i * cos_i, 0.0f));
    const float cos_pi = cos_sub_clamped(sin_i, cos_i, sin_b, cos_b);
    imp *= cos_pi;
    return maxf(imp, 0.0f);
}

struct Scene {
    const tt_light_node* nodes;
    const tt_light_tri* ltris;
    const tt_light_mesh* lmeshes;
    const tt_cuda_triangle* tris;
    const tt_mesh_data* md;
};

// The two children of a node: every `left` and every LightNodeOffset is even, so the pair is one 80-byte,
// 16-byte-aligned block: five 128-bit loads on the device.
TT_LT_FN void load_pair(const tt_light_node* nodes, uint32_t first, tt_light_node& a, tt_light_node& b) {
#if defined(__HIPCC__)
    const uint4* q = reinterpret_cast<const uint4*>(nodes + first);
    uint4 w[5];
#pragma unroll
    for (int k = 0; k < 5; k++) w[k] = q[k];
    memcpy(&a, &w[0], 40);
    memcpy(&b, reinterpret_cast<const char*>(&w[0]) + 40, 40);
#else
    a = nodes[first];
    b = nodes[first + 1];
#endif
}

// SampleLightBVH — CommonData.cginc:1126-1166. The text reloads LightNodes[node_index] each step for its `left`
// alone; the lane already holds it from the previous step's child pair, so it is carried.
TT_LT_FN int32_t sample_light_bvh(const Scene& S, V3 p, V3 n, const Rng& rng, float& pmf, int32_t& mesh_index, int32_t& reps) {
    int32_t left = S.nodes[0].left;
    int32_t node_offset = 0, start_index = 0;
    bool has_hit_tlas = false;
    reps = 0;
    while (reps < TT_LIGHT_MAX_REPS) {
        reps++;
        if (left >= 0) {
            tt_light_node a, b;
            load_pair(S.nodes, (uint32_t)(left + node_offset), a, b);
            const float cx = importance(p, n, a), cy = importance(p, n, b);
            if (cx == 0.0f && cy == 0.0f) break;
            const bool index = random_x(rng, 264u + (uint32_t)reps) >= (cx / (cx + cy));
            pmf /= ((index ? cy : cx) / (cx + cy));
            left = index ? b.left : a.left;
        } else {
            if (has_hit_tlas) return -(left + 1) + start_index;
            const tt_light_mesh& lm = S.lmeshes[-(left + 1)];
            start_index = lm.StartIndex;
            mesh_index = lm.LockedMeshIndex;
            const float* W = S.md[mesh_index].W2L;
            p = mul34(W, p);
            float inv[16];
            inverse4(W, inv);
            // mul(Inverse, float3(1, 0, 0)) is Inverse's first column, and so on
            const float sx = length(V3{M_(inv, 0, 0), M_(inv, 1, 0), M_(inv, 2, 0)});
            const float sy = length(V3{M_(inv, 0, 1), M_(inv, 1, 1), M_(inv, 2, 1)});
            const float sz = length(V3{M_(inv, 0, 2), M_(inv, 1, 2), M_(inv, 2, 2)});
            const V3 scale = {pow_pinned(1.0f / sx, 2.0f), pow_pinned(1.0f / sy, 2.0f), pow_pinned(1.0f / sz, 2.0f)};
            const V3 t = mul33(W, n);
            n = normalize(V3{t.x / scale.x, t.y / scale.y, t.z / scale.z});
            node_offset = S.md[mesh_index].LightNodeOffset;
            left = S.nodes[node_offset].left;
            has_hit_tlas = true;
        }
    }
    return -1;
}

// The hit's frame as the enqueue derives it (RayTracingShader.compute:99-122, 293): pos, the shading normal
// after its octahedral round trip, and ray.origin. The host's statement; the kernel takes these from the
// enqueue's own device code (tt_producer.h).
struct HitFrame {
    V3 pos, norm, origin;
};
TT_LT_FN HitFrame hit_frame(const tt_ray_data& R, const tt_cuda_triangle* tris, const tt_mesh_data* md) {
    const float t = from_bits(R.hits[2]);
    const V3 dir = ld3(R.direction), org = ld3(R.origin);
    HitFrame H;
    H.pos = V3{dir.x * t + org.x, dir.y * t + org.y, dir.z * t + org.z};
    const int32_t mesh_id = (int32_t)R.hits[0], tri = (int32_t)R.hits[1];
    const float u = (float)(R.hits[3] & 0xffffu) / 65535.0f, v = (float)(R.hits[3] >> 16) / 65535.0f;
    const float* W = md[mesh_id].W2L;
    const tt_cuda_triangle& T = tris[tri];
    const V3 n0 = i_octahedral_32(T.norms[0]), n1 = i_octahedral_32(T.norms[1]), n2 = i_octahedral_32(T.norms[2]);
    const float w0 = 1.0f - u - v;
    V3 g = normalize(mul33_t(W, V3{n0.x * w0 + u * n1.x + v * n2.x, n0.y * w0 + u * n1.y + v * n2.y, n0.z * w0 + u * n1.z + v * n2.z}));
    V3 us = normalize(mul33_t(W, cross(normalize(ld3(T.posedge1)), normalize(ld3(T.posedge2)))));
    us = V3{-us.x, -us.y, -us.z};
    if (dot(us, g) < 0) us = V3{-us.x, -us.y, -us.z};
    if (dot(dir, us) > 0.0f) {
        us = V3{-us.x, -us.y, -us.z};
        g = V3{-g.x, -g.y, -g.z};
    }
    H.norm = i_octahedral_32(octahedral_32(g));
    H.origin = V3{us.x * 0.0001f + H.pos.x, us.y * 0.0001f + H.pos.y, us.z * 0.0001f + H.pos.z};
    return H;
}

TT_LT_FN void miss_sample(tt_light_sample& s) {
    s.light_tri = s.mesh_index = s.agg_tri = -1;
    s.steps = 0;
    s.weight = s.area = 0.0f;
    for (int k = 0; k < 3; k++) s.position[k] = s.normal[k] = 0.0f;
}

// One hit: the light sample and, when it returns true, the shadow ray. pixel_index: the record's PixelIndex.
TT_LT_FN bool emit_one(const Scene& S, V3 pos, V3 norm, V3 origin, const Rng& rng, uint32_t pixel_index, bool negative_t,
                       tt_light_sample& smp, tt_shadow_ray& out) {
    miss_sample(smp);
    float weight = 1.0f;  // RunningWeight = selectionoptions = 1
    int32_t mesh_index = -1, reps = 0;
    const int32_t li = sample_light_bvh(S, pos, norm, rng, weight, mesh_index, reps);
    smp.mesh_index = mesh_index;
    smp.steps = reps;
    smp.weight = weight;
    if (li < 0) return false;
    const tt_light_tri& LT = S.ltris[li];
    // FinalUV = sample_triangle(random(79, pixel)) — CommonData.cginc:824-833
    float u1 = random_x(rng, 79u), u2 = random_y(rng, 79u);
    if (u2 > u1) {
        u1 *= 0.5f;
        u2 -= u1;
    } else {
        u2 *= 0.5f;
        u1 -= u2;
    }
    const V3 fp = {LT.pos0[0] + LT.posedge1[0] * u1 + LT.posedge2[0] * u2, LT.pos0[1] + LT.posedge1[1] * u1 + LT.posedge2[1] * u2,
                   LT.pos0[2] + LT.posedge1[2] * u1 + LT.posedge2[2] * u2};
    const tt_mesh_data& MD = S.md[mesh_index];
    const int32_t agg = (int32_t)LT.TriTarget + MD.TriOffset;
    const tt_cuda_triangle& T = S.tris[agg];
    float inv[16];
    inverse4(MD.W2L, inv);
    const V3 e1 = ld3(T.posedge1), e2 = ld3(T.posedge2);
    const V3 a1 = mul33(inv, e1), a2 = mul33(inv, e2);
    // AreaOfTriangle(0, a1, a2) — CommonData.cginc:979-985
    const float la = length(V3{0.0f - a1.x, 0.0f - a1.y, 0.0f - a1.z}), lb = length(sub(a1, a2)), lc = length(a2);
    const float hs = (la + lb + lc) / 2.0f;
    const float area = TT_LT_SQRT(hs * (hs - la) * (hs - lb) * (hs - lc));
    // mul(Minv, float4(LightPosition, 1)): a general inverse has a fourth row, but .xyz never reads it
    const V3 lp = mul34(inv, fp);
    const V3 ln = normalize(mul33(inv, normalize(cross(e1, e2))));
    smp.light_tri = li;
    smp.agg_tri = agg;
    smp.area = area;
    smp.position[0] = lp.x;
    smp.position[1] = lp.y;
    smp.position[2] = lp.z;
    smp.normal[0] = ln.x;
    smp.normal[1] = ln.y;
    smp.normal[2] = ln.z;
    // RayTracingShader.compute:419-426
    V3 to_light = sub(lp, origin);
    const float dist2 = dot(to_light, to_light);
    const float dist = TT_LT_SQRT(maxf(dist2, 0.0f));
    to_light = V3{to_light.x / dist, to_light.y / dist, to_light.z / dist};
    const float surface_cos = dot(to_light, norm);
    if (!(surface_cos > 0.0f)) return false;
    const float bsdf = surface_cos * 0.318309886548f;  // the diffuse stand-in: value = pdf = cos / pi
    if (!(bsdf > 0.0001f)) return false;
    const float nee_pdf = (1.0f / ((absf(dot(to_light, ln)) * area) / dist2)) / weight;  // :445
    const float mis = (nee_pdf * nee_pdf) / (nee_pdf * nee_pdf + bsdf * bsdf);          // power_heuristic
    const float illum = (bsdf / nee_pdf) * mis;
    const float t = dist - 0.01f;
    out.origin[0] = origin.x;
    out.origin[1] = origin.y;
    out.origin[2] = origin.z;
    out.LuminanceIncomming = from_bits(pack_rgbe(bsdf, bsdf, bsdf));
    out.direction[0] = to_light.x;
    out.direction[1] = to_light.y;
    out.direction[2] = to_light.z;
    out.t = negative_t ? -t : t;
    out.illumination[0] = out.illumination[1] = out.illumination[2] = illum;
    out.PixelIndex = pixel_index;
    return true;
}

// which records are hits the NEE block runs for: the enqueue's rule (a terrain record emits nothing)
TT_LT_FN bool is_hit(const uint32_t* hits, float far_plane, bool terrains) {
    const float t = from_bits(hits[2]);
    return t < far_plane && (int32_t)hits[1] >= 0 && !(terrains && hits[0] == TT_TERRAIN_MESH_ID);
}
// PixelIndex -> (pixel, frame) of the random numbers (tt_ctx_set_frame_pixels)
TT_LT_FN Rng make_rng(uint32_t pixel_index, uint32_t frame_pixels, int32_t frames, int32_t max_bounce, int32_t cur_bounce) {
    Rng r{pixel_index, frames, max_bounce, cur_bounce};
    if (frame_pixels) {
        const uint32_t j = pixel_index / frame_pixels;
        r.pixel = pixel_index - j * frame_pixels;
        r.frames = frames + (int32_t)j;
    }
    return r;
}

}  // namespace tt_lt
#endif
