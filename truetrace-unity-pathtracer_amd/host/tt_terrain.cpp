// tt_terrain.cpp — scalar host restatement of the reference's two heightmap kernels and the terrain
// normal, written from the HLSL (TrueTrace/Resources/MainCompute/IntersectionKernels.compute:508-710,
// CommonData.cginc:922-938). It is the reference the GPU kernels (csrc/tt_terrain.hip) are compared with
// bit for bit, and shares no code with them: it includes only the public headers.
//
// Numerics (include/truetrace_hip.h): IEEE + - * / and sqrt, no contraction (the file is compiled with
// -ffp-contract=off), rcp(x) = 1.0f / x, dot(a, b) = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)),
// cross(a, b).x = fmaf(a.y, b.z, -(a.z * b.y)), min / max NaN-ignoring, float -> uint as D3D (NaN -> 0,
// saturating); g = sin(atan(1/2)) is the fp32 nearest 1/sqrt(5); abs, max(0, q) and all(a < b) are plain
// IEEE comparisons; SampleLevel(sampler_trilinear_clamp, uv, 0) is the linear filter pinned for the alpha
// atlas (taps at floor(uv * size - 0.5) and + 1, clamped; lerp(a, b, f) = a * (1 - f) + b * f in x, then y)
// on exactly decoded binary16 texels.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/truetrace_scene.h"

namespace {

struct F3 {
    float x, y, z;
};

const float kG = 0.44721359549995793928f;  // :511 sin(atan(1.0f / 2.0f))

inline float min_nn(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }
inline float max_nn(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
inline float max0(float q) { return q > 0.0f ? q : 0.0f; }         // max(0, q): NaN -> 0
inline float min1(float q) { return q < 1.0f ? q : 1.0f; }         // min(q, 1): NaN -> 1
inline float absf(float q) {
    uint32_t u;
    std::memcpy(&u, &q, 4);
    u &= 0x7fffffffu;
    std::memcpy(&q, &u, 4);
    return q;
}
inline uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
inline float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
inline uint32_t d3d_f2u(float f) {  // (uint)f: NaN -> 0, negative -> 0, saturating
    if (!(f > 0.0f)) return 0u;
    if (f >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)f;
}
inline float half_to_float(uint16_t h) {  // exact
    const uint32_t s = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    if (e == 0x1fu) return from_bits(s | 0x7f800000u | (m << 13));
    if (e != 0u) return from_bits(s | ((e + 112u) << 23) | (m << 13));
    const float v = (float)m * 5.9604644775390625e-8f;  // m * 2^-24, exact
    return s ? -v : v;
}

struct Map {
    const uint16_t* texels;
    uint32_t w, h;
};
inline int clamp_texel(float c, uint32_t n) {
    const float hi = (float)(n - 1u);
    return (int)(c > 0.0f ? (c < hi ? c : hi) : 0.0f);
}
inline float texel(const Map& M, int x, int y) { return half_to_float(M.texels[(size_t)y * M.w + (size_t)x]); }
// Heightmap.SampleLevel(sampler_trilinear_clamp, uv, 0).x
float sample(const Map& M, float u, float v) {
    const float x = u * (float)M.w - 0.5f, y = v * (float)M.h - 0.5f;
    const float x0 = std::floor(x), y0 = std::floor(y);
    const float fx = x - x0, fy = y - y0;
    const int ix0 = clamp_texel(x0, M.w), ix1 = clamp_texel(x0 + 1.0f, M.w);
    const int iy0 = clamp_texel(y0, M.h), iy1 = clamp_texel(y0 + 1.0f, M.h);
    const float a = texel(M, ix0, iy0) * (1.0f - fx) + texel(M, ix1, iy0) * fx;
    const float b = texel(M, ix0, iy1) * (1.0f - fx) + texel(M, ix1, iy1) * fx;
    return a * (1.0f - fy) + b * fy;
}

// rayBoxIntersection — :513-521
bool ray_box(F3 o, F3 inv, F3 mn, F3 mx, float t_max, float& t0) {
    const F3 a = {(mn.x - o.x) * inv.x, (mn.y - o.y) * inv.y, (mn.z - o.z) * inv.z};
    const F3 b = {(mx.x - o.x) * inv.x, (mx.y - o.y) * inv.y, (mx.z - o.z) * inv.z};
    const F3 lo = {min_nn(a.x, b.x), min_nn(a.y, b.y), min_nn(a.z, b.z)};
    const F3 hi = {max_nn(a.x, b.x), max_nn(a.y, b.y), max_nn(a.z, b.z)};
    t0 = max_nn(lo.x, max_nn(lo.y, max_nn(lo.z, 0.025f)));
    const float t1 = min_nn(hi.x, min_nn(hi.y, min_nn(hi.z, t_max)));
    return t0 <= t1;
}

struct Counters {
    uint64_t samples = 0, exhausted = 0;
};

// GetDist — :604-618
bool get_dist(F3 p, float& u, float& v, float& dist, const tt_terrain& T, const Map& M, Counters& C) {
    const float dx = T.TerrainDim[0], dz = T.TerrainDim[1];
    F3 q = {absf(p.x) - dx, absf(p.y) - 0.01f, absf(p.z) - dz};
    q.x = q.x / dx;
    q.z = q.z / dz;
    u = min1(p.x / dx);
    v = min1(p.z / dz);
    float h = sample(M, u * (T.HeightMap[0] - T.HeightMap[2]) + T.HeightMap[2],
                     v * (T.HeightMap[1] - T.HeightMap[3]) + T.HeightMap[3]);
    C.samples++;
    h = h * (T.HeightScale * 2.0f);
    q.y = q.y - h;
    q.y = q.y * kG;
    const float b2 = q.y;
    q.x = max0(q.x);
    q.y = max0(q.y);
    q.z = max0(q.z);
    dist = std::sqrt(std::fmaf(q.z, q.z, std::fmaf(q.y, q.y, q.x * q.x)));
    return b2 != absf(b2);
}

inline F3 along(F3 o, F3 d, float t) { return {o.x + d.x * t, o.y + d.y * t, o.z + d.z * t}; }

bool valid_set(const tt_terrain* terrains, uint32_t n, const uint16_t* hm, uint32_t w, uint32_t h) {
    return (n == 0 || terrains) && hm && w && h;
}

}  // namespace

extern "C" {

// IntersectHeightMap — :620-703. detail (nullable), one word per ray: bit 0 the record was rewritten,
// bit 1 a bisection ran, bit 2 a march ended at the step bound, bits 8-15 the terrains (index < 8) whose
// box test passed, bits 16-23 the terrains (index < 8) that were hit.
tt_status tt_terrain_trace_detail_host(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap, uint32_t w,
                                       uint32_t h, const tt_trace_params* p, tt_ray_data* rays, uint32_t* primary_info,
                                       tt_stats* stats, uint32_t* detail) {
    if (!valid_set(terrains, n, heightmap, w, h) || !p || !rays || p->bounce < 0) return TT_ERR_INVALID_ARG;
    const Map M = {heightmap, w, h};
    const uint64_t wh = (uint64_t)p->screen_width * p->screen_height;
    const size_t off = (p->bounce % 2 == 1) ? (size_t)wh : 0u;  // :633
    const bool restir = (p->flags & TT_TRACE_USE_RESTIRGI) != 0;
    Counters C;
    uint64_t hits = 0;
    for (uint32_t r = 0; r < p->n_rays; r++) {
        tt_ray_data& R = rays[off + r];
        const F3 o2 = {R.origin[0], R.origin[1], R.origin[2]};            // ray2.origin
        const F3 d = {R.direction[0], R.direction[1], R.direction[2]};
        const F3 inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};             // :637
        float best_t = from_bits(R.hits[2]);                              // get(ray_index).t
        uint32_t dw = 0;
        float u = 0.0f, v = 0.0f;
        for (uint32_t i = 0; i < n; i++) {
            const tt_terrain& T = terrains[i];
            const F3 P = {T.PositionOffset[0], T.PositionOffset[1], T.PositionOffset[2]};
            const float dx = T.TerrainDim[0], dz = T.TerrainDim[1];
            const F3 mn = {P.x + 0.001f, P.y + 0.001f, P.z + 0.001f};
            const F3 mx = {(P.x + dx) - 0.001f, (P.y + dx) - 0.001f, (P.z + dz) - 0.001f};
            float t0;
            if (!ray_box(o2, inv, mn, mx, best_t, t0)) continue;  // :646
            if (i < 8u) dw |= 1u << (8u + i);
            float cur = 0.0f, prev = 0.0f, dist;
            const float s = max_nn(t0 + 0.0001f, 0.0f);
            const F3 o = {(o2.x + d.x * s) - P.x, (o2.y + d.y * s) - P.y, (o2.z + d.z * s) - P.z};  // :649
            int steps = 0;
            bool hit = false;
            while (true) {  // :653
                const F3 pos = along(o, d, cur);
                if (!(steps < TT_TERRAIN_MAX_STEPS && cur < best_t && pos.x < dx && pos.y < 1000.0f && pos.z < dz &&
                      pos.x > 0.0f && pos.y > 0.0f && pos.z > 0.0f))
                    break;
                steps++;
                const bool throwa = get_dist(pos, u, v, dist, T, M, C);  // :656
                if (dist < 0.0001f) {
                    if (throwa) {  // :658-677
                        dw |= 2u;
                        prev = prev / 2.0f;
                        cur = cur - prev;
                        for (int k = 0; k < 10; k++) {
                            if (get_dist(along(o, d, cur), u, v, dist, T, M, C)) {
                                prev = prev / 2.0f;
                                cur = cur - prev;
                            } else {
                                for (int k2 = 0; k2 < 10; k2++) {
                                    if (!get_dist(along(o, d, cur), u, v, dist, T, M, C)) {
                                        prev = prev / 2.0f;
                                        cur = cur + prev;
                                    } else {
                                        cur = cur - prev;
                                        break;
                                    }
                                }
                                break;
                            }
                        }
                    }
                    best_t = cur + t0;  // :684
                    const uint32_t pix = R.PixelIndex;
                    if (primary_info && pix < wh) {  // :687-691 (out-of-range texel writes are dropped)
                        uint32_t* o4 = primary_info + (size_t)4 * pix;
                        if (p->bounce == 0) {
                            o4[0] = TT_TERRAIN_MESH_ID;
                            o4[1] = i;
                            o4[2] = bits(u);
                            o4[3] = bits(v);
                        } else if (p->bounce == 1) {
                            if (!restir) {
                                o4[0] = bits(d.x);
                                o4[1] = bits(d.y);
                                o4[2] = bits(d.z);
                            } else {
                                o4[0] = bits(d.x * best_t + o2.x);
                                o4[1] = bits(d.y * best_t + o2.y);
                                o4[2] = bits(d.z * best_t + o2.z);
                            }
                            o4[3] = 1u;
                        }
                    }
                    R.hits[0] = TT_TERRAIN_MESH_ID;  // set() — CommonData.cginc:430-434
                    R.hits[1] = i;
                    R.hits[2] = bits(best_t);
                    R.hits[3] = d3d_f2u(u * 65535.0f) | (d3d_f2u(v * 65535.0f) << 16);
                    hit = true;
                    dw |= 1u;
                    if (i < 8u) dw |= 1u << (16u + i);
                    break;  // :693
                }
                prev = dist;
                cur = cur + dist;
            }
            if (!hit && steps >= TT_TERRAIN_MAX_STEPS) {
                C.exhausted++;
                dw |= 4u;
            }
        }
        if (dw & 1u) hits++;
        if (detail) detail[r] = dw;
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->rays = p->n_rays;
        stats->hits = hits;
        stats->node_visits = C.samples;
        stats->reps_exhausted = C.exhausted;
    }
    return TT_OK;
}

tt_status tt_terrain_trace_host(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap, uint32_t w, uint32_t h,
                                const tt_trace_params* p, tt_ray_data* rays, uint32_t* primary_info, tt_stats* stats) {
    return tt_terrain_trace_detail_host(terrains, n, heightmap, w, h, p, rays, primary_info, stats, nullptr);
}

// IntersectHeightMapShadow — :525-560, for the rays kernel_shadow_heightmap marches (t != 0, :570).
tt_status tt_terrain_occluded_host(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap, uint32_t w,
                                   uint32_t h, const tt_shadow_ray* shadow_rays, uint32_t n_rays, uint8_t* occluded_out,
                                   tt_stats* stats) {
    if (!valid_set(terrains, n, heightmap, w, h) || !shadow_rays || !occluded_out) return TT_ERR_INVALID_ARG;
    const Map M = {heightmap, w, h};
    Counters C;
    uint64_t marched = 0, occluded = 0;
    for (uint32_t r = 0; r < n_rays; r++) {
        const tt_shadow_ray& R = shadow_rays[r];
        occluded_out[r] = 0;
        if (!(R.t != 0.0f)) continue;  // :570
        marched++;
        const float max_dist = absf(R.t);
        const F3 origin = {R.origin[0], R.origin[1], R.origin[2]};
        const F3 d = {R.direction[0], R.direction[1], R.direction[2]};
        const F3 inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
        bool occ = false;
        for (uint32_t i = 0; i < n && !occ; i++) {
            const tt_terrain& T = terrains[i];
            const F3 P = {T.PositionOffset[0], T.PositionOffset[1], T.PositionOffset[2]};
            const float dx = T.TerrainDim[0], dz = T.TerrainDim[1];
            const F3 mx = {P.x + dx, P.y + dx, P.z + dz};
            float t0;
            if (!ray_box(origin, inv, P, mx, max_dist, t0)) continue;  // :530
            const float s = t0 + 0.001f;
            const F3 o = {(origin.x + d.x * s) - P.x, (origin.y + d.y * s) - P.y, (origin.z + d.z * s) - P.z};  // :531
            F3 cur_pos = o;
            int steps = 0;
            float dist_sum = 0.0f;
            while (true) {  // :535: the position test on `> 0` sees the previous iteration's CurrentPos
                const F3 pos = along(o, d, dist_sum);
                if (!(steps < TT_TERRAIN_MAX_STEPS && dist_sum < max_dist && pos.x < dx && pos.y < 1000.0f && pos.z < dz &&
                      cur_pos.x > 0.0f && cur_pos.y > 0.0f && cur_pos.z > 0.0f))
                    break;
                cur_pos = pos;
                float u, v, dist;
                steps++;
                (void)get_dist(cur_pos, u, v, dist, T, M, C);  // :537-549, the same arithmetic as GetDist
                if (dist < 0.0001f) {
                    occ = true;
                    break;
                }
                dist_sum = dist_sum + dist;
            }
            if (!occ && steps >= TT_TERRAIN_MAX_STEPS) C.exhausted++;
        }
        occluded_out[r] = occ ? 1 : 0;
        if (occ) occluded++;
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->rays = marched;
        stats->hits = occluded;
        stats->node_visits = C.samples;
        stats->reps_exhausted = C.exhausted;
    }
    return TT_OK;
}

}  // extern "C"

namespace {

inline F3 normalize(F3 a) {  // v * (1 / sqrt(dot(v, v)))
    const float k = 1.0f / std::sqrt(std::fmaf(a.z, a.z, std::fmaf(a.y, a.y, a.x * a.x)));
    return F3{a.x * k, a.y * k, a.z * k};
}
inline F3 cross(F3 a, F3 b) {
    return {std::fmaf(a.y, b.z, -(a.z * b.y)), std::fmaf(a.z, b.x, -(a.x * b.z)), std::fmaf(a.x, b.y, -(a.y * b.x))};
}
inline float dot(F3 a, F3 b) { return std::fmaf(a.z, b.z, std::fmaf(a.y, b.y, a.x * b.x)); }

// pcg_hash / hash_with / random() (non-ASVGF branch) — CommonData.cginc:374-389, :413-426
inline uint32_t pcg_hash(uint32_t seed) {
    const uint32_t state = seed * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
inline uint32_t hash_with(uint32_t seed, uint32_t hash) {
    seed = (seed ^ 61u) ^ hash;
    seed += seed << 3;
    seed ^= seed >> 4;
    seed *= 0x27d4eb2du;
    return seed;
}
inline void random2(uint32_t samdim, uint32_t pixel, int32_t frames, int32_t max_bounce, int32_t cur_bounce, float& rx,
                    float& ry) {
    const uint32_t hash = pcg_hash((pixel * 258u + samdim) * (uint32_t)(max_bounce + 1) + (uint32_t)cur_bounce);
    const float k = from_bits(0x2f7fffffu);  // 2.3283064365386963e-10
    rx = (float)hash_with((uint32_t)frames, hash) * k;
    ry = (float)hash_with((uint32_t)frames + 0xdeadbeefu, hash) * k;
}

// sin / cos of the disc-sample angle, pinned (truetrace_hip.h: the cephes single-precision minimax polynomials on
// [-pi/4, pi/4] with explicit FMAs; |phi| > pi/4 reduced by pi/2 with a two-constant Cody-Waite step)
inline void sincos_pinned(float phi, float& s, float& c) {
    const bool big = absf(phi) > 0.785398185253143310546875f;
    const float q = phi > 0.0f ? 1.0f : -1.0f;
    const float r = big ? std::fmaf(-q, -4.37113882867379e-8f, std::fmaf(-q, 1.57079637050628662109375f, phi)) : phi;
    const float z = r * r;
    const float sp =
        std::fmaf(std::fmaf(std::fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f) * z, r, r);
    const float cp = std::fmaf(
        std::fmaf(std::fmaf(std::fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), z, -0.5f),
        z, 1.0f);
    s = big ? q * cp : sp;   // phi = q pi/2 + r: sin(phi) = q cos(r)
    c = big ? -q * sp : cp;  //                   cos(phi) = -q sin(r)
}

// sample(): the cosine-weighted hemisphere direction and its pdf — RayTracingShader.compute:52-84
inline F3 cosine_sample(uint32_t pixel, int32_t frames, int32_t max_bounce, int32_t cur_bounce, float& pdf) {
    float rx, ry;
    random2(1, pixel, frames, max_bounce, cur_bounce, rx, ry);
    float a = 2.0f * rx - 1.0f, b = 2.0f * ry - 1.0f;
    if (a == 0.0f) a = 0.00001f;
    if (b == 0.0f) b = 0.00001f;
    float phi, rr;
    if (a * a > b * b) {
        rr = a;
        phi = (0.25f * 3.14159265f) * (b / a);
    } else {
        rr = b;
        phi = (0.25f * 3.14159265f) * (a / b) + (0.5f * 3.14159265f);
    }
    float sp, cp;
    sincos_pinned(phi, sp, cp);
    const float dx = rr * cp, dz = rr * sp;
    const F3 om = {dx, std::sqrt(absf(1.0f - (dx * dx + dz * dz))), dz};
    pdf = om.y * 0.318309886548f;
    return om;
}

// octahedral_32 / i_octahedral_32 — CommonData.cginc:840-857 (round = round-half-even)
inline uint32_t octahedral_32(F3 nor) {
    const float sx = nor.x >= 0.0f ? 1.0f : -1.0f, sy = nor.y >= 0.0f ? 1.0f : -1.0f;
    const float den = nor.x * sx + nor.y * sy + absf(nor.z);
    float x = nor.x / den, y = nor.y / den;
    if (!(nor.z >= 0.0f)) {
        const float ox = x;
        x = (1.0f - (y * sy)) * sx;
        y = (1.0f - (ox * sx)) * sy;
    }
    const uint32_t dx = (uint32_t)std::nearbyintf(32767.5f + x * 32767.5f);
    const uint32_t dy = (uint32_t)std::nearbyintf(32767.5f + y * 32767.5f);
    return dx | (dy << 16u);
}
inline F3 i_octahedral_32(uint32_t data) {
    const uint32_t ix = data & 65535u, iy = (data >> 16) & 65535u;
    const float vx = (float)ix / 32767.5f - 1.0f, vy = (float)iy / 32767.5f - 1.0f;
    F3 nor = {vx, vy, 1.0f - absf(vx) - absf(vy)};
    const float t = max_nn(-nor.z, 0.0f);
    nor.x += (nor.x > 0.0f) ? -t : t;
    nor.y += (nor.y > 0.0f) ? -t : t;
    return normalize(nor);
}

// GetHeightmapNormal — CommonData.cginc:922-938
F3 heightmap_normal(const tt_terrain& T, const Map& M, F3 pos) {
    auto height_raw = [&](F3 p) {  // GetHeightRaw
        p.x = p.x - T.PositionOffset[0];
        p.z = p.z - T.PositionOffset[2];
        const float dx = T.TerrainDim[0], dz = T.TerrainDim[1];
        const float u = min_nn(p.x / dx, dx / dx), v = min_nn(p.z / dz, dz / dz);
        const float s = sample(M, u * (T.HeightMap[0] - T.HeightMap[2]) + T.HeightMap[2],
                               v * (T.HeightMap[1] - T.HeightMap[3]) + T.HeightMap[3]);
        return s * (T.HeightScale * 2.0f);
    };
    const F3 c = {pos.x, height_raw(pos), pos.z};
    const F3 ox = {pos.x + 0.25f, height_raw({pos.x + 0.25f, pos.y + 0.0f, pos.z + 0.0f}), pos.z};
    const F3 oy = {pos.x, height_raw({pos.x + 0.0f, pos.y + 0.0f, pos.z + 0.25f}), pos.z + 0.25f};
    const F3 a = normalize({ox.x - c.x, ox.y - c.y, ox.z - c.z}), b = normalize({oy.x - c.x, oy.y - c.y, oy.z - c.z});
    return normalize(cross(a, b));
}

}  // namespace

extern "C" {

tt_status tt_terrain_normal_host(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap, uint32_t w, uint32_t h,
                                 const float* position3, uint32_t terrain_id, float* normal3) {
    if (!valid_set(terrains, n, heightmap, w, h) || !position3 || !normal3 || terrain_id >= n) return TT_ERR_INVALID_ARG;
    const F3 nn = heightmap_normal(terrains[terrain_id], Map{heightmap, w, h}, {position3[0], position3[1], position3[2]});
    normal3[0] = nn.x;
    normal3[1] = nn.y;
    normal3[2] = nn.z;
    return TT_OK;
}

// The terrain rows of the diffuse bounce enqueue (kernel_shade's next-ray subset with the terrain branch,
// RayTracingShader.compute:52-84, 99-122, 293, 498-506): the reference of TT_ENQUEUE_TERRAIN_BOUNCE.
tt_status tt_terrain_bounce_host(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap, uint32_t w, uint32_t h,
                                 const tt_trace_params* p, const tt_ray_data* global_rays, int32_t frames,
                                 int32_t max_bounce, uint32_t frame_pixels, tt_ray_data* out_rays, int32_t* survives) {
    if (!valid_set(terrains, n, heightmap, w, h) || !p || !global_rays || !out_rays || !survives || p->bounce < 0)
        return TT_ERR_INVALID_ARG;
    const Map M = {heightmap, w, h};
    const uint64_t wh = (uint64_t)p->screen_width * p->screen_height;
    const size_t off = (p->bounce % 2 == 1) ? (size_t)wh : 0u;
    for (uint32_t i = 0; i < p->n_rays; i++) {
        const tt_ray_data& R = global_rays[off + i];
        const float t = from_bits(R.hits[2]);
        if (R.hits[0] != TT_TERRAIN_MESH_ID) {  // a miss or a triangle record: not ours
            survives[i] = -1;
            continue;
        }
        survives[i] = 0;
        if (!(t < p->far_plane) || R.hits[1] >= n) continue;  // (malformed: triangle_id past the set) the path ends
        // batched frames (tt_ctx_set_frame_pixels): PixelIndex p is pixel p mod n of frame p / n
        uint32_t px = R.PixelIndex;
        int32_t fr = frames;
        if (frame_pixels) {
            const uint32_t j = px / frame_pixels;
            px -= j * frame_pixels;
            fr += (int32_t)j;
        }
        float pdf;
        const F3 om = cosine_sample(px, fr, max_bounce, p->bounce, pdf);
        if (!(pdf > 0.0f)) continue;
        const F3 dir = {R.direction[0], R.direction[1], R.direction[2]};
        const F3 pos = {dir.x * t + R.origin[0], dir.y * t + R.origin[1], dir.z * t + R.origin[2]};
        F3 g = heightmap_normal(terrains[R.hits[1]], M, pos);  // :109-111 Geomnorm = USGNorm
        F3 us = g;
        if (dot(dir, us) > 0.0f) {  // GotFlipped
            us = {-us.x, -us.y, -us.z};
            g = {-g.x, -g.y, -g.z};
        }
        const F3 norm = i_octahedral_32(octahedral_32(g));
        // GetTangentSpace(norm) — CommonData.cginc:332-343
        const F3 helper = absf(norm.x) > 0.99f ? F3{0.0f, 0.0f, 1.0f} : F3{1.0f, 0.0f, 0.0f};
        const F3 tangent = normalize(cross(norm, helper));
        const F3 binormal = cross(norm, tangent);
        const F3 nd = normalize({om.x * tangent.x + om.y * norm.x + om.z * binormal.x,
                                 om.x * tangent.y + om.y * norm.y + om.z * binormal.y,
                                 om.x * tangent.z + om.y * norm.z + om.z * binormal.z});
        tt_ray_data& O = out_rays[i];
        O.origin[0] = us.x * 0.0001f + pos.x;
        O.origin[1] = us.y * 0.0001f + pos.y;
        O.origin[2] = us.z * 0.0001f + pos.z;
        O.PixelIndex = R.PixelIndex;
        O.direction[0] = nd.x;
        O.direction[1] = nd.y;
        O.direction[2] = nd.z;
        O.last_pdf = pdf;
        for (int k = 0; k < 4; k++) O.hits[k] = R.hits[k];
        survives[i] = 1;
    }
    return TT_OK;
}

}  // extern "C"
