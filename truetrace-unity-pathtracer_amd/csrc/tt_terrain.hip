// tt_terrain.hip — gfx950 heightmap ray march: kernel_heightmap (closest hit) and kernel_shadow_heightmap
// (occlusion) of TrueTrace/Resources/MainCompute/IntersectionKernels.compute:508-710.
//
// Per ray and terrain the reference runs rayBoxIntersection, then sphere-traces a bilinear half-float
// heightmap: a chain of dependent sample -> divide -> sqrt steps whose length ranges from 0 (a box miss) to
// 2,000. One ray per lane; one launch marches one terrain, so its TerrainData sits in the kernel arguments
// (scalar registers) and the API issues the terrains in order, each launch reading the t the previous one
// shortened; the bisection of a ray that starts a step below the surface (:658-677) is a rolled side loop;
// counters exist only in the STATS instantiation; the four taps of a sample are 2-byte loads.
//
// Two forms of the march kernels, with identical results:
//  * grid (the product): one thread per ray, each marching until its own ray is done;
//  * persistent (TT_TERRAIN_FORM=persistent, kept for measurement): the closest-hit kernel's machinery
//    (tt_trace.hip) -- one-wave blocks dequeue 64-ray chunks from the per-XCD segment counters, filter a chunk
//    at full width (record load, box test) into a per-wave candidate list in LDS (ballot + mbcnt compaction)
//    and refill finished lanes in place from it once TT_REFILL_MIN are idle.
// The refill does not pay here (profiles/r08/terrain/bench.json, tools/terrain_bench.py: C2 at 1080p over a
// 1,025^2 terrain; grid vs persistent 0.055 vs 0.18 ms closest hit, 0.18 vs 0.28 ms shadow, and 1.5 vs 1.75 ms
// for an open terrain's long marches): rays of one wave are screen neighbours whose marches are about equally
// long, a triangle hit ends most of them after a few steps, and each refill costs a reload of the ray.
// tt_trace_heightmap_hits: with TerrainArgs::hits_out set, a rewritten record also goes to the contiguous hit
// stream tt_trace_closest_hits filled (ray i of the launch at [i]); both forms share write_hit.
// Numerics: include/truetrace_hip.h; results are bit-identical to host/tt_terrain.cpp. Everything is written
// with plain vector stores.
#include <algorithm>

#include "tt_encode.h"
#include "tt_launch.h"
#include "tt_terrain.h"
#include "tt_traverse.h"

namespace {

using namespace tt_ter;

struct March {
    float ox, oy, oz;  // march origin, terrain-local
    float dx, dy, dz;
    float lim;         // closest hit: bestHit.t; shadow: MaxDist
    float t0, cur, prev;
    uint32_t ri;       // closest hit: index into GlobalRays (ray_offset included); shadow: ray index
    int32_t step;
    bool pos_ok;       // shadow: all(CurrentPos > 0) of the previous sample (:535)
};

// rayBoxIntersection — :513-521
__device__ __forceinline__ bool ray_box(float ox, float oy, float oz, float ix, float iy, float iz, float mnx, float mny,
                                        float mnz, float mxx, float mxy, float mxz, float t_max, float& t0) {
    const float ax = (mnx - ox) * ix, ay = (mny - oy) * iy, az = (mnz - oz) * iz;
    const float bx = (mxx - ox) * ix, by = (mxy - oy) * iy, bz = (mxz - oz) * iz;
    t0 = max_nn(min_nn(ax, bx), max_nn(min_nn(ay, by), max_nn(min_nn(az, bz), 0.025f)));
    const float t1 = min_nn(max_nn(ax, bx), min_nn(max_nn(ay, by), min_nn(max_nn(az, bz), t_max)));
    return t0 <= t1;
}

// GetDist — :604-618 (and the body of the shadow loop, :537-549: the same arithmetic). INSIDE: the caller's
// loop condition established 0 < p.x < dim.x and 0 < p.z < dim.y, so dim > 0, |p| - dim < 0 and q.x, q.z are
// max(0, negative / positive) = +0: the two divisions and their squares drop out of length(q) exactly
// (fmaf(+0, +0, fmaf(qy, qy, +0 * +0)) == qy * qy).
template <bool INSIDE>
__device__ __forceinline__ bool get_dist(const tt_terrain& T, const HeightView& M, float hs2, float px, float py, float pz,
                                         float& u, float& v, float& dist) {
    const float dimx = T.TerrainDim[0], dimz = T.TerrainDim[1];
    u = min1(px / dimx);
    v = min1(pz / dimz);
    float h = height(M, T, u, v);
    h = h * hs2;
    float qy = fabsf(py) - 0.01f;
    qy = qy - h;
    qy = qy * kG;
    const float b2 = qy;
    qy = max0(qy);
    if (INSIDE) {
        dist = sqrtf(qy * qy);
    } else {
        float qx = fabsf(px) - dimx, qz = fabsf(pz) - dimz;
        qx = max0(qx / dimx);
        qz = max0(qz / dimz);
        dist = sqrtf(__builtin_fmaf(qz, qz, __builtin_fmaf(qy, qy, qx * qx)));
    }
    return b2 != fabsf(b2);
}

struct Box {
    float mnx, mny, mnz, mxx, mxy, mxz;
};
template <bool SHADOW>
__device__ __forceinline__ Box terrain_box(const tt_terrain& T) {
    const float px = T.PositionOffset[0], py = T.PositionOffset[1], pz = T.PositionOffset[2];
    const float dimx = T.TerrainDim[0], dimz = T.TerrainDim[1];
    if (SHADOW) return Box{px, py, pz, px + dimx, py + dimx, pz + dimz};                        // :530
    return Box{px + 0.001f, py + 0.001f, pz + 0.001f, (px + dimx) - 0.001f, (py + dimx) - 0.001f,  // :646
               (pz + dimz) - 0.001f};
}

// The filter of one ray: loads what the box test needs and tests it. Returns whether the ray is marched.
// Shadow rays that are alive (t != 0, not occluded by an earlier terrain) but miss this box get their
// visibility record here on the first terrain; marched rays get it when their march ends.
template <bool SHADOW>
__device__ __forceinline__ bool filter_ray(const TerrainArgs& A, const Box& B, uint32_t idx, float& t0) {
    float ox, oy, oz, dx, dy, dz, lim;
    if (SHADOW) {
        const uint4* rp = reinterpret_cast<const uint4*>(A.srays + idx);
        const uint4 r0 = rp[0], r1 = rp[1];
        const float t = __uint_as_float(r1.w);
        if (!(t != 0.0f)) return false;  // :570
        if (A.terrain_index != 0u && A.vis[idx].w != 1.0f) return false;  // an earlier terrain occluded it
        ox = __uint_as_float(r0.x), oy = __uint_as_float(r0.y), oz = __uint_as_float(r0.z);
        dx = __uint_as_float(r1.x), dy = __uint_as_float(r1.y), dz = __uint_as_float(r1.z);
        lim = fabsf(t);
    } else {
        const uint4* rp = reinterpret_cast<const uint4*>(A.rays + A.ray_offset + idx);
        const uint4 r0 = rp[0], r1 = rp[1];
        ox = __uint_as_float(r0.x), oy = __uint_as_float(r0.y), oz = __uint_as_float(r0.z);
        dx = __uint_as_float(r1.x), dy = __uint_as_float(r1.y), dz = __uint_as_float(r1.z);
        lim = __uint_as_float(A.rays[A.ray_offset + idx].hits[2]);  // get(ray_index).t
    }
    const bool pass = ray_box(ox, oy, oz, rcp_rn(dx), rcp_rn(dy), rcp_rn(dz), B.mnx, B.mny, B.mnz, B.mxx, B.mxy, B.mxz,
                              lim, t0);
    if (SHADOW && !pass && A.terrain_index == 0u) A.vis[idx] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    return pass;
}

// A filtered ray takes a lane: :647-652 / :531-534 (the ray is re-read: it was fetched a moment ago).
template <bool SHADOW>
__device__ __forceinline__ void start_march(const TerrainArgs& A, uint32_t idx, float t0, March& m) {
    const float px = A.T.PositionOffset[0], py = A.T.PositionOffset[1], pz = A.T.PositionOffset[2];
    const uint4* rp = SHADOW ? reinterpret_cast<const uint4*>(A.srays + idx)
                             : reinterpret_cast<const uint4*>(A.rays + A.ray_offset + idx);
    const uint4 r0 = rp[0], r1 = rp[1];
    const float ox = __uint_as_float(r0.x), oy = __uint_as_float(r0.y), oz = __uint_as_float(r0.z);
    m.dx = __uint_as_float(r1.x), m.dy = __uint_as_float(r1.y), m.dz = __uint_as_float(r1.z);
    const float s = SHADOW ? t0 + 0.001f : max_nn(t0 + 0.0001f, 0.0f);
    m.ox = (ox + m.dx * s) - px;
    m.oy = (oy + m.dy * s) - py;
    m.oz = (oz + m.dz * s) - pz;
    m.lim = SHADOW ? fabsf(__uint_as_float(r1.w)) : __uint_as_float(A.rays[A.ray_offset + idx].hits[2]);
    m.ri = SHADOW ? idx : A.ray_offset + idx;
    m.t0 = t0;
    m.cur = 0.0f;
    m.prev = 0.0f;
    m.step = 0;
    m.pos_ok = m.ox > 0.0f && m.oy > 0.0f && m.oz > 0.0f;
}

struct Counters {
    uint32_t samples = 0, hits = 0, exhausted = 0;
};

// :679-692: the hit record, the _PrimaryTriangleInfo texel.
template <bool STATS>
__device__ __forceinline__ void write_hit(const TerrainArgs& A, const March& m, float u, float v, Counters& C) {
    tt_ray_data* R = A.rays + m.ri;
    const float t = m.cur + m.t0;
    const uint32_t pix = R->PixelIndex;
    if (A.info && pix < A.n_pixels) {  // (pix % W, pix / W) with pix / W < H is the texel at index pix
        if (A.bounce == 0) {
            reinterpret_cast<uint4*>(A.info)[pix] =
                make_uint4(TT_TERRAIN_MESH_ID, A.terrain_index, __float_as_uint(u), __float_as_uint(v));
        } else if (A.bounce == 1) {
            uint4 o;
            if (!(A.flags & TT_TRACE_USE_RESTIRGI)) {
                o = make_uint4(__float_as_uint(m.dx), __float_as_uint(m.dy), __float_as_uint(m.dz), 1u);
            } else {  // ray2.direction * bestHit.t + ray2.origin
                o = make_uint4(__float_as_uint(m.dx * t + R->origin[0]), __float_as_uint(m.dy * t + R->origin[1]),
                               __float_as_uint(m.dz * t + R->origin[2]), 1u);
            }
            reinterpret_cast<uint4*>(A.info)[pix] = o;
        }
    }
    const uint32_t uv = d3d_f2u(u * 65535.0f) | (d3d_f2u(v * 65535.0f) << 16);  // set(), CommonData.cginc:430-434
    const uint4 rec = make_uint4(TT_TERRAIN_MESH_ID, A.terrain_index, __float_as_uint(t), uv);
    reinterpret_cast<uint4*>(R)[2] = rec;
    if (A.hits_out) A.hits_out[m.ri - A.ray_offset] = rec;  // the contiguous stream tt_trace_closest_hits filled
    if (STATS) {
        unsigned char& seen = A.touched[m.ri - A.ray_offset];
        if (!seen) {
            seen = 1;
            C.hits++;
        }
    }
}

// One iteration of the march loop (:653-698 / :535-555). Returns false once the lane's ray is finished.
template <bool SHADOW, bool STATS>
__device__ __forceinline__ bool march_step(const TerrainArgs& A, const HeightView& M, float hs2, March& m, Counters& C) {
    const tt_terrain& T = A.T;
    const float px = m.ox + m.dx * m.cur, py = m.oy + m.dy * m.cur, pz = m.oz + m.dz * m.cur;
    const bool below_dims = px < T.TerrainDim[0] && py < 1000.0f && pz < T.TerrainDim[1];
    const bool above_zero = px > 0.0f && py > 0.0f && pz > 0.0f;
    const bool go = m.step < TT_TERRAIN_MAX_STEPS && m.cur < m.lim && below_dims && (SHADOW ? m.pos_ok : above_zero);
    if (!go) {
        if (STATS && m.step >= TT_TERRAIN_MAX_STEPS) C.exhausted++;
        if (SHADOW && A.terrain_index == 0u) A.vis[m.ri] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        return false;
    }
    m.step++;
    if (STATS) C.samples++;
    float u, v, dist;
    if (SHADOW) {
        m.pos_ok = above_zero;
        (void)get_dist<false>(T, M, hs2, px, py, pz, u, v, dist);
        if (dist < 0.0001f) {  // :550: occluded; nothing but the visibility record is written
            A.vis[m.ri] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            return false;
        }
        m.cur = m.cur + dist;
        return true;
    }
    const bool throwa = get_dist<true>(T, M, hs2, px, py, pz, u, v, dist);
    if (dist < 0.0001f) {
        if (throwa) {  // :658-677, literally; rare, so rolled
            m.prev = m.prev / 2.0f;
            m.cur = m.cur - m.prev;
#pragma nounroll
            for (int k = 0; k < 10; k++) {
                if (STATS) C.samples++;
                if (get_dist<false>(T, M, hs2, m.ox + m.dx * m.cur, m.oy + m.dy * m.cur, m.oz + m.dz * m.cur, u, v, dist)) {
                    m.prev = m.prev / 2.0f;
                    m.cur = m.cur - m.prev;
                } else {
#pragma nounroll
                    for (int k2 = 0; k2 < 10; k2++) {
                        if (STATS) C.samples++;
                        if (!get_dist<false>(T, M, hs2, m.ox + m.dx * m.cur, m.oy + m.dy * m.cur, m.oz + m.dz * m.cur, u, v,
                                             dist)) {
                            m.prev = m.prev / 2.0f;
                            m.cur = m.cur + m.prev;
                        } else {
                            m.cur = m.cur - m.prev;
                            break;
                        }
                    }
                    break;
                }
            }
        }
        write_hit<STATS>(A, m, u, v, C);
        return false;
    }
    m.prev = dist;
    m.cur = m.cur + dist;
    return true;
}

template <bool STATS>
__device__ __forceinline__ void flush_counters(const TerrainArgs& A, const Counters& C, uint32_t lane) {
    if (!STATS) return;
    // stats slots as the closest-hit kernel: [1] node_visits = samples, [4] hits, [5] reps_exhausted
    const uint32_t s = wave_sum(C.samples), h = wave_sum(C.hits), e = wave_sum(C.exhausted);
    if (lane == 0) {
        if (s) atomicAdd(&A.ctl->stats[1], (unsigned long long)s);
        if (h) atomicAdd(&A.ctl->stats[4], (unsigned long long)h);
        if (e) atomicAdd(&A.ctl->stats[5], (unsigned long long)e);
    }
}

constexpr uint32_t TT_TER_BLOCK = TT_WAVE;  // one wave per persistent block: the scheduler and the list are per wave
constexpr uint32_t TT_TER_CAND = 2 * TT_WAVE;  // candidate list: fewer than 64 kept + at most 64 of a chunk

// The persistent form (measurement only). IND: device-resident ray count.
template <bool SHADOW, bool STATS, bool IND>
__device__ __forceinline__ void terrain_body(const TerrainArgs& A) {
    __shared__ uint2 s_cand[TT_TER_CAND];  // (ray index, asuint(t0)) of filtered rays waiting for a lane
    const uint32_t lane = threadIdx.x & (TT_WAVE - 1);
    const uint32_t wave_id = blockIdx.x;
    SegState S{blockIdx.x % TT_SEGS, 0u, 0u};
    const uint32_t n_rays = IND ? launch_ray_count(A) : A.n_rays;
    const uint32_t n_tiles = (n_rays + 63u) >> 6;
    const HeightView M{A.hmap, A.map_w, A.map_h};
    const Box B = terrain_box<SHADOW>(A.T);
    const float hs2 = A.T.HeightScale * 2.0f;

    uint32_t cand_n = 0, more = 1;
    bool active = false;
    March m{};
    Counters C;
    while (true) {
        const uint64_t idle = __ballot(!active);
        const uint32_t n_idle = (uint32_t)__builtin_popcount((uint32_t)idle) + (uint32_t)__builtin_popcount((uint32_t)(idle >> 32));
        const bool dry = !more && cand_n == 0u;
        if (n_idle == TT_WAVE && dry) break;
        if (n_idle >= TT_REFILL_MIN && !dry) {
            // filter whole chunks until the list can fill the idle lanes (cand_n < n_idle <= 64 before each
            // chunk adds at most 64: the list never exceeds TT_TER_CAND - 1 entries)
            while (cand_n < n_idle && more) {
                uint32_t base = 0;
                const uint32_t count = sched_reserve(A.ctl, n_rays, n_tiles, lane, TT_WAVE, wave_id, S, base);
                if (count == 0u) {
                    more = 0u;
                    break;
                }
                float t0 = 0.0f;
                const bool pass = lane < count && filter_ray<SHADOW>(A, B, base + lane, t0);
                const uint64_t pm = __ballot(pass);
                if (pass) s_cand[cand_n + lane_prefix(pm)] = make_uint2(base + lane, __float_as_uint(t0));
                cand_n += (uint32_t)__popcll(pm);
            }
            __syncthreads();  // (one wave: orders the list's writes before other lanes' reads)
            const uint32_t take = min(cand_n, n_idle);
            const uint32_t rank = lane_prefix(idle);
            if (!active && rank < take) {
                const uint2 e = s_cand[cand_n - 1u - rank];
                start_march<SHADOW>(A, e.x, __uint_as_float(e.y), m);
                active = true;
            }
            cand_n -= take;
            __syncthreads();
        }
        if (active) active = march_step<SHADOW, STATS>(A, M, hs2, m, C);
    }
    flush_counters<STATS>(A, C, lane);
}

// The product form: one thread per ray, each marching until its own ray is done.
constexpr uint32_t TT_TER_GRID_BLOCK = 256;
template <bool SHADOW, bool STATS, bool IND>
__device__ __forceinline__ void terrain_grid_body(const TerrainArgs& A) {
    const uint32_t idx = blockIdx.x * TT_TER_GRID_BLOCK + threadIdx.x;
    const uint32_t n_rays = IND ? launch_ray_count(A) : A.n_rays;
    const HeightView M{A.hmap, A.map_w, A.map_h};
    const Box B = terrain_box<SHADOW>(A.T);
    const float hs2 = A.T.HeightScale * 2.0f;
    Counters C;
    float t0 = 0.0f;
    if (idx < n_rays && filter_ray<SHADOW>(A, B, idx, t0)) {
        March m{};
        start_march<SHADOW>(A, idx, t0, m);
        while (march_step<SHADOW, STATS>(A, M, hs2, m, C)) {
        }
    }
    flush_counters<STATS>(A, C, threadIdx.x & (TT_WAVE - 1));
}

}  // namespace

template <bool SHADOW, bool STATS>
__global__ __launch_bounds__(TT_TER_BLOCK) void tt_terrain_kernel(TerrainArgs A) {
    terrain_body<SHADOW, STATS, false>(A);
}
template <bool SHADOW>
__global__ __launch_bounds__(TT_TER_BLOCK) void tt_terrain_kernel_indirect(TerrainArgs A) {
    terrain_body<SHADOW, false, true>(A);
}
template <bool SHADOW, bool STATS>
__global__ __launch_bounds__(TT_TER_GRID_BLOCK) void tt_terrain_grid_kernel(TerrainArgs A) {
    terrain_grid_body<SHADOW, STATS, false>(A);
}
template <bool SHADOW>
__global__ __launch_bounds__(TT_TER_GRID_BLOCK) void tt_terrain_grid_kernel_indirect(TerrainArgs A) {
    terrain_grid_body<SHADOW, false, true>(A);
}

// ---------------------------------------------------------- :573-591 outputs of kernel_shadow_heightmap
// A streaming pass after the last terrain's march over the launch's rays, driven by the visibility records
// ((1,1,1,1): no terrain occluded the ray): it keeps the encoders' registers out of the march kernel, as
// tt_shadow_accumulate does for the any-hit kernel. Uses ShadowArgs' ray / output / size fields only.
constexpr uint32_t TT_TER_OUT_BLOCK = 256;
__global__ __launch_bounds__(TT_TER_OUT_BLOCK) void tt_terrain_shadow_outputs(ShadowArgs A) {
    const uint32_t ri = blockIdx.x * TT_TER_OUT_BLOCK + threadIdx.x;
    if (ri >= launch_ray_count(A)) return;
    const tt_shadow_ray& R = A.rays[ri];
    const float t = R.t;
    if (!(t != 0.0f)) return;            // :570
    if (A.visibility[ri].w != 1.0f) return;  // occluded
    const uint32_t pix = R.PixelIndex;
    if (pix / A.width >= A.height) return;  // out-of-range UAV writes are dropped
    const bool restir = (A.flags & TT_TRACE_USE_RESTIRGI) != 0;
    const bool rc = (A.flags & TT_SHADOW_RADIANCE_CACHE) != 0;
    const float il[3] = {R.illumination[0], R.illumination[1], R.illumination[2]};
    if (A.bounce == 0 && A.nee_pos) {  // :574
        const float d = fabsf(t);
        A.nee_pos[pix] = make_float4(R.origin[0] + R.direction[0] * d, R.origin[1] + R.direction[1] * d,
                                     R.origin[2] + R.direction[2] * d, 0.0f);
    }
    if (rc && A.cache) {  // :577
        float k[3] = {1.0f, 1.0f, 1.0f};
        if (!(!restir || t >= 0.0f)) {
            const float3 u = tt_enc::unpackRGBE(__float_as_uint(R.LuminanceIncomming));
            k[0] = u.x;
            k[1] = u.y;
            k[2] = u.z;
        }
        uint32_t& ci = A.cache[pix].CurrentIlluminance;
        const float3 d = tt_enc::DecodeRGB(ci);
        ci = tt_enc::EncodeRGB(d.x + il[0] * k[0], d.y + il[1] * k[1], d.z + il[2] * k[2]);
    }
    if (!A.colors) return;
    tt_col_data& C = A.colors[pix];
    if (t >= 0.0f) {  // :579-587
        if (A.bounce == 0) {
            for (int c = 0; c < 3; c++) C.Direct[c] = C.Direct[c] + il[c];
        } else if (!rc) {
            for (int c = 0; c < 3; c++) C.Indirect[c] = C.Indirect[c] + il[c];
        }
    } else if (A.bounce != 0 && restir) {  // :589
        for (int c = 0; c < 3; c++) C.Indirect[c] = C.Indirect[c] + il[c];
    } else {  // :590
        const float3 p = tt_enc::unpackRGBE(C.PrimaryNEERay);
        const float pv[3] = {p.x, p.y, p.z};
        const float inv22 = 1.0f / 2.2f;
        float o[3];
        for (int c = 0; c < 3; c++) o[c] = tt_enc::pow_pinned(pv[c], 2.2f) + tt_enc::pow_pinned(il[c], inv22);
        C.PrimaryNEERay = tt_enc::packRGBE(o[0], o[1], o[2]);
    }
}

// ------------------------------------------------------------------ launchers
template <bool SH, bool ST>
static hipError_t launch_terrain(const TerrainArgs& a, bool grid_form, uint32_t grid, hipStream_t st) {
    if (grid_form) {
        const uint32_t g = (a.n_rays + TT_TER_GRID_BLOCK - 1u) / TT_TER_GRID_BLOCK;
        if constexpr (!ST) {
            if (a.n_rays_dev) {
                hipLaunchKernelGGL((tt_terrain_grid_kernel_indirect<SH>), dim3(g), dim3(TT_TER_GRID_BLOCK), 0, st, a);
                return hipGetLastError();
            }
        }
        hipLaunchKernelGGL((tt_terrain_grid_kernel<SH, ST>), dim3(g), dim3(TT_TER_GRID_BLOCK), 0, st, a);
        return hipGetLastError();
    }
    if constexpr (!ST) {
        if (a.n_rays_dev) {
            hipLaunchKernelGGL((tt_terrain_kernel_indirect<SH>), dim3(grid), dim3(TT_TER_BLOCK), 0, st, a);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((tt_terrain_kernel<SH, ST>), dim3(grid), dim3(TT_TER_BLOCK), 0, st, a);
    return hipGetLastError();
}

// One terrain's march. grid: blocks of the persistent form (ignored by the grid form). stats: closest hit only.
hipError_t tt_launch_terrain(const TerrainArgs* a, int shadow, int stats, int grid_form, uint32_t grid, hipStream_t st) {
    if (a->n_rays == 0) return hipSuccess;
    if (shadow) return launch_terrain<true, false>(*a, grid_form != 0, grid, st);
    return stats ? launch_terrain<false, true>(*a, grid_form != 0, grid, st)
                 : launch_terrain<false, false>(*a, grid_form != 0, grid, st);
}

hipError_t tt_launch_terrain_shadow_outputs(const ShadowArgs* a, hipStream_t st) {
    if (a->n_rays == 0) return hipSuccess;
    hipLaunchKernelGGL(tt_terrain_shadow_outputs, dim3((a->n_rays + TT_TER_OUT_BLOCK - 1) / TT_TER_OUT_BLOCK),
                       dim3(TT_TER_OUT_BLOCK), 0, st, *a);
    return hipGetLastError();
}

// resident blocks per CU of the persistent kernels: [0] closest hit, [1] closest hit with stats, [2] shadow
void tt_terrain_occupancy_table(int* out3) {
    auto occ = [](auto k) {
        int b = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k, TT_TER_BLOCK, 0) != hipSuccess) b = 1;
        return b;
    };
    out3[0] = std::min(occ(tt_terrain_kernel<false, false>), occ(tt_terrain_kernel_indirect<false>));
    out3[1] = occ(tt_terrain_kernel<false, true>);
    out3[2] = std::min(occ(tt_terrain_kernel<true, false>), occ(tt_terrain_kernel_indirect<true>));
}
