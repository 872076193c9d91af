// tt_raygen.hip — the producers either side of the trace dispatch:
//  * tt_generate_kernel: Generate + CreateCameraRay (RayGenKernels.compute:40-57,
//    CommonData.cginc:511-567, UseDoF off) writing RayData into GlobalRays[pixel];
//  * tt_bounce_kernel: the diffuse-lobe subset of kernel_shade's next-ray enqueue
//    (RayTracingShader.compute:52-84, 99-122, 293, 498-506): hit point, unsmoothed normal
//    offset, cosine-hemisphere direction in GetTangentSpace(norm), then compaction of the
//    survivors into the other half of the ping-pong buffer. The reference appends with one
//    InterlockedAdd per ray on one counter (RayTracingShader.compute:500), so its order is
//    whatever the atomics serialise to; one atomic per wave on one word still serialised at
//    ~88 per microsecond (375 us for a 1080p frame, profiles/r02/r02a_kernel_stats.csv). Here
//    the compaction is a STABLE single-pass scan: 4096-ray tiles taken in ticket order, a block
//    ballot/LDS prefix inside the tile and a decoupled look-back over the preceding tiles'
//    published counts (one 64-bit status word per tile, flag and value together), so the
//    survivors land in source order -- deterministic, and the oracle restates the same order.
//    tt_bounce_kernel<true> (TT_ENQUEUE_TERRAIN_BOUNCE on a context with terrains) adds kernel_shade's
//    terrain branch (:109-111, GetHeightmapNormal as both normals) for terrain records; the compaction is
//    the same code, and the plain instantiation keeps its registers (Terrains).
//  * sincos in the cosine-lobe sample is pinned (sincos_pinned): HLSL leaves its precision to
//    the driver, so both sides evaluate the same float polynomials with explicit FMAs.
#include "tt_device.h"
#include "tt_launch.h"
#include "tt_producer.h"

namespace {

// the camera travels in the kernel arguments (no staging copy per frame: a copy is one more small
// operation on the stream that waits for a free CU slot beside the persistent trace grids)
struct CamArgs {
    float c2w[16], ip[16];
};
// one camera ray of pixel (x, y) into *o (RayData, hits = (0, 0, asuint(FarPlane), 0))
__device__ __forceinline__ void generate_one(const CamArgs& cam, uint32_t x, uint32_t y, uint32_t width, uint32_t height,
                                             float near_plane, float far_plane, int32_t jitter, int32_t frames,
                                             int32_t max_bounce, uint4* o) {
    const uint32_t pixel_index = y * width + x;
    float jx = 0.0f, jy = 0.0f;
    if (jitter) {
        const float2 r = random2(0, pixel_index, frames, max_bounce, 0);
        jx = r.x - 0.5f;
        jy = r.y - 0.5f;
    }
    auto C = [&](int r, int c) { return cam.c2w[c * 4 + r]; };
    auto P = [&](int r, int c) { return cam.ip[c * 4 + r]; };
    const float uvx = ((float)x + jx) / (float)width * 2.0f - 1.0f;
    const float uvy = ((float)y + jy) / (float)height * 2.0f - 1.0f;
    const float3 origin = make_float3(C(0, 3), C(1, 3), C(2, 3));
    float3 d = make_float3(fma_(P(0, 1), uvy, P(0, 0) * uvx) + P(0, 3), fma_(P(1, 1), uvy, P(1, 0) * uvx) + P(1, 3),
                           fma_(P(2, 1), uvy, P(2, 0) * uvx) + P(2, 3));
    d = make_float3(fma_(C(0, 2), d.z, fma_(C(0, 1), d.y, C(0, 0) * d.x)),
                    fma_(C(1, 2), d.z, fma_(C(1, 1), d.y, C(1, 0) * d.x)),
                    fma_(C(2, 2), d.z, fma_(C(2, 1), d.y, C(2, 0) * d.x)));
    d = normalize3(d);
    o[0] = make_uint4(__float_as_uint(origin.x + near_plane * d.x), __float_as_uint(origin.y + near_plane * d.y),
                      __float_as_uint(origin.z + near_plane * d.z), pixel_index);
    o[1] = make_uint4(__float_as_uint(d.x), __float_as_uint(d.y), __float_as_uint(d.z), 0u);
    o[2] = make_uint4(0u, 0u, __float_as_uint(far_plane), 0u);
}

__global__ __launch_bounds__(256) void tt_generate_kernel(const CamArgs cam,
                                                          uint32_t width, uint32_t height, float near_plane,
                                                          float far_plane, int32_t jitter, int32_t frames,
                                                          int32_t max_bounce, tt_ray_data* __restrict__ rays) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= width || y >= height) return;
    generate_one(cam, x, y, width, height, near_plane, far_plane, jitter, frames, max_bounce,
                 reinterpret_cast<uint4*>(rays + y * width + x));
}

// The rays of a pixel list (a multi-GPU group member's screen tiles, tt_group_trace_frame) for `batch` frames:
// ray b n + i is pixel pixels[i]'s camera ray of frame b (frames_accumulated = frames + b), bit for bit the one
// tt_generate_kernel writes at GlobalRays[pixel] for that frame, with PixelIndex + b W H (frame b of a screen
// `batch` frames tall, tt_ctx_set_frame_pixels).
__global__ __launch_bounds__(256) void tt_generate_list_kernel(const CamArgs cam, const uint32_t* __restrict__ pixels,
                                                               uint32_t n, uint32_t batch, uint32_t width,
                                                               uint32_t height, float near_plane, float far_plane,
                                                               int32_t jitter, int32_t frames, int32_t max_bounce,
                                                               tt_ray_data* __restrict__ rays) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n * batch) return;
    const uint32_t b = r / n, p = pixels[r - b * n];
    uint4* o = reinterpret_cast<uint4*>(rays + r);
    generate_one(cam, p % width, p / width, width, height, near_plane, far_plane, jitter, frames + (int32_t)b,
                 max_bounce, o);
    if (b) o[0].w = p + b * width * height;
}

// sin/cos of the disc-sample angle phi in [-3pi/4, 3pi/4] (sample_disc's two branches give
// [-pi/4, pi/4] and [pi/4, 3pi/4]): cephes single-precision minimax polynomials on
// [-pi/4, pi/4] evaluated with explicit FMAs; |phi| > pi/4 is reduced by pi/2 (two-constant
// Cody-Waite). Pinned: oracle/tt_oracle.c sincos_pinned is the same sequence of operations.
__device__ __forceinline__ void sincos_pinned(float phi, float* s, float* c) {
    const bool big = fabsf(phi) > 0.785398185253143310546875f;
    const float q = phi > 0.0f ? 1.0f : -1.0f;
    const float r = big ? fma_(-q, -4.37113882867379e-8f, fma_(-q, 1.57079637050628662109375f, phi)) : phi;
    const float z = r * r;
    const float sp = fma_(fma_(fma_(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f) * z, r, r);
    const float cp = fma_(fma_(fma_(fma_(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), z,
                               -0.5f), z, 1.0f);
    // phi = q pi/2 + r: sin(phi) = q cos(r), cos(phi) = -q sin(r)
    *s = big ? q * cp : sp;
    *c = big ? -q * sp : cp;
}

// pdf > 0 decision and omega_o of sample(): cosine-weighted hemisphere from random(1, pixel)
// (RayTracingShader.compute:52-84)
__device__ __forceinline__ float3 cosine_sample(uint32_t pixel, int32_t frames, int32_t max_bounce, int32_t cur_bounce,
                                                float* pdf) {
    const float2 rnd = random2(1, pixel, frames, max_bounce, cur_bounce);
    float a = 2.0f * rnd.x - 1.0f, b = 2.0f * rnd.y - 1.0f;
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
    sincos_pinned(phi, &sp, &cp);
    const float dx = rr * cp, dz = rr * sp;
    const float3 om = make_float3(dx, sqrtf(fabsf(1.0f - (dx * dx + dz * dz))), dz);
    *pdf = om.y * 0.318309886548f;
    return om;
}

// The new ray of a surviving hit (kernel_shade's diffuse path, RayTracingShader.compute:99-122,
// 284, 293, 503); the hit's frame is tt_producer.h's.
template <bool TERRAIN>
__device__ __forceinline__ void bounce_ray(const Ray3& R, float3 om, float pdf, const tt_cuda_triangle* tris,
                                           const tt_mesh_data* md, const TerrainSet& ter, uint4* o) {
    const HitFrame H = hit_frame<TERRAIN>(R, tris, md, ter);
    const float3 pos = H.pos, g = H.g, us = H.us;
    const float3 norm = i_octahedral_32(octahedral_32(g));
    // GetTangentSpace(norm) — CommonData.cginc:332-343 (helper (1,0,0), or (0,0,1) if |n.x| > 0.99)
    const float3 helper = fabsf(norm.x) > 0.99f ? make_float3(0, 0, 1) : make_float3(1, 0, 0);
    const float3 tangent = normalize3(cross3(norm, helper));
    const float3 binormal = cross3(norm, tangent);
    float3 nd = make_float3(om.x * tangent.x + om.y * norm.x + om.z * binormal.x,
                            om.x * tangent.y + om.y * norm.y + om.z * binormal.y,
                            om.x * tangent.z + om.y * norm.z + om.z * binormal.z);
    nd = normalize3(nd);
    o[0] = make_uint4(__float_as_uint(us.x * 0.0001f + pos.x), __float_as_uint(us.y * 0.0001f + pos.y),
                      __float_as_uint(us.z * 0.0001f + pos.z), R.a.w);
    o[1] = make_uint4(__float_as_uint(nd.x), __float_as_uint(nd.y), __float_as_uint(nd.z), __float_as_uint(pdf));
    o[2] = R.h;
}

constexpr uint32_t TT_BOUNCE_K = 4;                          // rays per thread
constexpr uint32_t TT_BOUNCE_BLOCK = 1024;                   // threads per tile (16 waves)
constexpr uint32_t TT_BOUNCE_WAVES = TT_BOUNCE_BLOCK / 64;
constexpr uint32_t TT_BOUNCE_TILE = TT_BOUNCE_BLOCK * TT_BOUNCE_K;  // 4096 rays per tile: few tickets, short look-backs

// TERRAIN (TT_ENQUEUE_TERRAIN_BOUNCE on a context with terrains): a terrain record with triangle_id < ter.n
// survives under the triangle rule and takes bounce_ray's terrain branch; a separate instantiation, so the plain
// kernel keeps its code and registers. `terrains` (plain form): terrain records end their paths.
template <bool TERRAIN>
__global__ __launch_bounds__(TT_BOUNCE_BLOCK) void tt_bounce_kernel(tt_ray_data* __restrict__ rays, uint32_t src_off, uint32_t dst_off,
                                                        uint32_t n, float far_plane, int32_t cur_bounce, int32_t frames,
                                                        int32_t max_bounce, const tt_cuda_triangle* __restrict__ tris,
                                                        const tt_mesh_data* __restrict__ md, uint32_t* __restrict__ ctl,
                                                        unsigned long long* __restrict__ lb, uint32_t n_tiles,
                                                        const uint32_t* __restrict__ n_dev, uint32_t* __restrict__ n_next_dev,
                                                        uint32_t* __restrict__ ctl_next, uint32_t ctl_next_words,
                                                        uint32_t frame_pixels, uint32_t terrains, const TerrainSet ter) {
    __shared__ uint32_t s_tile, s_prefix;
    __shared__ uint32_t s_cnt[TT_BOUNCE_K][TT_BOUNCE_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // the next enqueue on this stream uses the other counter block: zero it now (plain vector stores; it
    // starts after this launch completes), so no fill kernel runs between enqueues
    if (ctl_next)
        for (uint32_t w = blockIdx.x * TT_BOUNCE_BLOCK + tid; w < ctl_next_words; w += gridDim.x * TT_BOUNCE_BLOCK)
            ctl_next[w] = 0u;
    if (tid == 0) s_tile = atomicAdd(&ctl[1], 1u);  // tiles in ticket order: look-back never waits on an unstarted block
    __syncthreads();
    const uint32_t tile = s_tile;
    const uint32_t base = tile * TT_BOUNCE_TILE;
    // device-resident count (the reference's BufferSizes[CurBounce].tracerays): tiles past it find no
    // rays, publish 0 and keep the look-back chain complete up to the grid's last tile
    if (n_dev) n = min(*n_dev, n);
    // pass 1: which rays survive (hit, and the cosine sample's pdf > 0); keep the ray and omega_o
    Ray3 R[TT_BOUNCE_K];
    float3 om[TT_BOUNCE_K];
    float pdf[TT_BOUNCE_K];
    uint64_t live[TT_BOUNCE_K];
#pragma unroll
    for (uint32_t k = 0; k < TT_BOUNCE_K; k++) {
        const uint32_t i = base + k * TT_BOUNCE_BLOCK + tid;
        bool ok = false;
        if (i < n) {
            const uint4* rp = reinterpret_cast<const uint4*>(rays + src_off + i);
            R[k].a = rp[0];
            R[k].b = rp[1];
            R[k].h = rp[2];
            const float t = __uint_as_float(R[k].h.z);
            // (on a context with terrains a terrain hit ends its path: its record indexes no _MeshData)
            const bool hit = TERRAIN ? (terrain_record(R[k].h) ? R[k].h.y < ter.n : (int32_t)R[k].h.y >= 0)
                                     : (int32_t)R[k].h.y >= 0 && !(terrains && R[k].h.x == TT_TERRAIN_MESH_ID);
            if (t < far_plane && hit) {
                // batched frames (tt_ctx_set_frame_pixels): PixelIndex p is pixel p mod n of frame p / n, whose
                // random numbers are that pixel's at frames + p / n; 0: PixelIndex as-is (the reference's form)
                uint32_t px = R[k].a.w;
                int32_t fr = frames;
                if (frame_pixels) {
                    const uint32_t j = px / frame_pixels;
                    px -= j * frame_pixels;
                    fr += (int32_t)j;
                }
                om[k] = cosine_sample(px, fr, max_bounce, cur_bounce, &pdf[k]);
                ok = pdf[k] > 0.0f;
            }
        }
        live[k] = __ballot(ok);
        if (lane == 0) s_cnt[k][wave] = (uint32_t)__popcll(live[k]);
    }
    __syncthreads();
    // tile count, published before the look-back so successors can sum past this tile
    if (wave == 0) {
        uint32_t total = 0;
#pragma unroll
        for (uint32_t k = 0; k < TT_BOUNCE_K; k++)
            for (uint32_t w = 0; w < TT_BOUNCE_WAVES; w++) total += s_cnt[k][w];
        uint32_t prefix = 0;
        if (tile == 0) {
            if (lane == 0) lb_publish(lb, 0, TT_LB_INC, total);
        } else {
            if (lane == 0) lb_publish(lb, tile, TT_LB_AGG, total);
            prefix = lb_lookback(lb, tile, lane);
            if (lane == 0) lb_publish(lb, tile, TT_LB_INC, prefix + total);
        }
        if (lane == 0) {
            s_prefix = prefix;
            if (tile == n_tiles - 1u) {
                ctl[0] = prefix + total;  // the survivor count tt_enqueue returns
                if (n_next_dev) *n_next_dev = prefix + total;  // BufferSizes[CurBounce + 1].tracerays
            }
        }
    }
    __syncthreads();
    // pass 2: survivors in source order (k-major, then thread) at prefix + rank
    uint32_t slot = s_prefix;
#pragma unroll
    for (uint32_t k = 0; k < TT_BOUNCE_K; k++) {
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < TT_BOUNCE_WAVES; w++) {
            before += w < wave ? s_cnt[k][w] : 0u;
            all += s_cnt[k][w];
        }
        if ((live[k] >> lane) & 1ull) {
            const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(live[k] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)live[k], 0u));
            bounce_ray<TERRAIN>(R[k], om[k], pdf[k], tris, md, ter, reinterpret_cast<uint4*>(rays + dst_off + slot + before + pre));
        }
        slot += all;
    }
}

}  // namespace

// c2w, ip: HOST arrays (column-major 4x4 each), copied into the kernel arguments
hipError_t tt_launch_generate(const float* c2w, const float* ip, uint32_t w, uint32_t h, float near_plane, float far_plane,
                              int32_t jitter, int32_t frames, int32_t max_bounce, tt_ray_data* rays, hipStream_t st) {
    CamArgs cam;
    for (int i = 0; i < 16; i++) {
        cam.c2w[i] = c2w[i];
        cam.ip[i] = ip[i];
    }
    hipLaunchKernelGGL(tt_generate_kernel, dim3((w + 255u) / 256u, h), dim3(256), 0, st, cam, w, h, near_plane, far_plane,
                       jitter, frames, max_bounce, rays);
    return hipGetLastError();
}

// pixels: DEVICE array of n pixel indices < w * h (the caller checked them)
hipError_t tt_launch_generate_list(const float* c2w, const float* ip, const uint32_t* pixels, uint32_t n,
                                   uint32_t batch, uint32_t w, uint32_t h, float near_plane, float far_plane,
                                   int32_t jitter, int32_t frames, int32_t max_bounce, tt_ray_data* rays,
                                   hipStream_t st) {
    if (n == 0 || batch == 0) return hipSuccess;
    CamArgs cam;
    for (int i = 0; i < 16; i++) {
        cam.c2w[i] = c2w[i];
        cam.ip[i] = ip[i];
    }
    hipLaunchKernelGGL(tt_generate_list_kernel, dim3((n * batch + 255u) / 256u), dim3(256), 0, st, cam, pixels, n,
                       batch, w, h, near_plane, far_plane, jitter, frames, max_bounce, rays);
    return hipGetLastError();
}

uint32_t tt_bounce_tiles(uint32_t n) { return (n + TT_BOUNCE_TILE - 1u) / TT_BOUNCE_TILE; }

// counter: [0] survivor count, [1] tile ticket, then tt_bounce_tiles(n) 64-bit status words; all
// zero at the launch (the caller's fill, or the previous launch's ctl_next). ctl_next (nullable): the
// ctl_next_words words this launch zeroes for the next one.
// n_dev (nullable): device-resident ray count, clamped to n (then n is the capacity the grid covers);
// n_next_dev (nullable): receives the survivor count on the device.
// terrains: the context has a terrain set (terrain records end their paths), unless ter / n_ter / hmap are passed
// too (TT_ENQUEUE_TERRAIN_BOUNCE): then the TERRAIN instantiation runs and such rays bounce off the terrain.
hipError_t tt_launch_bounce(tt_ray_data* rays, uint32_t src_off, uint32_t dst_off, uint32_t n, float far_plane,
                            int32_t cur_bounce, int32_t frames, int32_t max_bounce, const tt_cuda_triangle* tris,
                            const tt_mesh_data* md, uint32_t* counter, hipStream_t st, const uint32_t* n_dev,
                            uint32_t* n_next_dev, uint32_t* ctl_next, uint32_t ctl_next_words,
                            uint32_t frame_pixels, uint32_t terrains, const tt_terrain* ter, uint32_t n_ter,
                            const uint16_t* hmap, uint32_t hmap_w, uint32_t hmap_h) {
    if (n == 0) {
        if (ctl_next) {  // (this block stays zero: the next launch's block is the caller's to fill)
            const hipError_t e = hipMemsetAsync(ctl_next, 0, 4 * (size_t)ctl_next_words, st);
            if (e != hipSuccess) return e;
        }
        if (n_next_dev) return hipMemsetAsync(n_next_dev, 0, 4, st);
        return hipSuccess;
    }
    const uint32_t tiles = tt_bounce_tiles(n);
    const bool bounce_off = ter && n_ter && hmap;
    const TerrainSet set = bounce_off ? TerrainSet{ter, n_ter, tt_ter::HeightView{hmap, hmap_w, hmap_h}} : TerrainSet{};
    hipLaunchKernelGGL(bounce_off ? tt_bounce_kernel<true> : tt_bounce_kernel<false>, dim3(tiles), dim3(TT_BOUNCE_BLOCK), 0,
                       st, rays, src_off, dst_off, n, far_plane, cur_bounce, frames, max_bounce, tris, md, counter,
                       reinterpret_cast<unsigned long long*>(counter + 4), tiles, n_dev, n_next_dev, ctl_next,
                       ctl_next_words, frame_pixels, terrains, set);
    return hipGetLastError();
}
