// tt_lights.hip — the scene's lights and the NEE emit (include/truetrace_hip.h, "lights"):
//  * tt_lights_validate / tt_scene_upload_lights / tt_scene_update_light_nodes: LightNodes, LightTriangles and
//    _LightMeshes live with the scene's device buffers (SceneDev), checked on the host first
//    (tt_lights_check_host.h): the kernel below indexes them without bounds checks;
//  * tt_lights_refit: the host side of the per-frame refit (the plan of tt_light_refit_plan_host.h, the call's
//    checks and block table); its two launches are tt_light_refit.hip. tt_scene_read_light_nodes / _tris;
//  * tt_nee_kernel: one lane per traced ray. The hit's frame is the enqueue's own device code (tt_producer.h);
//    SampleLightBVH, Importance and the emitted record are tt_lights_core.h, the text the host reference builds
//    too. Per descent step a lane fetches its two children as one 80-byte block (five 128-bit loads) and carries
//    the chosen child's `left`, hashes twice for random(264 + Reps), and evaluates Importance twice (about twenty
//    sqrt / divide operations). The TLAS -> mesh-tree transition inverts W2L per lane (no per-mesh cache: see
//    DESIGN.md, Lights). The loop is bounded by TT_LIGHT_MAX_REPS and, on validated lights, ends earlier: every
//    step moves to a larger node index.
//  * Survivors are compacted in source order by the enqueue's scheme: 256-ray tiles taken in ticket order, a
//    ballot / LDS prefix inside the tile, the decoupled look-back over the preceding tiles. LDS holds only that.
#include "tt_call_host.h"
#include "tt_ctx.h"
#include "tt_light_refit.h"
#include "tt_light_refit_plan_host.h"
#include "tt_lights_check_host.h"
#include "tt_lights_core.h"
#include "tt_producer.h"

namespace {

constexpr uint32_t TT_NEE_BLOCK = 256;  // one ray per thread, one tile per block
constexpr uint32_t TT_NEE_WAVES = TT_NEE_BLOCK / 64;

struct NeeArgs {
    const tt_ray_data* rays;  // at the launch's first ray
    uint32_t n;
    float far_plane;
    int32_t cur_bounce, frames, max_bounce;
    tt_lt::Scene S;
    uint32_t n_mesh, n_tris;
    uint32_t frame_pixels, terrains, negative_t;
    tt_light_sample* samples;
    tt_shadow_ray* out;
    uint32_t* ctl;             // [0] survivor count, [1] tile ticket; zero at the launch
    unsigned long long* lb;    // one look-back word per tile; zero at the launch
    uint32_t n_tiles;
    const uint32_t* n_dev;
    uint32_t* n_out_dev;
};

__device__ __forceinline__ tt_lt::V3 v3(float3 a) { return tt_lt::V3{a.x, a.y, a.z}; }

__global__ __launch_bounds__(TT_NEE_BLOCK) void tt_nee_kernel(const NeeArgs a) {
    __shared__ uint32_t s_tile, s_prefix;
    __shared__ uint32_t s_cnt[TT_NEE_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) s_tile = atomicAdd(&a.ctl[1], 1u);  // tiles in ticket order: look-back never waits on an unstarted block
    __syncthreads();
    const uint32_t tile = s_tile;
    const uint32_t i = tile * TT_NEE_BLOCK + tid;
    const uint32_t n = a.n_dev ? min(*a.n_dev, a.n) : a.n;
    bool ok = false;
    tt_shadow_ray ray;
    if (i < n) {
        const uint4* rp = reinterpret_cast<const uint4*>(a.rays + i);
        Ray3 R;
        R.a = rp[0];
        R.b = rp[1];
        R.h = rp[2];
        tt_light_sample smp;
        const uint32_t hits[4] = {R.h.x, R.h.y, R.h.z, R.h.w};
        // (a record whose mesh or triangle index is past the scene's is not a hit: nothing is indexed with it)
        if (tt_lt::is_hit(hits, a.far_plane, a.terrains != 0u) && R.h.x < a.n_mesh && R.h.y < a.n_tris) {
            const HitFrame H = hit_frame<false>(R, a.S.tris, a.S.md, TerrainSet{});
            const float3 norm = i_octahedral_32(octahedral_32(H.g));
            const float3 origin = make_float3(H.us.x * 0.0001f + H.pos.x, H.us.y * 0.0001f + H.pos.y, H.us.z * 0.0001f + H.pos.z);
            const tt_lt::Rng rng = tt_lt::make_rng(R.a.w, a.frame_pixels, a.frames, a.max_bounce, a.cur_bounce);
            ok = tt_lt::emit_one(a.S, v3(H.pos), v3(norm), v3(origin), rng, R.a.w, a.negative_t != 0u, smp, ray);
        } else {
            tt_lt::miss_sample(smp);
        }
        if (a.samples) {
            uint4* sp = reinterpret_cast<uint4*>(a.samples + i);
            uint4 w[3];
            __builtin_memcpy(w, &smp, 48);
            sp[0] = w[0];
            sp[1] = w[1];
            sp[2] = w[2];
        }
    }
    const uint64_t live = __ballot(ok);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(live);
    __syncthreads();
    if (wave == 0) {
        uint32_t total = 0;
#pragma unroll
        for (uint32_t w = 0; w < TT_NEE_WAVES; w++) total += s_cnt[w];
        uint32_t prefix = 0;
        if (tile == 0) {
            if (lane == 0) lb_publish(a.lb, 0, TT_LB_INC, total);
        } else {
            if (lane == 0) lb_publish(a.lb, tile, TT_LB_AGG, total);
            prefix = lb_lookback(a.lb, tile, lane);
            if (lane == 0) lb_publish(a.lb, tile, TT_LB_INC, prefix + total);
        }
        if (lane == 0) {
            s_prefix = prefix;
            if (tile == a.n_tiles - 1u) {
                a.ctl[0] = prefix + total;
                if (a.n_out_dev) *a.n_out_dev = prefix + total;  // BufferSizes[CurBounce].shadow_rays
            }
        }
    }
    __syncthreads();
    if (ok && a.out) {
        uint32_t before = 0;
#pragma unroll
        for (uint32_t w = 0; w < TT_NEE_WAVES; w++) before += w < wave ? s_cnt[w] : 0u;
        const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(live >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)live, 0u));
        uint4* op = reinterpret_cast<uint4*>(a.out + s_prefix + before + pre);
        uint4 w[3];
        __builtin_memcpy(w, &ray, 48);
        op[0] = w[0];
        op[1] = w[1];
        op[2] = w[2];
    }
}

uint32_t nee_tiles(uint32_t n) { return (n + TT_NEE_BLOCK - 1u) / TT_NEE_BLOCK; }

tt_status refused(tt_ctx* c, const tt_call::Refusal& r) { return fail(c, r.status, "%s", r.text); }

tt_lcheck::Lights host_lights(const SceneDev& d) {
    return tt_lcheck::Lights{d.lnodes_host.data(), (uint32_t)d.lnodes_host.size(), d.ltris_host.data(),
                             (uint32_t)d.ltris_host.size(), d.lmeshes_host.data(), (uint32_t)d.lmeshes_host.size()};
}

// n_dev (nullable): device-resident count of the traced rays; n_out_dev (nullable): the survivor count goes there
// on the device and the call returns without synchronizing.
tt_status emit_call(tt_ctx* c, const tt_trace_params* p, const uint32_t* n_dev, const tt_ray_data* rays, int32_t frames,
                    int32_t max_bounce, tt_light_sample* samples, tt_shadow_ray* shadow, uint32_t* n_shadow,
                    uint32_t* n_out_dev) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    if (c->ovl || c->group_member)
        return fail(c, TT_ERR_UNSUPPORTED, "tt_emit_nee: frame slots (tt_ctx_share_blas) and group members carry no lights");
    if (c->scene.n_lnodes == 0) return fail(c, TT_ERR_NO_SCENE, "no lights uploaded (tt_scene_upload_lights)");
    const bool have_args = p && rays;
    const tt_call::EnqueuePlan pl =
        tt_call::check_enqueue(have_args, have_args ? tt_call::common_of(*p) : tt_call::Common{}, n_dev || n_out_dev);
    if (pl.refusal) return refused(c, pl.refusal);
    if (p->bounce < 0) return fail(c, TT_ERR_INVALID_ARG, "negative bounce");
    const bool dev = pl.dev;
    const bool async = dev && ((p->flags & TT_TRACE_ASYNC) || n_out_dev);
    if (!async && !n_shadow) return fail(c, TT_ERR_INVALID_ARG, "null survivor count");
    if ((n_dev && !is_device_ptr(n_dev)) || (n_out_dev && !is_device_ptr(n_out_dev)))
        return fail(c, TT_ERR_INVALID_ARG, "a ray count pointer is not device memory");
    if (dev && (!is_device_ptr(rays) || (samples && !is_device_ptr(samples)) || (shadow && !is_device_ptr(shadow))))
        return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but rays / samples / shadow rays are not device memory");
    if (dev && (((uintptr_t)rays | (uintptr_t)samples | (uintptr_t)shadow) % 16))
        return fail(c, TT_ERR_INVALID_ARG, "GlobalRays / samples / shadow rays must be 16-byte aligned");
    TT_HIP(c, hipSetDevice(c->device));
    if (p->n_rays == 0) {
        if (n_out_dev) TT_HIP(c, hipMemsetAsync(n_out_dev, 0, 4, c->stream));
        if (n_shadow) *n_shadow = 0;
        return TT_OK;
    }
    const uint32_t tiles = nee_tiles(p->n_rays);
    const size_t ctl_words = 4 + 2 * (size_t)tiles;
    if (c->nee_ctl.n < ctl_words) {
        TT_HIP(c, hipStreamSynchronize(c->stream));  // (the old block may be in use)
        TT_HIP(c, c->nee_ctl.alloc(ctl_words));
    }
    TT_HIP(c, hipMemsetAsync(c->nee_ctl.p, 0, 4 * ctl_words, c->stream));
    NeeArgs a{};
    if (dev) {
        a.rays = rays + pl.src;
        a.samples = samples;
        a.out = shadow;
    } else {
        const tt_ray_data* d;
        TT_HIP(c, stage_in(c, c->st_rays, rays, p->n_rays, pl.src, d));
        a.rays = d + pl.src;
        if (samples) TT_HIP(c, stage_in(c, c->st_samples, nullptr, p->n_rays, 0, a.samples));
        if (shadow) TT_HIP(c, stage_in(c, c->st_shadow, nullptr, p->n_rays, 0, a.out));
    }
    const SceneDev& sd = c->scene;
    a.n = p->n_rays;
    a.far_plane = p->far_plane;
    a.cur_bounce = p->bounce;
    a.frames = frames;
    a.max_bounce = max_bounce;
    a.S = tt_lt::Scene{sd.lnodes.p, sd.ltris.p, sd.lmeshes.p, sd.tris_raw.p, sd.mesh_raw.p};
    a.n_mesh = (uint32_t)sd.mesh_raw.n;
    a.n_tris = (uint32_t)sd.tris_raw.n;
    a.frame_pixels = c->frame_pixels;
    a.terrains = sd.terrains_host.empty() ? 0u : 1u;
    a.negative_t = (p->flags & TT_NEE_NEGATIVE_T) ? 1u : 0u;
    a.ctl = c->nee_ctl.p;
    a.lb = reinterpret_cast<unsigned long long*>(c->nee_ctl.p + 4);
    a.n_tiles = tiles;
    a.n_dev = n_dev;
    a.n_out_dev = n_out_dev;
    uint32_t slot;
    SceneRead sr(c);
    TT_HIP(c, sr.err);
    TT_HIP(c, ring_open(c, c->timing, slot));
    hipLaunchKernelGGL(tt_nee_kernel, dim3(tiles), dim3(TT_NEE_BLOCK), 0, c->stream, a);
    TT_HIP(c, hipGetLastError());
    note_stream_launch(c->stream);
    TT_HIP(c, ring_close(c, c->timing, slot));
    sr.end();
    if (async) return TT_OK;
    uint32_t cnt = 0;
    TT_HIP(c, hipMemcpyAsync(&cnt, c->nee_ctl.p, 4, hipMemcpyDeviceToHost, c->stream));
    TT_HIP(c, hipStreamSynchronize(c->stream));
    if (!dev) {
        if (samples) TT_HIP(c, hipMemcpy(samples, a.samples, sizeof(tt_light_sample) * p->n_rays, hipMemcpyDeviceToHost));
        if (shadow && cnt) TT_HIP(c, hipMemcpy(shadow, a.out, sizeof(tt_shadow_ray) * cnt, hipMemcpyDeviceToHost));
    }
    *n_shadow = cnt;
    return TT_OK;
}

}  // namespace

void tt_ctx_mark_group_member(tt_ctx* c) { c->group_member = true; }

extern "C" {

tt_status tt_lights_validate(const tt_light_node* nodes, uint32_t n_nodes, const tt_light_tri* tris, uint32_t n_tris,
                             const tt_light_mesh* meshes, uint32_t n_meshes, const tt_mesh_data* meshdata,
                             uint32_t n_mesh, uint32_t n_scene_tris, char* why, uint32_t why_len) {
    std::string w;
    const tt_status st = tt_lcheck::validate(tt_lcheck::Lights{nodes, n_nodes, tris, n_tris, meshes, n_meshes}, meshdata,
                                             n_mesh, n_scene_tris, w);
    copy_why(w, why, why_len);
    return st;
}

tt_status tt_scene_upload_lights(tt_ctx* c, const tt_light_node* nodes, uint32_t n_nodes, const tt_light_tri* tris,
                                 uint32_t n_tris, const tt_light_mesh* meshes, uint32_t n_meshes) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    if (c->group_member) return fail(c, TT_ERR_UNSUPPORTED, "tt_scene_upload_lights: group members carry no lights");
    TT_REFUSE_BORROWER(c);
    TT_REFUSE_LENDER(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "tt_scene_upload_lights: no scene uploaded");
    std::string why;
    const tt_status vs = tt_lcheck::validate(tt_lcheck::Lights{nodes, n_nodes, tris, n_tris, meshes, n_meshes},
                                             c->host.mesh.data(), (uint32_t)c->host.mesh.size(), c->host.n_tris, why);
    if (vs != TT_OK) return fail(c, vs, "light validation failed: %s", why.c_str());
    TT_HIP(c, hipSetDevice(c->device));
    TT_HIP(c, hipStreamSynchronize(c->stream));  // nothing still reads the lights being replaced
    SceneDev& d = c->scene;
    d.release_lights();
    hipError_t e;
    if ((e = d.lnodes.alloc(n_nodes)) != hipSuccess || (e = d.ltris.alloc(n_tris)) != hipSuccess ||
        (e = d.lmeshes.alloc(n_meshes)) != hipSuccess) {
        d.release_lights();
        return hip_fail(c, e, "light allocation");
    }
    TT_HIP(c, hipMemcpy(d.lnodes.p, nodes, sizeof(tt_light_node) * n_nodes, hipMemcpyHostToDevice));
    TT_HIP(c, hipMemcpy(d.ltris.p, tris, sizeof(tt_light_tri) * n_tris, hipMemcpyHostToDevice));
    TT_HIP(c, hipMemcpy(d.lmeshes.p, meshes, sizeof(tt_light_mesh) * n_meshes, hipMemcpyHostToDevice));
    d.lnodes_host.assign(nodes, nodes + n_nodes);
    d.ltris_host.assign(tris, tris + n_tris);
    d.lmeshes_host.assign(meshes, meshes + n_meshes);
    d.n_lnodes = n_nodes;
    tt_lplan::build(host_lights(d), c->host.mesh.data(), d.lrefit.plan);  // (its device arrays: the first refit's)
    d.lrefit.plan_valid = true;
    return TT_OK;
}

tt_status tt_scene_update_light_nodes(tt_ctx* c, uint32_t first, uint32_t count, const tt_light_node* nodes) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER(c);
    if (!c->has_scene || c->scene.n_lnodes == 0) return fail(c, TT_ERR_NO_SCENE, "tt_scene_update_light_nodes: no lights uploaded");
    SceneDev& d = c->scene;
    if (!nodes || (uint64_t)first + count > d.n_lnodes)
        return fail(c, TT_ERR_INVALID_ARG, "light node update range [%u, %llu) outside the %u light nodes", first,
                    (unsigned long long)first + count, d.n_lnodes);
    if (count == 0) return TT_OK;
    std::vector<tt_light_node> next = d.lnodes_host;
    std::copy(nodes, nodes + count, next.begin() + first);
    std::string why;
    tt_lcheck::Lights L = host_lights(d);
    L.nodes = next.data();
    const tt_status vs = tt_lcheck::validate(L, c->host.mesh.data(), (uint32_t)c->host.mesh.size(), c->host.n_tris, why);
    if (vs != TT_OK) return fail(c, vs, "light validation failed: %s", why.c_str());
    TT_HIP(c, hipSetDevice(c->device));
    SceneWrite w(c, false);
    TT_HIP(c, w.err);
    void* pin;
    TT_HIP(c, stage_begin(c, nodes, sizeof(tt_light_node) * count, pin));
    TT_HIP(c, hipMemcpyAsync(d.lnodes.p + first, pin, sizeof(tt_light_node) * count, hipMemcpyHostToDevice, c->stream));
    TT_HIP(c, stage_end(c));
    TT_HIP(c, w.end());
    // a changed `left` changes what the refit climbs: its plan is rebuilt by the next tt_lights_refit
    if (!tt_lplan::same_structure(next.data() + first, d.lnodes_host.data() + first, count)) d.lrefit.plan_valid = false;
    d.lnodes_host.swap(next);
    return TT_OK;
}

tt_status tt_lights_refit(tt_ctx* c, const uint32_t* mesh_indices, uint32_t n_mesh_indices, const tt_light_transform* transforms,
                          uint32_t n_transforms, uint32_t flags) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    if (c->ovl || c->group_member)
        return fail(c, TT_ERR_UNSUPPORTED, "tt_lights_refit: frame slots (tt_ctx_share_blas) and group members carry no lights");
    TT_REFUSE_BORROWER(c);
    if (!c->has_scene || c->scene.n_lnodes == 0) return fail(c, TT_ERR_NO_SCENE, "tt_lights_refit: no lights uploaded");
    if (flags & ~(uint32_t)(TT_TRACE_DEVICE_PTRS | TT_TRACE_ASYNC | TT_LIGHT_REFIT_CONSERVATIVE))
        return fail(c, TT_ERR_INVALID_ARG, "tt_lights_refit: unknown flag bits 0x%x", flags);
    SceneDev& d = c->scene;
    // the kernels address the nodes through a buffer resource of n * 40 bytes and 32-bit byte offsets
    if (d.n_lnodes > TT_LIGHT_REFIT_MAX_NODES)
        return fail(c, TT_ERR_UNSUPPORTED, "tt_lights_refit: %u light nodes, more than the %u it can address", d.n_lnodes,
                    (uint32_t)TT_LIGHT_REFIT_MAX_NODES);
    SceneDev::LightRefit& R = d.lrefit;
    const bool dev = (flags & TT_TRACE_DEVICE_PTRS) != 0, cons = (flags & TT_LIGHT_REFIT_CONSERVATIVE) != 0;
    const bool tlas_pass = transforms != nullptr;
    if (!R.plan_valid) {
        tt_lplan::build(host_lights(d), c->host.mesh.data(), R.plan);
        R.plan_valid = true;
        R.dev_valid = false;
    }
    std::string why;
    const tt_status cs = tt_lplan::check_call(R.plan, c->host.mesh.data(), (uint32_t)c->host.mesh.size(), (uint32_t)d.lmeshes_host.size(),
                                              d.n_lnodes, mesh_indices, n_mesh_indices, tlas_pass, dev ? nullptr : transforms,
                                              n_transforms, why);
    if (cs != TT_OK) return fail(c, cs, "tt_lights_refit: %s", why.c_str());
    if (dev && tlas_pass && !is_device_ptr(transforms))
        return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but transforms are not device memory");
    TT_HIP(c, hipSetDevice(c->device));
    const tt_lplan::Plan& P = R.plan;
    if (!R.dev_valid) {
        TT_HIP(c, hipStreamSynchronize(c->stream));  // the old plan's arrays may be in use
        std::vector<int2> up(d.n_lnodes);
        for (uint32_t i = 0; i < d.n_lnodes; i++) up[i] = make_int2(P.parent[i], P.base[i]);
        TT_HIP(c, R.up.alloc(up.size()));
        TT_HIP(c, R.arrive.alloc(up.size()));
        TT_HIP(c, R.leaf_node.alloc(P.leaf_node.size()));
        TT_HIP(c, R.leaf_row.alloc(P.leaf_row.size()));
        TT_HIP(c, hipMemcpy(R.up.p, up.data(), sizeof(int2) * up.size(), hipMemcpyHostToDevice));
        TT_HIP(c, hipMemset(R.arrive.p, 0, sizeof(uint32_t) * up.size()));
        TT_HIP(c, hipMemcpy(R.leaf_node.p, P.leaf_node.data(), sizeof(int32_t) * P.leaf_node.size(), hipMemcpyHostToDevice));
        TT_HIP(c, hipMemcpy(R.leaf_row.p, P.leaf_row.data(), sizeof(int32_t) * P.leaf_row.size(), hipMemcpyHostToDevice));
        R.dev_valid = true;
    }
    // the call's block table: every listed tree's leaves, 256 to a block, no block across two trees
    std::vector<LightRefitBlock> blocks;
    for (uint32_t i = 0; i < n_mesh_indices; i++) {
        const tt_mesh_data& M = c->host.mesh[mesh_indices[i]];
        const tt_lplan::Tree& T = P.trees.at((uint32_t)M.LightNodeOffset);
        for (uint32_t k = 0; k < T.leaf_count; k += 256u)
            blocks.push_back(LightRefitBlock{T.leaf_first + k, std::min(256u, T.leaf_count - k), M.TriOffset, 0u});
    }
    const bool stage_x = tlas_pass && !dev;
    if (R.blocks.n < blocks.size() || (stage_x && R.transforms.n < n_transforms)) {
        TT_HIP(c, hipStreamSynchronize(c->stream));  // (the old tables may be in use)
        if (R.blocks.n < blocks.size()) TT_HIP(c, R.blocks.alloc(blocks.size()));
        if (stage_x && R.transforms.n < n_transforms) TT_HIP(c, R.transforms.alloc(n_transforms));
    }
    const LightRefitPlanDev pd{R.up.p, R.arrive.p, R.leaf_node.p, R.leaf_row.p, d.lnodes.p, d.n_lnodes};
    const tt_light_transform* d_x = transforms;
    SceneWrite w(c, false);
    TT_HIP(c, w.err);
    const size_t b_bytes = sizeof(LightRefitBlock) * blocks.size(), x_bytes = stage_x ? sizeof(tt_light_transform) * n_transforms : 0;
    if (b_bytes + x_bytes) {
        void* pin;
        TT_HIP(c, stage_begin(c, nullptr, b_bytes + x_bytes, pin));
        if (b_bytes) {
            std::memcpy(pin, blocks.data(), b_bytes);
            TT_HIP(c, hipMemcpyAsync(R.blocks.p, pin, b_bytes, hipMemcpyHostToDevice, c->stream));
        }
        if (x_bytes) {
            std::memcpy(static_cast<char*>(pin) + b_bytes, transforms, x_bytes);
            TT_HIP(c, hipMemcpyAsync(R.transforms.p, static_cast<char*>(pin) + b_bytes, x_bytes, hipMemcpyHostToDevice, c->stream));
            d_x = R.transforms.p;
        }
        TT_HIP(c, stage_end(c));
    }
    uint32_t slot;
    TT_HIP(c, ring_open(c, c->timing, slot));
    TT_HIP(c, tt_light_refit_forest(pd, R.blocks.p, (uint32_t)blocks.size(), d.ltris.p, d.tris_raw.p, (uint32_t)d.tris_raw.n, cons, c->stream));
    if (tlas_pass)
        TT_HIP(c, tt_light_refit_tlas(pd, P.tlas.leaf_first, P.tlas.leaf_count, d_x, n_transforms, cons, c->stream));
    note_stream_launch(c->stream);
    TT_HIP(c, ring_close(c, c->timing, slot));
    TT_HIP(c, w.end());
    if (!(flags & TT_TRACE_ASYNC)) TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_scene_read_light_nodes(tt_ctx* c, uint32_t first, uint32_t count, tt_light_node* out) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (!c->has_scene || c->scene.n_lnodes == 0) return fail(c, TT_ERR_NO_SCENE, "tt_scene_read_light_nodes: no lights uploaded");
    if (!out || (uint64_t)first + count > c->scene.n_lnodes)
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_read_light_nodes: range out of bounds");
    TT_HIP(c, hipSetDevice(c->device));
    SceneRead sr(c);
    TT_HIP(c, sr.err);
    TT_HIP(c, hipMemcpyAsync(out, c->scene.lnodes.p + first, sizeof(tt_light_node) * count, hipMemcpyDeviceToHost, c->stream));
    sr.end();
    TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_scene_read_light_tris(tt_ctx* c, uint32_t first, uint32_t count, tt_light_tri* out) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (!c->has_scene || c->scene.n_lnodes == 0) return fail(c, TT_ERR_NO_SCENE, "tt_scene_read_light_tris: no lights uploaded");
    if (!out || (uint64_t)first + count > c->scene.ltris.n)
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_read_light_tris: range out of bounds");
    TT_HIP(c, hipSetDevice(c->device));
    SceneRead sr(c);
    TT_HIP(c, sr.err);
    TT_HIP(c, hipMemcpyAsync(out, c->scene.ltris.p + first, sizeof(tt_light_tri) * count, hipMemcpyDeviceToHost, c->stream));
    sr.end();
    TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_emit_nee(tt_ctx* c, const tt_trace_params* p, const tt_ray_data* rays, int32_t frames, int32_t max_bounce,
                      tt_light_sample* samples, tt_shadow_ray* shadow, uint32_t* n_shadow) {
    return emit_call(c, p, nullptr, rays, frames, max_bounce, samples, shadow, n_shadow, nullptr);
}

tt_status tt_emit_nee_indirect(tt_ctx* c, const tt_trace_params* p, const uint32_t* n_rays_dev, const tt_ray_data* rays,
                               int32_t frames, int32_t max_bounce, tt_light_sample* samples, tt_shadow_ray* shadow,
                               uint32_t* n_shadow_dev) {
    if (!n_shadow_dev) return c ? fail(c, TT_ERR_INVALID_ARG, "null device survivor count") : TT_ERR_INVALID_ARG;
    return emit_call(c, p, n_rays_dev, rays, frames, max_bounce, samples, shadow, nullptr, n_shadow_dev);
}

}  // extern "C"
