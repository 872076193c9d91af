// tt_dispatch.hip — the C ABI of include/truetrace_hip.h, part three: the launches. Closest hit, any hit, the
// heightmap and shadow-heightmap marches, the normal resolve, primary-ray generation and the bounce enqueue.
#include <cstdlib>

#include "tt_call_host.h"
#include "tt_ctx.h"
#include "tt_launch.h"

namespace {
MatView mat_view(const tt_ctx* c) {
    MatView m;
    m.word = c->scene.mat_tag.p;
    m.cut = c->scene.mat_cut.p;
    m.raw = c->scene.tris_raw.p;
    m.atlas = c->scene.atlas.p;
    m.n_mat = c->host.n_mat;
    m.atlas_w = c->scene.atlas_w;
    m.atlas_h = c->scene.atlas_h;
    m.glass = c->scene.mat_glass.p;
    m.tex = c->scene.tex.p;
    m.tex_w = c->scene.tex_w;
    m.tex_h = c->scene.tex_h;
    return m;
}

tt_status refused(tt_ctx* c, const tt_call::Refusal& r) { return fail(c, r.status, "%s", r.text); }

// the scene as the traversal kernels see it: the fields TraceArgs and ShadowArgs have in common
template <class Args>
void fill_scene_args(const tt_ctx* c, Args& a) {
    a.nodes = kernel_nodes(c);
    a.n_nodes = c->n_nodes_dev;  // (the overlay regions included: a frame-slot TLAS lives there)
    a.tlas_base = c->tlas_base;
    a.tris = c->scene.tris.p;
    a.n_tris = c->host.n_tris;
    a.tlas = c->scene.tlas.p;
    a.mesh = c->scene.mesh.p;
    a.leaf = c->scene.leaf.p;
    a.mat_tag = c->scene.mat_tag.p;
    a.n_mat = c->host.n_mat;
    a.mat = mat_view(c);
    a.sticky_overflow = c->sticky;
    a.spill = c->spill.p;
}

void read_stats(const TraceControl& ctl, tt_stats* stats) {
    stats->rays = ctl.stats[0];
    stats->node_visits = ctl.stats[1];
    stats->tri_tests = ctl.stats[2];
    stats->blas_entries = ctl.stats[3];
    stats->hits = ctl.stats[4];
    stats->reps_exhausted = ctl.stats[5];
    stats->stack_overflows = ctl.stats[6];
    stats->accepts = ctl.stats[7];
}

// Host-pointer staging of the any-hit paths (tt_trace_shadow*, tt_trace_shadow_heightmap*): the rays, and
// GlobalColors / NEEPosA / CacheBuffer where passed. The visibility records follow each path's own rule.
struct ShadowArrays {
    tt_shadow_ray* rays;
    float4* vis;
    tt_col_data* col;
    float4* nee;
    tt_cache_data* cache;
};
tt_status stage_shadow_in(tt_ctx* c, uint32_t n_rays, uint64_t wh, const tt_shadow_ray* rays, const tt_col_data* colors,
                          const float* nee_pos, const tt_cache_data* cache, ShadowArrays& d) {
    if (cache) TT_HIP(c, stage_in(c, c->st_cache, cache, wh, 0, d.cache));
    TT_HIP(c, stage_in(c, c->st_shadow, rays, n_rays, 0, d.rays));
    if (colors) TT_HIP(c, stage_in(c, c->st_colors, colors, wh, 0, d.col));
    if (nee_pos) TT_HIP(c, stage_in(c, c->st_nee, nee_pos, wh, 0, d.nee));
    return TT_OK;
}
tt_status stage_shadow_out(tt_ctx* c, uint32_t n_rays, uint64_t wh, const ShadowArrays& d, float* visibility,
                           tt_col_data* colors, float* nee_pos, tt_cache_data* cache) {
    if (visibility) TT_HIP(c, stage_out(c, visibility, d.vis, n_rays));
    if (colors) TT_HIP(c, stage_out(c, colors, d.col, wh));
    if (nee_pos) TT_HIP(c, stage_out(c, nee_pos, d.nee, wh));
    if (cache) TT_HIP(c, stage_out(c, cache, d.cache, wh));
    return TT_OK;
}
}  // namespace

// n_dev (nullable): the device-resident ray count (tt_trace_closest_indirect); p->n_rays is then the
// capacity the launch covers, and the call is asynchronous with device pointers.
static tt_status trace_closest_call(tt_ctx* c, const tt_trace_params* p, const uint32_t* n_dev, tt_ray_data* rays,
                                    uint32_t* info, const tt_col_data* colors, tt_stats* stats,
                                    uint32_t* hits_out = nullptr) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    const tt_call::Path& path = tt_call::kTrace;
    const tt_call::Common q = (p && rays) ? tt_call::common_of(*p) : tt_call::Common{};
    if (const tt_call::Refusal r = tt_call::check_shape(path, p && rays, q)) return refused(c, r);
    // FarPlane (camera.farClipPlane) seeds best.t, the node test's t_max; the kernel's t_max clamp
    // assumes it is not a NaN (tt_traverse.h)
    if (p->far_plane != p->far_plane) return fail(c, TT_ERR_INVALID_ARG, "far_plane is NaN");
    if (info && p->bounce > 0 && !colors)
        return fail(c, TT_ERR_INVALID_ARG, "GlobalColors required for _PrimaryTriangleInfo at bounce > 0");
    if (c->host.any_cutout && !c->scene.atlas.p)
        return fail(c, TT_ERR_UNSUPPORTED,
                    "scene has Cutout materials but no alpha atlas was uploaded (tt_scene_upload_alpha_atlas)");
    const tt_call::Plan pl = tt_call::plan_call(path, q, n_dev != nullptr, n_dev && is_device_ptr(n_dev));
    if (pl.refusal) return refused(c, pl.refusal);
    const uint64_t wh = pl.wh;
    const uint32_t off = pl.off;
    const bool dev = pl.dev, async = pl.async, want_stats = pl.want_stats;
    const int info_mode = info ? (p->bounce == 0 ? 1 : 2) : 0;
    const bool adaptive = (p->flags & TT_TRACE_ADAPTIVE_ORDER) && !want_stats && !n_dev;
    if (hits_out) {
        if (!dev) return fail(c, TT_ERR_INVALID_ARG, "a hit-record stream needs TT_TRACE_DEVICE_PTRS");
        if (!is_device_ptr(hits_out)) return fail(c, TT_ERR_INVALID_ARG, "hits_out is not device memory");
        if (reinterpret_cast<uintptr_t>(hits_out) % 16) return fail(c, TT_ERR_INVALID_ARG, "hits_out must be 16-byte aligned");
        // the kernel stores record i at the 32-bit byte offset 16 i of a 2 GiB buffer descriptor
        if (p->n_rays > (1u << 27)) return fail(c, TT_ERR_INVALID_ARG, "a hit-record stream holds at most 2^27 rays per call");
    }
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (p->n_rays == 0) return TT_OK;
    if (const tt_call::Refusal r = tt_call::check_alignment(path, rays, info)) return refused(c, r);
    TT_HIP(c, hipSetDevice(c->device));

    tt_ray_data* d_rays = rays;
    uint32_t* d_info = info;
    const tt_col_data* d_colors = colors;
    if (dev) {
        if (!is_device_ptr(rays)) return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but rays is not device memory");
    } else {
        TT_HIP(c, stage_in(c, c->st_rays, rays, p->n_rays, off, d_rays));
        if (info) TT_HIP(c, stage_in(c, c->st_info, info, wh * 4, 0, d_info));
        if (info && p->bounce > 0) TT_HIP(c, stage_in(c, c->st_colors, colors, wh, 0, d_colors));
    }
    TraceArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_scene_args(c, a);
    a.rays = d_rays;
    a.info = d_info;
    a.colors = d_colors;
    const uint32_t ci = c->ctl_cur;
    a.ctl = c->ctl + ci;
    a.ctl_next = c->ctl + (ci ^ 1u);
    a.n_rays = p->n_rays;
    a.n_rays_dev = n_dev;
    a.ray_offset = off;
    a.width = p->screen_width;
    a.height = p->screen_height;
    a.n_pixels = (uint32_t)wh;
    a.far_plane = p->far_plane;
    a.bounce = p->bounce;
    a.flags = p->flags;
    // (the kernel also requires its actual count to be W*H: a device count decides at run time)
    a.tile_swizzle = ((n_dev ? p->n_rays >= wh : p->n_rays == wh) && p->screen_width % 8 == 0 &&
                      p->screen_height % 8 == 0) ? 1u : 0u;
    a.div_width = fastdiv_make(std::max(1u, p->screen_width));
    a.div_tiles = fastdiv_make(std::max(1u, p->screen_width >> 3));
    a.hits_out = reinterpret_cast<uint4*>(hits_out);
    {  // TT_ROOT_LEAF: node 0 as a one-leaf TLAS root, when the host knows the device's node 0 (the lender's,
       // or a frame-slot TLAS's own)
        tt_ctx* owner = (c->lender && !c->ovl) ? c->lender : c;
        std::lock_guard<std::recursive_mutex> lk(owner->mu);
        if (owner->root_known && !owner->host.nodes.empty()) {
            a.root = root_leaf_of(reinterpret_cast<const uint32_t*>(owner->host.nodes.data()));
            a.root.base_child += c->tlas_base;
        }
    }
#ifdef TT_DIAG_BLOCKS  // diagnostic builds only: the block counters' device buffer (tools/diag_blocks.py)
    if (const char* dp = std::getenv("TT_DIAG_PTR"))
        a.diag_times = reinterpret_cast<unsigned long long*>(std::strtoull(dp, nullptr, 0));
#endif
    const bool matcheck = (c->any_invisible && p->bounce == 0) || c->host.any_cutout ||
                          ((p->flags & TT_TRACE_IGNORE_GLASS) && c->host.any_atlas_shadow) ||
                          ((p->flags & TT_TRACE_IGNORE_BACKFACING) && p->bounce == 0);
    // one dequeue chunk per wave: a launch smaller than the resident grid spreads over as many
    // waves as it has chunks (r02: sizing this for 256-ray chunks left a 260k-ray launch -- one
    // rank's shard at 8 GPUs -- on ~1 wave per SIMD, 4 chunks each)
    static const uint32_t chunks_per_wave = [] {  // TT_CHUNKS_PER_WAVE: experiment knob (default 1)
        const char* e = std::getenv("TT_CHUNKS_PER_WAVE");
        const int v = e ? std::atoi(e) : 1;
        return (uint32_t)std::max(1, std::min(v, 64));
    }();
    const uint32_t chunks_needed = (p->n_rays + tt_trace_chunk_rays() - 1u) / tt_trace_chunk_rays();
    const uint32_t waves_needed = (chunks_needed + chunks_per_wave - 1u) / chunks_per_wave;
    const uint32_t wpb = std::max(1u, tt_trace_block_size() / 64u);  // waves per block
    const uint32_t blocks_needed = (waves_needed + wpb - 1u) / wpb;
    // The leaf-TLAS kernels (tt_trace.hip): node 0, known to the host, is one leaf holding exactly one instance
    // (a device TLAS refit clears root_known, so a.root.ok is 0 until the next node update), and the launch wants
    // no stats, no material check and no adaptive order. TT_LEAF_KERNEL=0 forces the generic kernels (A/B, tests).
    static const bool leaf_enabled = [] {
        const char* e = std::getenv("TT_LEAF_KERNEL");
        return !(e && std::atoi(e) == 0);
    }();
    const bool leaf = leaf_enabled && root_one_instance(a.root) && !want_stats && !matcheck && !adaptive;
    const uint32_t grid_index = leaf ? 18u + (n_dev ? 3u : 0u) + (uint32_t)info_mode
                                     : (adaptive ? 12u : want_stats ? 6u : 0u) + (matcheck ? 3u : 0u) + (uint32_t)info_mode;
    const uint32_t grid = std::max(1u, std::min(c->grid_of[grid_index], blocks_needed));
    // TT_TRACE_ADAPTIVE_ORDER: this launch fills cost[cur ^ 1] (per 64-ray chunk); with the previous
    // launch's costs in cost[cur] the order kernel (inside the timed entry) sorts this launch's chunks
    tt_ctx::OrderSlot* os = nullptr;
    const uint32_t n_chunks = (p->n_rays + 63u) / 64u;
    if (adaptive) {
        os = &c->ord[std::min(p->bounce, 7)];
        if (os->w != p->screen_width || os->h != p->screen_height) {  // (costs outlive scene updates: a hint)
            os->valid = false;
            os->w = p->screen_width;
            os->h = p->screen_height;
        }
        if (os->order.n < n_chunks) {  // (a fresh map pair starts from zero costs)
            TT_HIP(c, os->order.alloc(n_chunks));
            TT_HIP(c, os->cost[0].alloc(n_chunks));
            TT_HIP(c, os->cost[1].alloc(n_chunks));
            TT_HIP(c, hipMemsetAsync(os->cost[0].p, 0, sizeof(uint32_t) * n_chunks, c->stream));
            os->valid = false;
        }
        if (!os->valid) TT_HIP(c, hipMemsetAsync(os->cost[os->cur ^ 1u].p, 0, sizeof(uint32_t) * n_chunks, c->stream));
        a.chunk_cost = os->cost[os->cur ^ 1u].p;
    }
    // Control blocks: every trace kernel zeroes the OTHER block at its start (block 0, plain stores;
    // the previous launch on the stream, which used it, has finished), so back-to-back async
    // launches need no fill kernel in between. Synchronous / stats launches, and the first launch
    // after an any-hit launch, still zero their block here. (A reset by the last wave to exit instead
    // needs a device-scope fence per wave, which writes back L2 under the draining waves: measured
    // 15% slower, profiles/r01_exp_ctl_reset.txt.)
    static const bool always_reset = std::getenv("TT_CTL_ALWAYS_RESET") != nullptr;  // A/B knob
    if (!async || want_stats || !c->ctl_zero[ci] || always_reset)
        TT_HIP(c, hipMemsetAsync(c->ctl + ci, 0, sizeof(TraceControl), c->stream));
    SceneRead sr(c);
    TT_HIP(c, sr.err);
    const bool ring = c->timing || !async;  // (a synchronous call reports its kernel time)
    uint32_t slot;
    TT_HIP(c, ring_open(c, ring, slot));
    c->ctl_zero[0] = c->ctl_zero[1] = false;
    static const bool record_only = std::getenv("TT_ORDER_RECORD_ONLY") != nullptr;  // A/B knob: costs, no order
    if (os && os->valid && record_only)  // the order kernel (which clears the map this launch fills) is skipped
        TT_HIP(c, hipMemsetAsync(os->cost[os->cur ^ 1u].p, 0, sizeof(uint32_t) * n_chunks, c->stream));
    if (os && os->valid && !record_only) {
        OrderArgs o;
        o.cost = os->cost[os->cur].p;
        o.cost_clear = os->cost[os->cur ^ 1u].p;
        o.n_rays = p->n_rays;
        o.n_chunks = n_chunks;
        static const uint32_t hot = [] {  // A/B knob: hoist only the chunks of long rays
            const char* e = std::getenv("TT_ORDER_HOT");
            return e ? (uint32_t)std::atoi(e) : 0u;
        }();
        o.hot = hot;
        o.order = os->order.p;
        TT_HIP(c, tt_launch_order(o, c->stream));
        a.order = os->order.p;
    }
    TT_HIP(c, tt_launch_trace(a, want_stats, matcheck, info_mode, leaf, grid, c->stream));
    c->last_form = leaf ? TT_TRACE_FORM_LEAF : TT_TRACE_FORM_GENERIC;
    note_stream_launch(c->stream);
    if (os) {
        os->cur ^= 1u;
        os->valid = true;
        os->n_chunks = n_chunks;
    }
    c->ctl_zero[ci ^ 1u] = true;
    c->ctl_cur = ci ^ 1u;
    TT_HIP(c, ring_close(c, ring, slot));
    sr.end();
    if (async) return TT_OK;
    TraceControl ctl;
    TT_HIP(c, hipMemcpyAsync(&ctl, c->ctl + ci, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    if (!dev) {
        TT_HIP(c, stage_out(c, rays, d_rays, p->n_rays, off));
        if (info) TT_HIP(c, stage_out(c, info, d_info, wh * 4));
    }
    TT_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    TT_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (stats) {
        stats->kernel_ms = ms;
        if (want_stats) {
            read_stats(ctl, stats);
            for (int k = 0; k < 8; k++) c->last_diag[k] = ctl.diag[k];
        }
        stats->stack_overflows = std::max<uint64_t>(stats->stack_overflows, ctl.err_overflow);
    }
    if (ctl.err_overflow)
        return fail(c, TT_ERR_STACK_OVERFLOW, "%u rays needed more than %d traversal stack entries", ctl.err_overflow,
                    TT_STACK_SIZE);
    return TT_OK;
}

extern "C" {

tt_status tt_trace_chunk_costs(tt_ctx* c, int32_t bounce, uint32_t* costs, uint32_t max, uint32_t* n) {
    if (!c || !n || (max && !costs) || bounce < 0) return TT_ERR_INVALID_ARG;
    *n = 0;
    const tt_ctx::OrderSlot& os = c->ord[std::min(bounce, 7)];
    if (!os.valid) return TT_OK;
    TT_HIP(c, hipSetDevice(c->device));
    const uint32_t k = std::min(os.n_chunks, max);
    if (k) TT_HIP(c, hipMemcpyAsync(costs, os.cost[os.cur].p, sizeof(uint32_t) * k, hipMemcpyDeviceToHost, c->stream));
    TT_HIP(c, hipStreamSynchronize(c->stream));
    *n = k;
    return TT_OK;
}

tt_status tt_trace_closest(tt_ctx* c, const tt_trace_params* p, tt_ray_data* rays, uint32_t* info,
                           const tt_col_data* colors, tt_stats* stats) {
    return trace_closest_call(c, p, nullptr, rays, info, colors, stats);
}

tt_status tt_trace_closest_hits(tt_ctx* c, const tt_trace_params* p, tt_ray_data* rays, uint32_t* info,
                                const tt_col_data* colors, uint32_t* hits_out) {
    if (!hits_out) return c ? fail(c, TT_ERR_INVALID_ARG, "null hits_out") : TT_ERR_INVALID_ARG;
    return trace_closest_call(c, p, nullptr, rays, info, colors, nullptr, hits_out);
}

tt_status tt_trace_closest_indirect(tt_ctx* c, const tt_trace_params* p, const uint32_t* n_rays_dev, tt_ray_data* rays,
                                    uint32_t* info, const tt_col_data* colors) {
    if (!n_rays_dev) return c ? fail(c, TT_ERR_INVALID_ARG, "null device ray count") : TT_ERR_INVALID_ARG;
    return trace_closest_call(c, p, n_rays_dev, rays, info, colors, nullptr);
}

}  // extern "C"

// full = false: tt_trace_shadow's contract (Direct at bounce 0 + NEEPosA only, the caller does the
// rest); full = true: tt_trace_shadow_ex's (plus CacheBuffer / Indirect / PrimaryNEERay)
static tt_status shadow_call(tt_ctx* c, const tt_shadow_params* p, tt_shadow_ray* rays, float* visibility,
                             tt_col_data* colors, float* nee_pos, tt_cache_data* cache, tt_stats* stats, bool full,
                             const uint32_t* n_dev = nullptr) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    const tt_call::Path& path = tt_call::kShadow;
    const tt_call::Common q = (p && rays) ? tt_call::common_of(*p) : tt_call::Common{};
    if (const tt_call::Refusal r = tt_call::check_shape(path, p && rays, q)) return refused(c, r);
    if (c->host.any_atlas_shadow && !c->scene.tex.p)
        return fail(c, TT_ERR_UNSUPPORTED,
                    "scene has glass (specTrans == 1) materials but no texture atlas was uploaded "
                    "(tt_scene_upload_texture_atlas; the shadow tint samples it, CommonData.cginc:618-625)");
    if (c->host.any_cutout && !c->scene.atlas.p)
        return fail(c, TT_ERR_UNSUPPORTED,
                    "scene has Cutout materials but no alpha atlas was uploaded (tt_scene_upload_alpha_atlas)");
    const tt_call::Plan pl = tt_call::plan_call(path, q, n_dev != nullptr, n_dev && is_device_ptr(n_dev));
    if (pl.refusal) return refused(c, pl.refusal);
    const uint64_t wh = pl.wh;
    const bool dev = pl.dev, async = pl.async, want_stats = pl.want_stats;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (p->n_rays == 0) return TT_OK;
    if (const tt_call::Refusal r = tt_call::check_alignment(path, rays, visibility, nee_pos)) return refused(c, r);
    TT_HIP(c, hipSetDevice(c->device));
    ShadowArrays d{rays, reinterpret_cast<float4*>(visibility), colors, reinterpret_cast<float4*>(nee_pos), cache};
    if (dev) {
        if (!is_device_ptr(rays)) return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but rays is not device memory");
    } else {
        const tt_status st = stage_shadow_in(c, p->n_rays, wh, rays, colors, nee_pos, cache, d);
        if (st != TT_OK) return st;
        if (visibility) TT_HIP(c, stage_in(c, c->st_vis, nullptr, p->n_rays, 0, d.vis));  // (an output only)
    }
    // the accumulations beyond Direct / NEEPosA run in a second pass that reads the visibility
    // records: give the traversal one when the caller passed none
    const bool vis_check = (p->flags & TT_SHADOW_VISIBILITY_CHECK) != 0;
    const bool accumulate = full && !vis_check && (d.col || d.cache);
    if (accumulate && !d.vis) TT_HIP(c, stage_in(c, c->st_vis, nullptr, p->n_rays, 0, d.vis));
    ShadowArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_scene_args(c, a);
    a.rays = d.rays;
    a.visibility = d.vis;
    a.colors = d.col;
    a.nee_pos = d.nee;
    a.cache = d.cache;
    a.ctl = c->ctl + c->ctl_cur;
    a.n_rays = p->n_rays;
    a.n_rays_dev = n_dev;
    a.width = p->screen_width;
    a.height = p->screen_height;
    a.bounce = p->bounce;
    a.flags = p->flags;
    const bool matcheck = c->host.any_shadow_skip || c->host.any_cutout || c->host.any_atlas_shadow;
    const uint32_t wpb = std::max(1u, tt_trace_block_size() / 64u);  // waves per block
    const uint32_t blocks_needed = ((p->n_rays + tt_trace_chunk_rays() - 1u) / tt_trace_chunk_rays() + wpb - 1u) / wpb;
    const uint32_t grid =
        std::max(1u, std::min(c->shadow_grid_of[(want_stats ? 2 : 0) + (matcheck ? 1 : 0)], blocks_needed));
    TT_HIP(c, hipMemsetAsync(c->ctl + c->ctl_cur, 0, sizeof(TraceControl), c->stream));
    SceneRead sr(c);
    TT_HIP(c, sr.err);
    const bool ring = c->timing || !async;  // (a synchronous call reports its kernel time)
    uint32_t slot;
    TT_HIP(c, ring_open(c, ring, slot));
    c->ctl_zero[0] = c->ctl_zero[1] = false;  // the any-hit kernel zeroes nothing
    TT_HIP(c, tt_launch_shadow(&a, grid, c->stream, want_stats ? 1 : 0, matcheck ? 1 : 0));
    note_stream_launch(c->stream);
    TT_HIP(c, ring_close(c, ring, slot));
    if (accumulate) TT_HIP(c, tt_launch_shadow_accumulate(&a, d.vis, c->stream));
    sr.end();
    if (async) return TT_OK;
    TraceControl ctl;
    TT_HIP(c, hipMemcpyAsync(&ctl, c->ctl + c->ctl_cur, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    if (!dev) {
        TT_HIP(c, stage_out(c, rays, d.rays, p->n_rays));
        const tt_status st = stage_shadow_out(c, p->n_rays, wh, d, visibility, colors, nee_pos, cache);
        if (st != TT_OK) return st;
    }
    TT_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    TT_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (stats) {
        stats->kernel_ms = ms;
        if (want_stats) read_stats(ctl, stats);  // hits = occluded rays, accepts = rays that reached |t|
        stats->stack_overflows = std::max<uint64_t>(stats->stack_overflows, ctl.err_overflow);
    }
    if (ctl.err_overflow)
        return fail(c, TT_ERR_STACK_OVERFLOW, "%u shadow rays needed more than %d traversal stack entries",
                    ctl.err_overflow, TT_STACK_SIZE);
    return TT_OK;
}

extern "C" {

tt_status tt_trace_shadow(tt_ctx* c, const tt_shadow_params* p, tt_shadow_ray* rays, float* visibility,
                          tt_col_data* colors, float* nee_pos, tt_stats* stats) {
    return shadow_call(c, p, rays, visibility, colors, nee_pos, nullptr, stats, false);
}

tt_status tt_trace_shadow_ex(tt_ctx* c, const tt_shadow_params* p, tt_shadow_ray* rays, float* visibility,
                             tt_col_data* colors, float* nee_pos, tt_cache_data* cache, tt_stats* stats) {
    return shadow_call(c, p, rays, visibility, colors, nee_pos, cache, stats, true);
}

tt_status tt_trace_shadow_ex_indirect(tt_ctx* c, const tt_shadow_params* p, const uint32_t* n_rays_dev,
                                      tt_shadow_ray* rays, float* visibility, tt_col_data* colors, float* nee_pos,
                                      tt_cache_data* cache) {
    if (!n_rays_dev) return c ? fail(c, TT_ERR_INVALID_ARG, "null device ray count") : TT_ERR_INVALID_ARG;
    return shadow_call(c, p, rays, visibility, colors, nee_pos, cache, nullptr, true, n_rays_dev);
}

tt_status tt_resolve_normals(tt_ctx* c, const tt_trace_params* p, const tt_ray_data* rays, float* normals6) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    if (!p || !rays || !normals6) return fail(c, TT_ERR_INVALID_ARG, "null argument");
    const uint64_t wh = (uint64_t)p->screen_width * p->screen_height;
    const uint32_t off = (p->bounce % 2 == 1) ? (uint32_t)wh : 0u;
    if (p->n_rays == 0) return TT_OK;
    TT_HIP(c, hipSetDevice(c->device));
    const bool dev = (p->flags & TT_TRACE_DEVICE_PTRS) != 0;
    const tt_ray_data* d_rays = rays;
    float* d_out = normals6;
    if (!dev) {
        TT_HIP(c, stage_in(c, c->st_rays, rays, p->n_rays, off, d_rays));
        TT_HIP(c, stage_in(c, c->st_normals, nullptr, (size_t)6 * p->n_rays, 0, d_out));
    }
    SceneRead sr(c);
    TT_HIP(c, sr.err);
    TT_HIP(c, tt_launch_resolve(d_rays, off, p->n_rays, p->far_plane, c->scene.tris_raw.p, (uint32_t)c->scene.tris_raw.n,
                                c->scene.mesh_raw.p, (uint32_t)c->scene.mesh_raw.n, d_out, c->stream, c->scene.terrains.p,
                                (uint32_t)c->scene.terrains_host.size(), c->scene.hmap.p, c->scene.hmap_w, c->scene.hmap_h));
    sr.end();
    if (!dev) TT_HIP(c, stage_out(c, normals6, d_out, (size_t)6 * p->n_rays));
    TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_generate_primary(tt_ctx* c, const tt_camera* cam, tt_ray_data* rays) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    if (!cam || !rays || !cam->width || !cam->height) return fail(c, TT_ERR_INVALID_ARG, "bad camera or rays");
    const uint64_t wh = (uint64_t)cam->width * cam->height;
    if (wh > 0x7fffffffull) return fail(c, TT_ERR_INVALID_ARG, "screen too large");
    TT_HIP(c, hipSetDevice(c->device));
    const bool dev = (cam->flags & TT_TRACE_DEVICE_PTRS) != 0;
    // TT_TRACE_ASYNC with device rays: nothing waits (the camera goes in the kernel arguments)
    const bool async = dev && (cam->flags & TT_TRACE_ASYNC);
    tt_ray_data* d = rays;
    if (!dev) {
        TT_HIP(c, stage_in(c, c->st_rays, nullptr, wh, 0, d));
    } else if (!is_device_ptr(rays)) {
        return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but rays is not device memory");
    }
    uint32_t slot;
    TT_HIP(c, ring_open(c, c->timing, slot));
    TT_HIP(c, tt_launch_generate(cam->cam_to_world, cam->cam_inv_proj, cam->width, cam->height, cam->near_plane, cam->far_plane,
                                 cam->jitter, cam->frames_accumulated, cam->max_bounce, d, c->stream));
    note_stream_launch(c->stream);
    TT_HIP(c, ring_close(c, c->timing, slot));
    if (!dev) TT_HIP(c, stage_out(c, rays, d, wh));
    if (!async) TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

}  // extern "C"

// n_dev (nullable): device-resident count of the rays traced at p->bounce (p->n_rays = capacity);
// n_next_dev (nullable): the survivor count is written there on the device and the call returns
// without synchronizing (n_next may then be null).
static tt_status enqueue_call(tt_ctx* c, const tt_trace_params* p, const uint32_t* n_dev, tt_ray_data* rays,
                              int32_t frames, int32_t max_bounce, uint32_t* n_next, uint32_t* n_next_dev) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    const bool have_args = p && rays && (n_next || n_next_dev);
    const tt_call::EnqueuePlan pl =
        tt_call::check_enqueue(have_args, have_args ? tt_call::common_of(*p) : tt_call::Common{}, n_dev || n_next_dev);
    if (pl.refusal) return refused(c, pl.refusal);
    const uint64_t wh = pl.wh;
    const uint32_t src = pl.src, dst = pl.dst;
    const bool dev = pl.dev;
    if ((n_dev && !is_device_ptr(n_dev)) || (n_next_dev && !is_device_ptr(n_next_dev)))
        return fail(c, TT_ERR_INVALID_ARG, "a ray count pointer is not device memory");
    TT_HIP(c, hipSetDevice(c->device));
    // [0] survivor count, [1] tile ticket, [2..3] pad, then one 64-bit look-back word per tile
    // two counter blocks, used in turn: each enqueue zeroes the other block for the next one (no fill
    // between enqueues); a larger capacity reallocates and fills both
    const size_t ctl_words = 4 + 2 * (size_t)tt_bounce_tiles(p->n_rays);
    if (c->counter_words < ctl_words) {
        TT_HIP(c, hipStreamSynchronize(c->stream));  // (the old blocks may be in use)
        c->counter.release();
        TT_HIP(c, c->counter.alloc(2 * ctl_words));
        TT_HIP(c, hipMemsetAsync(c->counter.p, 0, 2 * 4 * ctl_words, c->stream));
        c->counter_words = (uint32_t)ctl_words;
        c->counter_cur = 0;
    }
    uint32_t* const ctl_cur = c->counter.p + (size_t)c->counter_cur * c->counter_words;
    uint32_t* const ctl_next = c->counter.p + (size_t)(c->counter_cur ^ 1u) * c->counter_words;
    tt_ray_data* d = rays;
    if (!dev) {
        // room for both windows; keep nothing: the host copy is the source of truth for host-pointer calls
        TT_HIP(c, stage_in(c, c->st_rays, nullptr, 2 * wh, 0, d));
        TT_HIP(c, stage_in(c, c->st_rays, rays, p->n_rays, src, d));
    }
    // TT_ENQUEUE_TERRAIN_BOUNCE on a context with terrains: the kernel's terrain instantiation (tt_raygen.hip)
    const uint32_t n_ter = (uint32_t)c->scene.terrains_host.size();
    const bool bounce_off = n_ter != 0u && (p->flags & TT_ENQUEUE_TERRAIN_BOUNCE) != 0;
    uint32_t slot;
    SceneRead sr(c);
    TT_HIP(c, sr.err);
    TT_HIP(c, ring_open(c, c->timing, slot));
    TT_HIP(c, tt_launch_bounce(d, src, dst, p->n_rays, p->far_plane, p->bounce, frames, max_bounce, c->scene.tris_raw.p,
                               c->scene.mesh_raw.p, ctl_cur, c->stream, n_dev, n_next_dev, ctl_next, c->counter_words,
                               c->frame_pixels, n_ter ? 1u : 0u, bounce_off ? c->scene.terrains.p : nullptr,
                               bounce_off ? n_ter : 0u, c->scene.hmap.p, c->scene.hmap_w, c->scene.hmap_h));
    c->counter_cur ^= 1u;
    TT_HIP(c, ring_close(c, c->timing, slot));
    sr.end();
    if (n_next_dev) {  // BufferSizes[CurBounce + 1].tracerays stays on the GPU: no host round trip
        if (n_next) *n_next = 0;
        return TT_OK;
    }
    uint32_t cnt = 0;
    TT_HIP(c, hipMemcpyAsync(&cnt, ctl_cur, 4, hipMemcpyDeviceToHost, c->stream));
    TT_HIP(c, hipStreamSynchronize(c->stream));
    if (!dev && cnt) {
        TT_HIP(c, hipMemcpy(rays + dst, d + dst, sizeof(tt_ray_data) * cnt, hipMemcpyDeviceToHost));
    }
    *n_next = cnt;
    return TT_OK;
}

extern "C" {

tt_status tt_enqueue_diffuse_bounce(tt_ctx* c, const tt_trace_params* p, tt_ray_data* rays, int32_t frames,
                                    int32_t max_bounce, uint32_t* n_next) {
    if (c && !n_next) return fail(c, TT_ERR_INVALID_ARG, "null argument");
    return enqueue_call(c, p, nullptr, rays, frames, max_bounce, n_next, nullptr);
}

tt_status tt_enqueue_diffuse_bounce_indirect(tt_ctx* c, const tt_trace_params* p, const uint32_t* n_rays_dev,
                                             tt_ray_data* rays, int32_t frames, int32_t max_bounce,
                                             uint32_t* n_next_dev) {
    if (!n_next_dev) return c ? fail(c, TT_ERR_INVALID_ARG, "null device survivor count") : TT_ERR_INVALID_ARG;
    return enqueue_call(c, p, n_rays_dev, rays, frames, max_bounce, nullptr, n_next_dev);
}

}  // extern "C"

// ------------------------------------------------------------------ terrains (tt_terrain.hip)
namespace {

// The march kernels' form. The one-thread-per-ray grid kernels are the product: on the measured workloads
// (profiles/r08/terrain/bench.json) they beat the persistent refill kernels, which TT_TERRAIN_FORM=persistent
// (read once per process) selects for A/B measurement. Results are identical in both forms.
bool terrain_grid_form() {
    static const bool grid = [] {
        const char* e = std::getenv("TT_TERRAIN_FORM");
        return !(e && std::strcmp(e, "persistent") == 0);
    }();
    return grid;
}

// resident persistent grid of the march kernels, sized on first use; kind: 0 closest hit, 1 with stats, 2 shadow
uint32_t terrain_grid(tt_ctx* c, int kind, uint32_t n_rays) {
    if (terrain_grid_form()) return 0u;  // (the grid form sizes itself by the ray count)
    if (!c->terrain_grid_of[0]) {
        int occ[3];
        tt_terrain_occupancy_table(occ);
        for (int k = 0; k < 3; k++) c->terrain_grid_of[k] = (uint32_t)(c->num_cus * std::max(1, std::min(occ[k], 32)));
    }
    return std::max(1u, std::min(c->terrain_grid_of[kind], (n_rays + 63u) / 64u));
}

// the scheduler tickets (and, first = true, the stats) of the launch's control block
hipError_t reset_terrain_control(tt_ctx* c, bool first) {
    if (!first && terrain_grid_form()) return hipSuccess;  // (no tickets; the stats accumulate over the terrains)
    c->ctl_zero[0] = c->ctl_zero[1] = false;  // the march kernels zero nothing for later trace launches
    return hipMemsetAsync(c->ctl + c->ctl_cur, 0, first ? sizeof(TraceControl) : offsetof(TraceControl, stats), c->stream);
}

void fill_terrain_args(const tt_ctx* c, uint32_t i, TerrainArgs& a) {
    a.T = c->scene.terrains_host[i];
    a.terrain_index = i;
    a.hmap = c->scene.hmap.p;
    a.map_w = c->scene.hmap_w;
    a.map_h = c->scene.hmap_h;
    a.ctl = c->ctl + c->ctl_cur;
}

// hits_out (nullable, tt_trace_heightmap_hits): the rewritten records also go to the contiguous hit stream
tt_status heightmap_call(tt_ctx* c, const tt_trace_params* p, const uint32_t* n_dev, tt_ray_data* rays, uint32_t* info,
                         tt_stats* stats, uint32_t* hits_out = nullptr) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    if (c->scene.terrains_host.empty()) return fail(c, TT_ERR_NO_SCENE, "no terrain set uploaded (tt_scene_upload_terrains)");
    const tt_call::Path& path = tt_call::kHeightmap;
    const tt_call::Common q = (p && rays) ? tt_call::common_of(*p) : tt_call::Common{};
    if (const tt_call::Refusal r = tt_call::check_shape(path, p && rays, q)) return refused(c, r);
    const tt_call::Plan pl = tt_call::plan_call(path, q, n_dev != nullptr, n_dev && is_device_ptr(n_dev));
    if (pl.refusal) return refused(c, pl.refusal);
    const uint64_t wh = pl.wh;
    const uint32_t off = pl.off;
    const bool dev = pl.dev, async = pl.async, want_stats = pl.want_stats;
    if (hits_out) {  // (the refusals of trace_closest_call's hit-record stream)
        if (!dev) return fail(c, TT_ERR_INVALID_ARG, "a hit-record stream needs TT_TRACE_DEVICE_PTRS");
        if (want_stats) return fail(c, TT_ERR_INVALID_ARG, "tt_trace_heightmap_hits has no TT_TRACE_STATS form");
        if (!is_device_ptr(hits_out)) return fail(c, TT_ERR_INVALID_ARG, "hits_out is not device memory");
        if (reinterpret_cast<uintptr_t>(hits_out) % 16) return fail(c, TT_ERR_INVALID_ARG, "hits_out must be 16-byte aligned");
    }
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (p->n_rays == 0) return TT_OK;
    if (const tt_call::Refusal r = tt_call::check_alignment(path, rays, info)) return refused(c, r);
    TT_HIP(c, hipSetDevice(c->device));
    tt_ray_data* d_rays = rays;
    uint32_t* d_info = info;
    if (dev) {
        if (!is_device_ptr(rays)) return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but rays is not device memory");
    } else {
        TT_HIP(c, stage_in(c, c->st_rays, rays, p->n_rays, off, d_rays));
        if (info) TT_HIP(c, stage_in(c, c->st_info, info, wh * 4, 0, d_info));
    }
    if (want_stats) {
        if (c->st_touched.n < p->n_rays) TT_HIP(c, c->st_touched.alloc(p->n_rays));
        TT_HIP(c, hipMemsetAsync(c->st_touched.p, 0, p->n_rays, c->stream));
    }
    TerrainArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rays = d_rays;
    a.info = d_info;
    a.hits_out = reinterpret_cast<uint4*>(hits_out);
    a.touched = want_stats ? c->st_touched.p : nullptr;
    a.n_rays = p->n_rays;
    a.n_rays_dev = n_dev;
    a.ray_offset = off;
    a.n_pixels = (uint32_t)wh;
    a.bounce = p->bounce;
    a.flags = p->flags;
    const uint32_t grid = terrain_grid(c, want_stats ? 1 : 0, p->n_rays);
    const bool ring = c->timing || !async;  // (a synchronous call reports its kernels' time)
    uint32_t slot;
    TT_HIP(c, reset_terrain_control(c, true));
    TT_HIP(c, ring_open(c, ring, slot));
    for (uint32_t i = 0; i < (uint32_t)c->scene.terrains_host.size(); i++) {  // in order: terrain i + 1 sees i's shortened t
        if (i) TT_HIP(c, reset_terrain_control(c, false));
        fill_terrain_args(c, i, a);
        TT_HIP(c, tt_launch_terrain(&a, 0, want_stats ? 1 : 0, terrain_grid_form() ? 1 : 0, grid, c->stream));
    }
    note_stream_launch(c->stream);
    TT_HIP(c, ring_close(c, ring, slot));
    if (async) return TT_OK;
    TraceControl ctl;
    TT_HIP(c, hipMemcpyAsync(&ctl, c->ctl + c->ctl_cur, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    if (!dev) {
        TT_HIP(c, stage_out(c, rays, d_rays, p->n_rays, off));
        if (info) TT_HIP(c, stage_out(c, info, d_info, wh * 4));
    }
    TT_HIP(c, hipStreamSynchronize(c->stream));
    if (stats) {
        TT_HIP(c, hipEventElapsedTime(&stats->kernel_ms, c->ev0, c->ev1));
        if (want_stats) {
            stats->rays = p->n_rays;
            stats->node_visits = ctl.stats[1];
            stats->hits = ctl.stats[4];
            stats->reps_exhausted = ctl.stats[5];
        }
    }
    return TT_OK;
}

tt_status shadow_heightmap_call(tt_ctx* c, const tt_shadow_params* p, const uint32_t* n_dev, tt_shadow_ray* rays,
                                float* visibility, tt_col_data* colors, float* nee_pos, tt_cache_data* cache) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    if (c->scene.terrains_host.empty()) return fail(c, TT_ERR_NO_SCENE, "no terrain set uploaded (tt_scene_upload_terrains)");
    const tt_call::Path& path = tt_call::kShadowHeightmap;
    const tt_call::Common q = (p && rays) ? tt_call::common_of(*p) : tt_call::Common{};
    if (const tt_call::Refusal r = tt_call::check_shape(path, p && rays, q)) return refused(c, r);
    if (p->flags & TT_SHADOW_VISIBILITY_CHECK)
        return fail(c, TT_ERR_INVALID_ARG, "TT_SHADOW_VISIBILITY_CHECK has no heightmap form (VisabilityCheckCompute never marches terrains)");
    const tt_call::Plan pl = tt_call::plan_call(path, q, n_dev != nullptr, n_dev && is_device_ptr(n_dev));
    if (pl.refusal) return refused(c, pl.refusal);
    const uint64_t wh = pl.wh;
    const bool dev = pl.dev, async = pl.async;
    if (p->n_rays == 0) return TT_OK;
    if (const tt_call::Refusal r = tt_call::check_alignment(path, rays, visibility, nee_pos)) return refused(c, r);
    TT_HIP(c, hipSetDevice(c->device));
    ShadowArrays d{rays, reinterpret_cast<float4*>(visibility), colors, reinterpret_cast<float4*>(nee_pos), cache};
    if (dev) {
        if (!is_device_ptr(rays)) return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but rays is not device memory");
    } else {
        const tt_status st = stage_shadow_in(c, p->n_rays, wh, rays, colors, nee_pos, cache, d);
        if (st != TT_OK) return st;
    }
    // the per-ray visibility record carries "not occluded so far" from one terrain's launch to the next and to
    // the output pass: the caller's array, or the context's scratch (a host array is staged: rays with t == 0
    // keep the caller's values)
    if (!dev || !d.vis) TT_HIP(c, stage_in(c, c->st_vis, visibility, p->n_rays, 0, d.vis));
    TerrainArgs a;
    std::memset(&a, 0, sizeof(a));
    a.srays = d.rays;
    a.vis = d.vis;
    a.n_rays = p->n_rays;
    a.n_rays_dev = n_dev;
    a.n_pixels = (uint32_t)wh;
    a.bounce = p->bounce;
    a.flags = p->flags;
    const uint32_t grid = terrain_grid(c, 2, p->n_rays);
    const bool ring = c->timing || !async;
    uint32_t slot;
    TT_HIP(c, reset_terrain_control(c, true));
    TT_HIP(c, ring_open(c, ring, slot));
    for (uint32_t i = 0; i < (uint32_t)c->scene.terrains_host.size(); i++) {
        if (i) TT_HIP(c, reset_terrain_control(c, false));
        fill_terrain_args(c, i, a);
        TT_HIP(c, tt_launch_terrain(&a, 1, 0, terrain_grid_form() ? 1 : 0, grid, c->stream));
    }
    ShadowArgs o;
    std::memset(&o, 0, sizeof(o));
    o.rays = d.rays;
    o.visibility = d.vis;
    o.colors = d.col;
    o.nee_pos = d.nee;
    o.cache = d.cache;
    o.n_rays = p->n_rays;
    o.n_rays_dev = n_dev;
    o.width = p->screen_width;
    o.height = p->screen_height;
    o.bounce = p->bounce;
    o.flags = p->flags;
    if (d.col || d.nee || d.cache) TT_HIP(c, tt_launch_terrain_shadow_outputs(&o, c->stream));
    note_stream_launch(c->stream);
    TT_HIP(c, ring_close(c, ring, slot));
    if (async) return TT_OK;
    if (!dev) {
        const tt_status st = stage_shadow_out(c, p->n_rays, wh, d, visibility, colors, nee_pos, cache);
        if (st != TT_OK) return st;
    }
    TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

}  // namespace

extern "C" {

tt_status tt_trace_heightmap(tt_ctx* c, const tt_trace_params* p, tt_ray_data* rays, uint32_t* info, tt_stats* stats) {
    return heightmap_call(c, p, nullptr, rays, info, stats);
}

tt_status tt_trace_heightmap_hits(tt_ctx* c, const tt_trace_params* p, tt_ray_data* rays, uint32_t* info,
                                  uint32_t* hits_out) {
    if (!hits_out) return c ? fail(c, TT_ERR_INVALID_ARG, "null hits_out") : TT_ERR_INVALID_ARG;
    return heightmap_call(c, p, nullptr, rays, info, nullptr, hits_out);
}

tt_status tt_trace_heightmap_indirect(tt_ctx* c, const tt_trace_params* p, const uint32_t* n_rays_dev, tt_ray_data* rays,
                                      uint32_t* info) {
    if (!n_rays_dev) return c ? fail(c, TT_ERR_INVALID_ARG, "null device ray count") : TT_ERR_INVALID_ARG;
    return heightmap_call(c, p, n_rays_dev, rays, info, nullptr);
}

tt_status tt_trace_shadow_heightmap(tt_ctx* c, const tt_shadow_params* p, tt_shadow_ray* rays, float* visibility,
                                    tt_col_data* colors, float* nee_pos, tt_cache_data* cache) {
    return shadow_heightmap_call(c, p, nullptr, rays, visibility, colors, nee_pos, cache);
}

tt_status tt_trace_shadow_heightmap_indirect(tt_ctx* c, const tt_shadow_params* p, const uint32_t* n_rays_dev,
                                             tt_shadow_ray* rays, float* visibility, tt_col_data* colors, float* nee_pos,
                                             tt_cache_data* cache) {
    if (!n_rays_dev) return c ? fail(c, TT_ERR_INVALID_ARG, "null device ray count") : TT_ERR_INVALID_ARG;
    return shadow_heightmap_call(c, p, n_rays_dev, rays, visibility, colors, nee_pos, cache);
}

}  // extern "C"
