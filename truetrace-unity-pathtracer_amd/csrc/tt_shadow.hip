// tt_shadow.hip — gfx950 any-hit CWBVH8 visibility traversal (replaces kernel_shadow,
// TrueTrace/Resources/MainCompute/IntersectionKernels.compute:264-505, HardwareRT off).
//
// Same persistent-wave machinery as the closest-hit kernel (tt_trace.hip): per-XCD segment
// dequeues, in-place lane refill, LDS traversal stack. Differences that follow the reference:
//  * the culling distance is the fixed |t| of the shadow ray (max_distance, :366), not a
//    shrinking best hit;
//  * the first occluder ends the ray (:441-454): t = 0 is written back to ShadowRaysBuffer;
//  * triangle_intersect_shadow (CommonData.cginc:593-634) reads the material BEFORE the t-range
//    test and ignores IsBackground / ShadowCaster surfaces; Cutout runs the point-sampled alpha
//    test; glass (specTrans == 1) never occludes and tints the throughput through the texture
//    atlas (stained-glass shadows), in traversal order;
//  * the same cooperative drain phase as the closest-hit kernel (tt_wide.h): once the queue is dry
//    the live rays regroup into 2/4/8-lane groups; a triangle pass tests up to G of the leaf's
//    triangles and the ray is occluded if any of them occludes (what the sequential loop, which
//    stops at the first occluder, concludes as well).
//  * a ray that reaches |t| writes NEEPosA (bounce 0) and the GlobalColors / CacheBuffer
//    accumulations of :457-485 (Direct, Indirect, PrimaryNEERay, CurrentIlluminance; both the
//    RadianceCache and the plain define set, encoders pinned in tt_encode.h);
//  * TT_SHADOW_VISIBILITY_CHECK: VisabilityCheckCompute (CommonData.cginc:710-819) -- the Reps
//    bound counts as visible and only the visibility is written.
#include "tt_encode.h"
#include "tt_launch.h"
#include "tt_wide.h"

namespace {

// triangle_intersect_shadow — CommonData.cginc:593-634. Returns true for an occluder.
// A glass surface (specTrans == 1) never occludes; it multiplies `thr` by its tint (:617-625).
template <bool MATCHECK>
__device__ __forceinline__ bool shadow_triangle(__amdgpu_buffer_rsrc_t tris, const MatView& M, int32_t tri_id,
                                                int32_t mat_offset, const LaneRay& r, float max_distance,
                                                float3& thr) {
    const TriData d = triangle_load<MATCHECK, 0>(tris, tri_id);
    const TriHit h = triangle_hit(d, r);
    const bool in_tri = TT_IN_TRIANGLE(h.u, h.v);
    bool occ = in_tri && (h.t > 0.0f && h.t < max_distance);
    if (MATCHECK && in_tri) {
        // IsBackground / ShadowCaster surfaces never occlude (:612); Cutout with the point sampler
        // (:613-616); out-of-range material = zeros
        const uint32_t mi = (uint32_t)(mat_offset + (int32_t)d.c.y);
        const uint32_t w = mi < M.n_mat ? M.word[mi] : 0u;
        const bool glass = (w >> TT_MATWORD_GLASS) & 1u, cutout = (w >> TT_MATWORD_CUTOUT) & 1u;
        if (((w >> TT_FLAG_IS_BACKGROUND) | (w >> TT_FLAG_SHADOW_CASTER)) & 1u) {
            occ = false;
        } else if (glass || (occ && cutout)) {
            // the alpha test comes first (:616); a glass surface that passes it tints (:621-622)
            const float2 buv = base_uv(M, tri_id, h.u, h.v);
            bool rejected = false;
            if (cutout) {
                const CutoutMat cm = M.cut[mi];
                rejected = sample_point(M, align_uv(buv, cm)) < cm.cutoff;
            }
            if (rejected) {
                occ = false;
            } else if (glass) {
                const float3 f = glass_tint(M, M.glass[mi], buv);
                thr.x = thr.x * f.x;
                thr.y = thr.y * f.y;
                thr.z = thr.z * f.z;
                occ = false;
            }
        }
    }
    return occ;
}

struct ShadowWide : DrainRay {
    float max_distance;
    float3 thr;
};

struct ShadowCounters {
    uint32_t &nodes, &tris, &blas, &occ, &vis, &reps, &ovf;
};

template <int GN>
__device__ __forceinline__ void regroup_shadow(ShadowWide& s, uint64_t lead, uint32_t lane) {
    const uint32_t src = regroup_ray<GN>(s, lead, lane);
    s.max_distance = shfl_f(s.max_distance, src);
    s.thr.x = shfl_f(s.thr.x, src);
    s.thr.y = shfl_f(s.thr.y, src);
    s.thr.z = shfl_f(s.thr.z, src);
}

// The drain loop of the any-hit kernel for groups of G lanes (tt_wide.h's wide_phase with the
// any-hit step): `occlude(st)` / `reach(st)` / `exhaust(st)` write a finished ray's outputs (group's
// first lane only).
template <bool STATS, bool MATCHECK, int G, class Occ, class Reach, class Exh>
__device__ void shadow_wide_phase(const ShadowArgs& A, ShadowWide& st, uint2 (*s_stack)[TT_BLOCK],
                                  uint2* __restrict__ spill, uint32_t spill_stride, __amdgpu_buffer_rsrc_t nodes,
                                  __amdgpu_buffer_rsrc_t tris, uint32_t lane, ShadowCounters C, Occ& occlude,
                                  Reach& reach, Exh& exhaust) {
    const uint32_t sub = lane & (G - 1);
    const uint32_t tid = st.scol, gtid = st.gcol;  // the stack the TT_PUSH / TT_POP macros address
    int32_t& stack_size = st.stack_size;
    while (true) {
        const uint64_t lead = __ballot(st.active && sub == 0u);
        const uint32_t n = (uint32_t)__popcll(lead);
        if (n == 0u) return;
        if constexpr (G < 8) {
            if (n * (2 * G) <= TT_WAVE) {
                regroup_shadow<2 * G>(st, lead, lane);
                shadow_wide_phase<STATS, MATCHECK, 2 * G>(A, st, s_stack, spill, spill_stride, nodes, tris, lane, C,
                                                          occlude, reach, exhaust);
                return;
            }
        }
        // ------------------------------------------------------------- node phase
        if (st.active && st.tg.y == 0u) {
            if (st.Reps >= TT_MAX_REPS) {  // :373 loop bound
                st.active = false;
                if (sub == 0u) {
                    if (STATS) C.reps++;
                    exhaust(st);
                }
            } else if (st.cg.y & 0xff000000u) {  // :374-403
                const uint32_t child = take_child(st.cg, st.oct);
                bool ok = true;
                if (st.cg.y & 0xff000000u) TT_PUSH(st.cg, ok);
                if (ok) {
                    const NodeWords n = load_node<0>(nodes, child);
                    const uint32_t hitmask = group_or<G>(
                        node_intersect_part<G>(n.n0, n.n1, n.n2, n.n3, n.n4, st.ray, st.oct, st.max_distance, sub));
                    st.cg = node_group(hitmask, n, st.NodeOffset);
                    st.tg = tri_group(hitmask, n, st.TriOffset);
                    st.Reps++;
                    if (STATS && sub == 0u) C.nodes++;
                } else {
                    st.active = false;
                    if (sub == 0u) {
                        if (STATS) C.ovf++;
                        TT_REPORT_OVERFLOW(A);
                    }
                }
            } else {  // :404-407
                st.tg = st.cg;
                st.cg = make_uint2(0u, 0u);
            }
            if (st.active && st.tg.y != 0u && st.tlas_ss == -1) {  // :411-435 TLAS leaf -> BLAS
                const uint32_t mo = firstbithigh(st.tg.y);
                st.tg.y &= ~(1u << mo);
                const LeafEntry e = load_leaf_mesh<false>(A.leaf, st.tg.x + mo);
                st.NodeOffset = e.off.y;
                st.TriOffset = e.off.x;
                bool ok = true;
                if (st.tg.y != 0u) TT_PUSH(st.tg, ok);
                if (ok && (st.cg.y & 0xff000000u)) TT_PUSH(st.cg, ok);
                if (ok) {
                    st.tlas_ss = stack_size;
                    st.MatOffset = e.off.z;
                    enter_object_space(e, st.ray, st.oct, st.cg);
                    if (STATS && sub == 0u) C.blas++;
                } else {
                    st.active = false;
                    if (sub == 0u) {
                        if (STATS) C.ovf++;
                        TT_REPORT_OVERFLOW(A);
                    }
                }
                st.tg.y = 0u;
            }
        }

        // --------------------------------------------------------- triangle phase
        // :436-446: highest bit first until the first occluder; lane `sub` takes the sub-th triangle
        if (st.active && st.tg.y != 0u) {
            uint32_t m = st.tg.y;
#pragma unroll
            for (uint32_t k = 0; k + 1 < (uint32_t)G; k++)
                if (k < sub && m) m &= ~(1u << firstbithigh(m));
            const bool has = m != 0u;
            bool occ = false;
            float3 f = make_float3(1.0f, 1.0f, 1.0f);  // this lane's glass tint (1: none)
            if (has)
                occ = shadow_triangle<MATCHECK>(tris, A.mat, (int32_t)(st.tg.x + firstbithigh(m)), st.MatOffset, st.ray,
                                                st.max_distance, f);
            // the first occluder in the reference's order (lowest sub), G if none
            const uint32_t first = (uint32_t)group_min_u64<G>(occ ? (uint64_t)sub : (uint64_t)G);
            if (STATS && sub == 0u)
                C.tris += first < (uint32_t)G ? first + 1u : min((uint32_t)__builtin_popcount(st.tg.y), (uint32_t)G);
            if (first < (uint32_t)G) {  // :449-454
                st.active = false;
                if (sub == 0u) {
                    if (STATS) C.occ++;
                    occlude(st);
                }
            } else {
                if (MATCHECK) {  // the tints in the reference's order (lane k holds the k-th triangle)
                    const uint32_t base = lane & ~(uint32_t)(G - 1);
#pragma unroll
                    for (uint32_t k = 0; k < (uint32_t)G; k++) {
                        st.thr.x = st.thr.x * shfl_f(f.x, base + k);
                        st.thr.y = st.thr.y * shfl_f(f.y, base + k);
                        st.thr.z = st.thr.z * shfl_f(f.z, base + k);
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)G; k++)
                    if (st.tg.y) st.tg.y &= ~(1u << firstbithigh(st.tg.y));
            }
        }

        // ----------------------------------------- advance: pop / finish (:456-494)
        if (st.active && st.tg.y == 0u && (st.cg.y & 0xff000000u) == 0u) {
            if (stack_size != 0) {
                if (stack_size == st.tlas_ss) {
                    leave_blas(A.tlas_base, st.wray, st.NodeOffset, st.TriOffset, st.tlas_ss, st.ray, st.oct);
                }
                TT_POP(st.cg);
            } else {
                st.active = false;
                if (sub == 0u) {
                    if (STATS) C.vis++;
                    reach(st);
                }
            }
        }
    }
}

}  // namespace

// IND: device-resident ray count (tt_trace_shadow_ex_indirect), its own kernel (tt_shadow_kernel_indirect)
template <bool STATS, bool MATCHECK, bool IND>
__device__ __forceinline__ void shadow_body(const ShadowArgs& A) {
    __shared__ uint2 s_stack[TT_LDS_STACK][TT_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint32_t gtid = blockIdx.x * TT_BLOCK + tid;
    const uint32_t spill_stride = gridDim.x * TT_BLOCK;
    uint2* __restrict__ spill = A.spill;
    (void)gtid;
    (void)spill_stride;
    (void)spill;
    const uint32_t lane = tid & (TT_WAVE - 1);

    uint32_t pool_next = 0, pool_end = 0, more = 1;
    const uint32_t wave_id = blockIdx.x * (TT_BLOCK / TT_WAVE) + (tid >> 6);
    SegState S{blockIdx.x % TT_SEGS, 0u, 0u};
    const uint32_t n_rays = IND ? launch_ray_count(A) : A.n_rays;
    const uint32_t n_tiles = (n_rays + 63u) >> 6;
    const __amdgpu_buffer_rsrc_t nodes = buffer_rsrc(A.nodes, A.n_nodes * (uint32_t)TT_NODE_STRIDE);
    const __amdgpu_buffer_rsrc_t tris = buffer_rsrc(A.tris, A.n_tris * (uint32_t)sizeof(TriPos));

    // a lane without a ray holds tg.y == TT_IDLE (as in tt_trace.hip: a live ray's pending-leaf word never
    // has bit 31 set), so each phase test is one compare of tg.y
    constexpr uint32_t TT_IDLE = 0x80000000u;
    uint32_t ray_index = 0;
    LaneRay ray{}, wray{};
    float max_distance = 0.0f;
    float3 thr = make_float3(1.0f, 1.0f, 1.0f);  // throughput (:361), scaled by glass tints
    uint2 cg = make_uint2(0u, 0u), tg = make_uint2(0u, TT_IDLE);
    uint32_t oct = 0;
    int32_t stack_size = 0, tlas_ss = -1;
    int32_t NodeOffset = 0, TriOffset = 0, MatOffset = 0, Reps = 0;
    uint32_t c_nodes = 0, c_tris = 0, c_blas = 0, c_occ = 0, c_rays = 0, c_vis = 0, c_reps = 0, c_ovf = 0;

    // a finished ray's outputs: occluded (:449-454), Reps exhausted (:373), reached the light (:457-485)
    const bool vis_check = (A.flags & TT_SHADOW_VISIBILITY_CHECK) != 0;
    auto do_occlude = [&](uint32_t ri) {
        if (!vis_check) A.rays[ri].t = 0.0f;
        if (A.visibility) A.visibility[ri] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    };
    auto do_exhaust = [&](uint32_t ri) {  // VisabilityCheckCompute returns true once its loop ends
        if (A.visibility)
            A.visibility[ri] = vis_check ? make_float4(1.0f, 1.0f, 1.0f, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    };
    auto do_reach = [&](uint32_t ri, const LaneRay& w, const float3& thr) {  // TerrainExists false
        if (vis_check) {
            if (A.visibility) A.visibility[ri] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            return;
        }
        const tt_shadow_ray& R = A.rays[ri];
        const uint32_t pix = R.PixelIndex;
        const float t = R.t;
        if (A.visibility) A.visibility[ri] = make_float4(thr.x, thr.y, thr.z, 1.0f);
        if (A.bounce == 0 && A.nee_pos && pix / A.width < A.height) {
            const float d = fabsf(t);
            A.nee_pos[pix] = make_float4(w.ox + w.dx * d, w.oy + w.dy * d, w.oz + w.dz * d, 0.0f);
        }
        if (A.bounce == 0 && t >= 0.0f && A.colors && pix / A.width < A.height) {  // Direct (:469)
            tt_col_data& C = A.colors[pix];
            C.Direct[0] = C.Direct[0] + R.illumination[0] * thr.x;
            C.Direct[1] = C.Direct[1] + R.illumination[1] * thr.y;
            C.Direct[2] = C.Direct[2] + R.illumination[2] * thr.z;
        }
        // the rest of :457-485 (CacheBuffer, Indirect, PrimaryNEERay) runs in tt_shadow_accumulate
    };

    while (true) {
        // ---------------------------------------------------------------- refill
        const uint64_t idle = __ballot((int32_t)tg.y < 0);
        // (two 32-bit SALU counts: a 64-bit count is tested with VALU v_cmp_*_u64)
        const uint32_t n_idle = (uint32_t)__builtin_popcount((uint32_t)idle) + (uint32_t)__builtin_popcount((uint32_t)(idle >> 32));
        const bool pool_dry = !more && pool_next >= pool_end;
        if (n_idle == TT_WAVE && pool_dry) break;
#if TT_WIDE
        // the queue is dry and the live rays fit in 2-lane groups: cooperative drain (tt_wide.h)
        if (pool_dry && TT_WAVE - n_idle <= TT_WIDE_ENTER) {
            ShadowWide st{{ray, wray, cg, tg, oct, stack_size, tlas_ss, NodeOffset, TriOffset, MatOffset, Reps,
                           ray_index, tid, gtid, (int32_t)tg.y >= 0},
                          max_distance, thr};
            regroup_shadow<2>(st, __ballot((int32_t)tg.y >= 0), lane);
            auto occ_w = [&](const ShadowWide& w) { do_occlude(w.ray_index); };
            auto reach_w = [&](const ShadowWide& w) { do_reach(w.ray_index, w.wray, w.thr); };
            auto exh_w = [&](const ShadowWide& w) { do_exhaust(w.ray_index); };
            shadow_wide_phase<STATS, MATCHECK, 2>(A, st, s_stack, spill, spill_stride, nodes, tris, lane,
                                                  ShadowCounters{c_nodes, c_tris, c_blas, c_occ, c_vis, c_reps, c_ovf},
                                                  occ_w, reach_w, exh_w);
            break;
        }
#endif
        if (n_idle >= TT_REFILL_MIN && !pool_dry) {
            const uint32_t avail = pool_end - pool_next;
            uint32_t new_base = 0, new_count = 0;
            if (avail < n_idle && more) {
                new_count = sched_reserve(A.ctl, n_rays, n_tiles, lane, n_idle - avail, wave_id, S, new_base);
                more = new_count > 0 ? 1u : 0u;
            }
            const PoolTake pt = pool_take(idle, n_idle, new_base, new_count, pool_next, pool_end, more);
            const uint32_t widx = pt.widx;
            pool_next = pt.pool_next;
            pool_end = pt.pool_end;
            more = pt.more;
            if ((int32_t)tg.y < 0 && widx != 0xffffffffu) {  // :355-371
                ray_index = widx;
                const uint4* rp = reinterpret_cast<const uint4*>(A.rays + ray_index);
                const uint4 r0 = rp[0], r1 = rp[1];
                ray.ox = __uint_as_float(r0.x);
                ray.oy = __uint_as_float(r0.y);
                ray.oz = __uint_as_float(r0.z);
                ray.dx = __uint_as_float(r1.x);
                ray.dy = __uint_as_float(r1.y);
                ray.dz = __uint_as_float(r1.z);
                // |t| (:356); VisabilityCheckCompute takes its dist as given, throughput 0 (:732)
                // canonicalized once per ray: node_intersect's t_max clamp is a plain v_min_f32
                max_distance = __builtin_canonicalizef(vis_check ? __uint_as_float(r1.w)
                                                                 : fabsf(__uint_as_float(r1.w)));
                thr = vis_check ? make_float3(0.0f, 0.0f, 0.0f) : make_float3(1.0f, 1.0f, 1.0f);
                ray.ix = rcp_rn(ray.dx);
                ray.iy = rcp_rn(ray.dy);
                ray.iz = rcp_rn(ray.dz);
                wray = ray;
                oct = octant_inv4(ray);
                cg = make_uint2(A.tlas_base, 0x80000000u);
                tg = make_uint2(0u, 0u);
                stack_size = 0;
                tlas_ss = -1;
                NodeOffset = (int32_t)A.tlas_base;
                TriOffset = 0;
                MatOffset = 0;
                Reps = 0;
                if (STATS) c_rays++;
            }
        }

        // ------------------------------------------------------------- node phase
        if (tg.y == 0u) {
            if (Reps >= TT_MAX_REPS) {  // :373 loop bound: nothing is written
                tg.y = TT_IDLE;
                if (STATS) c_reps++;
                do_exhaust(ray_index);
            } else if (cg.y & 0xff000000u) {  // :374-403
                const uint32_t child = take_child(cg, oct);
                bool ok = true;
                if (cg.y & 0xff000000u) TT_PUSH(cg, ok);
                if (ok) {
                    const NodeWords n = load_node<0>(nodes, child);
                    const uint32_t hitmask = node_intersect(n.n0, n.n1, n.n2, n.n3, n.n4, ray, oct, max_distance);
                    cg = node_group(hitmask, n, NodeOffset);
                    tg = tri_group(hitmask, n, TriOffset);
                    Reps++;
                    if (STATS) c_nodes++;
                } else {
                    tg.y = TT_IDLE;
                    if (STATS) c_ovf++;
                    TT_REPORT_OVERFLOW(A);
                }
            } else {  // :404-407
                tg = cg;
                cg = make_uint2(0u, 0u);
            }
            if ((int32_t)tg.y > 0 && tlas_ss == -1) {  // :411-435 TLAS leaf -> BLAS
                const uint32_t mo = firstbithigh(tg.y);
                tg.y &= ~(1u << mo);
                const LeafEntry e = load_leaf_mesh<false>(A.leaf, tg.x + mo);
                NodeOffset = e.off.y;
                TriOffset = e.off.x;
                bool ok = true;
                if (tg.y != 0u) TT_PUSH(tg, ok);
                if (ok && (cg.y & 0xff000000u)) TT_PUSH(cg, ok);
                tg.y = 0u;
                if (ok) {
                    tlas_ss = stack_size;
                    MatOffset = e.off.z;
                    enter_object_space(e, ray, oct, cg);
                    if (STATS) c_blas++;
                } else {
                    tg.y = TT_IDLE;
                    if (STATS) c_ovf++;
                    TT_REPORT_OVERFLOW(A);
                }
            }
        }

        // --------------------------------------------------------- triangle phase
        if ((int32_t)tg.y > 0) {  // :436-446, highest bit first, until the first occluder
            const uint32_t ti = firstbithigh(tg.y);
            tg.y &= ~(1u << ti);
            const bool occ =
                shadow_triangle<MATCHECK>(tris, A.mat, (int32_t)(tg.x + ti), MatOffset, ray, max_distance, thr);
            if (STATS) c_tris++;
            if (occ) {  // :449-454
                do_occlude(ray_index);
                tg.y = TT_IDLE;
                if (STATS) c_occ++;
            }
        }

        // ----------------------------------------- advance: pop / finish (:456-494)
        if (tg.y == 0u && (cg.y & 0xff000000u) == 0u) {
            if (stack_size != 0) {
                if (stack_size == tlas_ss) {
                    leave_blas(A.tlas_base, wray, NodeOffset, TriOffset, tlas_ss, ray, oct);
                }
                TT_POP(cg);
            } else {  // reached the light (TerrainExists false): :457-485
                do_reach(ray_index, wray, thr);
                tg.y = TT_IDLE;
                if (STATS) c_vis++;
            }
        }
    }

    if (STATS) {
        // stats slots as the closest-hit kernel: rays, nodes, tris, blas, hits (= occluded),
        // reps_exhausted, overflow, accepts (= reached the light)
        const uint32_t v[8] = {wave_sum(c_rays), wave_sum(c_nodes), wave_sum(c_tris), wave_sum(c_blas),
                               wave_sum(c_occ),  wave_sum(c_reps),  wave_sum(c_ovf),  wave_sum(c_vis)};
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (v[k]) atomicAdd(&A.ctl->stats[k], (unsigned long long)v[k]);
        }
    }
}

// ---------------------------------------------------------- :457-485 accumulations (row f1)
// The outputs of a ray that reached |t| beyond Direct / NEEPosA: CacheBuffer.CurrentIlluminance,
// Indirect and PrimaryNEERay, with or without the RadianceCache define (include/truetrace_hip.h).
// A streaming pass over the launch's rays after the traversal, driven by its visibility record
// (throughput.xyz, 1 = reached): it keeps the encoders' registers out of the traversal kernel.
constexpr uint32_t TT_ACC_BLOCK = 256;  // streaming pass: plain 256-thread blocks
__global__ __launch_bounds__(TT_ACC_BLOCK) void tt_shadow_accumulate(ShadowArgs A, const float4* __restrict__ vis) {
    const uint32_t ri = blockIdx.x * TT_ACC_BLOCK + threadIdx.x;
    if (ri >= launch_ray_count(A)) return;
    const float4 v = vis[ri];
    if (v.w != 1.0f) return;
    const tt_shadow_ray& R = A.rays[ri];
    const uint32_t pix = R.PixelIndex;
    if (pix / A.width >= A.height) return;  // out-of-range UAV writes are dropped
    const float t = R.t;
    const bool restir = (A.flags & TT_TRACE_USE_RESTIRGI) != 0;
    const bool rc = (A.flags & TT_SHADOW_RADIANCE_CACHE) != 0;
    const float il[3] = {R.illumination[0], R.illumination[1], R.illumination[2]};
    const float th[3] = {v.x, v.y, v.z};
    if (rc && A.cache) {  // :464
        float k[3] = {1.0f, 1.0f, 1.0f};
        if (!(!restir || t >= 0.0f)) {
            const float3 u = tt_enc::unpackRGBE(__float_as_uint(R.LuminanceIncomming));
            k[0] = u.x;
            k[1] = u.y;
            k[2] = u.z;
        }
        uint32_t& ci = A.cache[pix].CurrentIlluminance;
        const float3 d = tt_enc::DecodeRGB(ci);
        ci = tt_enc::EncodeRGB(d.x + (il[0] * th[0]) * k[0], d.y + (il[1] * th[1]) * k[1], d.z + (il[2] * th[2]) * k[2]);
    }
    if (!A.colors) return;
    tt_col_data& C = A.colors[pix];
    if (t >= 0.0f) {  // :466-474 (Direct at bounce 0 was added by the traversal kernel)
        if (A.bounce != 0 && !rc)
            for (int c = 0; c < 3; c++) C.Indirect[c] = C.Indirect[c] + il[c] * th[c];
        return;
    }
    const bool indirect = rc ? (A.bounce != 0 && (restir || C.Data[3] == (float)A.bounce))  // :477
                             : (A.bounce != 0 && (!restir && C.Data[3] == -1.0f));         // :479
    if (indirect) {
        float k[3] = {1.0f, 1.0f, 1.0f};
        if (rc && restir) {
            const float3 u = tt_enc::unpackRGBE(__float_as_uint(R.LuminanceIncomming));
            k[0] = u.x;
            k[1] = u.y;
            k[2] = u.z;
        }
        for (int c = 0; c < 3; c++) C.Indirect[c] = C.Indirect[c] + (il[c] * th[c]) * k[c];
    } else {  // :481 packRGBE(pow(unpackRGBE(PrimaryNEERay), 2.2f) + pow(illumination, rcp(2.2f)) * throughput)
        const float3 p = tt_enc::unpackRGBE(C.PrimaryNEERay);
        const float pv[3] = {p.x, p.y, p.z};
        const float inv22 = 1.0f / 2.2f;
        float o[3];
        for (int c = 0; c < 3; c++) o[c] = tt_enc::pow_pinned(pv[c], 2.2f) + tt_enc::pow_pinned(il[c], inv22) * th[c];
        C.PrimaryNEERay = tt_enc::packRGBE(o[0], o[1], o[2]);
    }
}

hipError_t tt_launch_shadow_accumulate(const ShadowArgs* a, const float4* vis, hipStream_t st) {
    hipLaunchKernelGGL(tt_shadow_accumulate, dim3((a->n_rays + TT_ACC_BLOCK - 1) / TT_ACC_BLOCK), dim3(TT_ACC_BLOCK), 0,
                       st, *a, vis);
    return hipGetLastError();
}

template <bool STATS, bool MATCHECK>
__global__ TT_BOUNDS void tt_shadow_kernel(ShadowArgs A) {
    shadow_body<STATS, MATCHECK, false>(A);
}
template <bool MATCHECK>
__global__ TT_BOUNDS void tt_shadow_kernel_indirect(ShadowArgs A) {
    shadow_body<false, MATCHECK, true>(A);
}

// ------------------------------------------------------------------ launchers
template <bool S, bool M>
static hipError_t launch_shadow(const ShadowArgs& a, uint32_t grid, hipStream_t st) {
    if constexpr (!S) {
        if (a.n_rays_dev) {
            hipLaunchKernelGGL((tt_shadow_kernel_indirect<M>), dim3(grid), dim3(TT_BLOCK), 0, st, a);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((tt_shadow_kernel<S, M>), dim3(grid), dim3(TT_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t tt_launch_shadow(const ShadowArgs* a, uint32_t grid, hipStream_t st, int stats, int matcheck) {
    if (stats) return matcheck ? launch_shadow<true, true>(*a, grid, st) : launch_shadow<true, false>(*a, grid, st);
    return matcheck ? launch_shadow<false, true>(*a, grid, st) : launch_shadow<false, false>(*a, grid, st);
}

// resident blocks per CU per instantiation, index stats * 2 + matcheck
void tt_shadow_occupancy_table(int* out4) {
    out4[0] = occupancy_of(tt_shadow_kernel<false, false>);
    out4[1] = occupancy_of(tt_shadow_kernel<false, true>);
    out4[2] = occupancy_of(tt_shadow_kernel<true, false>);
    out4[3] = occupancy_of(tt_shadow_kernel<true, true>);
}
