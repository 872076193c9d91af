// tt_trace.hip — gfx950 closest-hit CWBVH8 traversal (replaces kernel_trace,
// TrueTrace/Resources/MainCompute/IntersectionKernels.compute:60-260).
//
// Design (MI355X-first, not a translation of the HLSL dispatch):
//  * persistent waves: grid = CUs x resident blocks; rays are dequeued per wave from per-XCD
//    segment counters, TT_CHUNK_BIG at a time with ONE atomic (the reference pops one ray per
//    thread from a single globally-coherent counter, IntersectionKernels.compute:79-81);
//  * lanes that finish are refilled in place (ballot + mbcnt prefix over idle lanes) so the
//    64-wide wave keeps working instead of idling behind its slowest ray;
//  * the 16-entry uint2 traversal stack lives in LDS, [entry][thread] so a wave's 64 stack
//    accesses hit 64 distinct banks (ds_read_b64/ds_write_b64, conflict-free);
//  * 80-B nodes are five 16-B loads; triangles use a 48-B traversal layout (three 16-B loads)
//    derived from AggTris at upload;
//  * the per-ray visit order, the culling distance and the strict t < best.t acceptance are
//    exactly the reference's, so t / primID / instID are bit-identical to the oracle.
// Numerics follow include/truetrace_hip.h (compiled with -ffp-contract=off).
#include "tt_launch.h"
#include "tt_wide.h"

// TT_REFILL_MIN of the leaf-TLAS kernels (trace_body<LEAF>), whose ray start is cheaper: a knob of its own.
// With the prepared-ray pool (TT_LEAF_POOL) the headline is flat over 14 - 20 and falls below 12 (4: -5 %): a
// refill that only reads a record still costs the wave an iteration with its record writes (profiles/r12/refill/).
#ifndef TT_LEAF_REFILL_MIN
#define TT_LEAF_REFILL_MIN (TT_LEAF_POOL ? 16 : TT_REFILL_MIN)
#endif

namespace {
// :229-241 + set() CommonData.cginc:430-434: the hit record and _PrimaryTriangleInfo of a finished
// ray (wr = the world-space ray, ray2). Returns whether the ray hit something.
// LEAF (the leaf-TLAS kernels): best.mesh_id is not kept. A ray that hit anything hit the launch's one instance
// (inst_mesh / inst_tri_offset, wave-uniform); one that did not has tri_id -1 and mesh 0 as ever. LEAF == 1:
// wr is not kept either, and the bounce forms that need the world ray re-read it from RayData words 0-1, which
// a trace never writes.
template <int INFO, int LEAF = 0>
__device__ __forceinline__ bool write_record(const TraceArgs& A, uint32_t ray_index, uint32_t pix, float col_w,
                                             const Best& best, const LaneRay& wr, int32_t inst_mesh = 0,
                                             int32_t inst_tri_offset = 0) {
    tt_ray_data* R = A.rays + ray_index;
    const int32_t best_mesh = LEAF ? (best.tri_id != -1 ? inst_mesh : 0) : best.mesh_id;
    auto tri_offset_of_best = [&]() -> int32_t {
        if (LEAF) return best.tri_id != -1 ? inst_tri_offset : A.mesh[0].TriOffset;
        return A.mesh[best.mesh_id].TriOffset;
    };
    if (INFO != 0) {
        // (pix % W, pix / W) with pix / W < H is the texel at index pix: no division needed
        if (pix < A.n_pixels) {
            uint4 o;
            bool write = false;
            if (INFO == 1) {
                const int32_t to = tri_offset_of_best();
                o = make_uint4((uint32_t)best_mesh, (uint32_t)(best.tri_id - to),
                               __float_as_uint(best.u), __float_as_uint(best.v));
                write = true;
            } else {
                const float w = col_w;
                if (w == -1.0f || (float)A.bounce == w) {
                    write = true;
                    const bool miss = best.t == A.far_plane;
                    if ((A.flags & TT_TRACE_USE_RESTIRGI) && !miss) {
                        const int32_t to = tri_offset_of_best();
                        o.x = (uint32_t)best_mesh;
                        o.y = (uint32_t)(best.tri_id - to);
                        o.z = (uint32_t)(best.u * 65535.0f) | ((uint32_t)(best.v * 65535.0f) << 16);
                    } else {
                        LaneRay w = wr;
                        if (LEAF == 1) {
                            const uint4* rp = reinterpret_cast<const uint4*>(R);
                            const uint4 r0 = rp[0], r1 = rp[1];
                            w.ox = __uint_as_float(r0.x);
                            w.oy = __uint_as_float(r0.y);
                            w.oz = __uint_as_float(r0.z);
                            w.dx = __uint_as_float(r1.x);
                            w.dy = __uint_as_float(r1.y);
                            w.dz = __uint_as_float(r1.z);
                        }
                        if ((A.flags & TT_TRACE_USE_ASVGF) || !miss) {
                            o.x = __float_as_uint(w.dx);
                            o.y = __float_as_uint(w.dy);
                            o.z = __float_as_uint(w.dz);
                        } else {
                            o.x = __float_as_uint(w.dx * best.t + w.ox);
                            o.y = __float_as_uint(w.dy * best.t + w.oy);
                            o.z = __float_as_uint(w.dz * best.t + w.oz);
                        }
                    }
                    o.w = miss ? 1u : 0u;
                }
            }
            if (write) reinterpret_cast<uint4*>(A.info)[pix] = o;
        }
    }
    const uint32_t uv = (uint32_t)(best.u * 65535.0f) | ((uint32_t)(best.v * 65535.0f) << 16);
    const uint4 hit = make_uint4((uint32_t)best_mesh, (uint32_t)best.tri_id, __float_as_uint(best.t), uv);
    reinterpret_cast<uint4*>(R)[2] = hit;
    if (A.hits_out) {  // the compact record stream (multi-GPU gather): a raw buffer store, 32-bit offset
        const u32x4 v = {hit.x, hit.y, hit.z, hit.w};
        __builtin_amdgcn_raw_buffer_store_b128(v, buffer_rsrc(A.hits_out, 0x7fffffff), (ray_index - A.ray_offset) << 4,
                                               0, 0);
    }
    return best.t != A.far_plane;
}

// A ray that ends without a record (the Reps bound, IntersectionKernels.compute:155, or a stack
// overflow) leaves RayData.hits as it was; the compact stream (tt_trace_closest_hits) promises the
// same bytes as RayData.hits, so it gets the unchanged word (a rare path: one 16-B load).
__device__ __forceinline__ void keep_record(const TraceArgs& A, uint32_t ray_index) {
    if (A.hits_out) {
        const uint4 h = reinterpret_cast<const uint4*>(A.rays + ray_index)[2];
        const u32x4 v = {h.x, h.y, h.z, h.w};
        __builtin_amdgcn_raw_buffer_store_b128(v, buffer_rsrc(A.hits_out, 0x7fffffff), (ray_index - A.ray_offset) << 4,
                                               0, 0);
    }
}

// TT_TRACE_ADAPTIVE_ORDER: a finished (or Reps-exhausted) ray's cost -- its Reps count -- into its
// ray chunk's entry of the launch's cost map (no-return atomic max; tt_order.hip sorts the next
// launch's chunks by it). The ray chunk is the 8x8 pixel tile in the full-frame swizzle, else
// (ray index - offset) / 64. Rays below TT_ORDER_MIN_REPS skip the atomic: chunks whose rays are all
// cheap keep cost 0 and their natural order, and a launch issues few atomics.
static_assert(TT_CHUNK_BIG == 64, "the adaptive order maps one dequeue (TT_CHUNK_BIG rays) to one 64-ray chunk");
#ifndef TT_ORDER_MIN_REPS
#define TT_ORDER_MIN_REPS 32
#endif
__device__ __forceinline__ void record_chunk_cost(const TraceArgs& A, bool swizzle, uint32_t ray_index, int32_t reps) {
    if (reps < TT_ORDER_MIN_REPS) return;
    const uint32_t local = ray_index - A.ray_offset;
    uint32_t c = local >> 6;
    if (swizzle) {
        const uint32_t py = fastdiv(local, A.div_width), px = local - py * A.width;
        c = (py >> 3) * (A.width >> 3) + (px >> 3);
    }
    atomicMax(A.chunk_cost + c, (uint32_t)reps);
}
}  // namespace


// TT_ROOT_LEAF (TraceArgs::root, tt_device.h): the root of a one-leaf TLAS is stepped when a ray starts
// and the TLAS leaf -> BLAS switch follows before the loop's node step, so the ray's first node step in
// the loop is already its BLAS root (one loop iteration less per ray).
namespace {
// node_intersect (tt_traverse.h) for the root's one child: the same operations in the same order
__device__ __forceinline__ bool root_leaf_hit(const RootLeaf& R, const LaneRay& r, float max_distance) {
    const float adjx = __uint_as_float(rl_byte(R.e, 0) << 23) * r.ix;
    const float adjy = __uint_as_float(rl_byte(R.e, 1) << 23) * r.iy;
    const float adjz = __uint_as_float(rl_byte(R.e, 2) << 23) * r.iz;
    const float orgx = r.ix * (R.px - r.ox);
    const float orgy = r.iy * (R.py - r.oy);
    const float orgz = r.iz * (R.pz - r.oz);
    const bool nx = r.dx < 0.0f, ny = r.dy < 0.0f, nz = r.dz < 0.0f;
    const uint32_t x_min = rl_byte(nx ? R.qhi : R.qlo, 0), x_max = rl_byte(nx ? R.qlo : R.qhi, 0);
    const uint32_t y_min = rl_byte(ny ? R.qhi : R.qlo, 1), y_max = rl_byte(ny ? R.qlo : R.qhi, 1);
    const uint32_t z_min = rl_byte(nz ? R.qhi : R.qlo, 2), z_max = rl_byte(nz ? R.qlo : R.qhi, 2);
    const float tminx = fma_((float)x_min, adjx, orgx);
    const float tminy = fma_((float)y_min, adjy, orgy);
    const float tminz = fma_((float)z_min, adjz, orgz);
    const float tmaxx = fma_((float)x_max, adjx, orgx);
    const float tmaxy = fma_((float)y_max, adjy, orgy);
    const float tmaxz = fma_((float)z_max, adjz, orgz);
    const float tmin = fmaxf(fmaxf(tminx, tminy), fmaxf(tminz, 1e-8f));
    float tmaxz_c;
    asm("v_min_f32 %0, %1, %2" : "=v"(tmaxz_c) : "v"(tmaxz), "v"(max_distance));
    const float tmax = fminf(fminf(tmaxx, tmaxy), tmaxz_c);
    return tmin < tmax;
}
}  // namespace


// INFO: 0 = no _PrimaryTriangleInfo, 1 = bounce 0 form, 2 = bounce > 0 form (GlobalColors).
// IND: the ray count is device-resident (tt_trace_closest_indirect): instantiated as its own kernel
// (tt_trace_kernel_indirect), so the direct launches keep exactly their code and kernel names.
// ORD: TT_TRACE_ADAPTIVE_ORDER (tt_trace_kernel_ord): chunks are dequeued in A.order (when set) and
// every ray's Reps count goes into the tile cost map.
// LEAF: the leaf-TLAS form (tt_trace_leaf_kernel<IND, INFO>) for launches whose TLAS root
// is one leaf holding one instance (root_one_instance; C2, C3, C5). Every ray that hits the root's box switches
// to the same BLAS through the same LeafMesh record and never leaves it (the switch pushes nothing, so the
// BLAS-exit test `stack_size == tlas_ss` could only hold at stack_size 0, where the ray finishes). The record
// is read once per wave at a wave-uniform address (scalar loads; from device memory at every launch, so
// tt_scene_update_meshdata is honoured as in the generic kernel), the offsets and the mesh id are wave-uniform,
// and no lane keeps tlas_ss, best.mesh_id or (LEAF == 1; LEAF == 2 keeps it for the INFO = 2 record) the world
// ray: fewer VGPRs (more resident waves), a cheaper ray start, no TLAS-leaf test after a node step and no
// BLAS-exit test in the advance. The arithmetic of a ray and its order are the generic kernel's, so results are
// bit-identical. Never with STATS, MATCHECK or ORD. With TT_LEAF_POOL the ray start runs once per dequeued chunk,
// for all 64 rays at full wave width, into a per-wave pool in LDS that the refills read (POOL below).
template <bool STATS, bool MATCHECK, int INFO, bool IND, bool ORD, int LEAF = 0>
__device__ __forceinline__ void trace_body(const TraceArgs& A) {
    static_assert(!LEAF || (!STATS && !MATCHECK && !ORD), "the leaf-TLAS form has no stats / material / order variants");
    // POOL (the leaf-TLAS form, TT_LEAF_POOL): the rays of a dequeued chunk are set up by all 64 lanes at once into
    // s_pool, one 48-B record per ray as three 16-B words [word][slot]: (o.xyz, d.x) (d.yz, i.xy) (i.z, PixelIndex,
    // Data.w, octant | root hit << 31), o / d / i the ray in the instance's object space. A refilled lane reads the
    // record of its slot (slot = work index & 63: a reservation is one chunk-aligned chunk of TT_CHUNK_BIG rays).
    // ROOTSTEP (TT_LEAF_ROOT_STEP): the setup also makes the ray's first node step of the loop -- the BLAS root, L.off.w,
    // with t_max = FarPlane, the same node for every ray of the launch -- at full width, from wave-uniform loads of
    // the node. The step's child base, triangle base and imask are wave-uniform, so the record stays 48 B: word 10 is
    // octant | root box hit << 31 and word 11 the step's 32-bit hit mask (0 for a ray that missed the root's box).
    // Data.w (INFO 2), whose place that takes, is only ever tested by write_record: the setup makes the test and a
    // ray that fails it carries PixelIndex 0xffffffff, which writes no texel either. A refilled lane starts after
    // the step: Reps 2, the hit inner children in cg and the hit leaf triangles in tg, or an empty group.
    // (TT_LEAF_READY_STATE: word 10 is instead octant byte | imask-or-0 << 8 | Reps << 16, see READY below.)
    constexpr bool POOL = LEAF != 0 && TT_LEAF_POOL != 0;
    constexpr bool ROOTSTEP = POOL && TT_LEAF_ROOT_STEP != 0;
    // RESTART (TT_LEAF_RESTART): a lane whose ray finishes while the pool holds prepared rays takes the next one in
    // the same advance block. The finished ray's result is parked in the slot just consumed -- word 0: (tri_id, t, u,
    // v), word 1: (work index, PixelIndex) -- and bit `slot` of the wave-uniform mask `parked` is set; lane s writes
    // the record of slot s, through write_record, before a chunk setup overwrites the pool, before the cooperative
    // drain and at the loop's exit. A lane's ray_index holds the ray's WORK index (ray_of() maps it where a record
    // is written), and the INFO 2 record's world ray is read back from RayData words 0-1 by the full-width write
    // (the form LEAF == 1), so no lane keeps it.
    constexpr bool RESTART = ROOTSTEP && TT_LEAF_RESTART != 0;
    static_assert(!RESTART || LEAF == 1, "the restart parks no world ray: the record write reads it back");
    // The restart form's bookkeeping knobs (tt_traverse.h): READY, the pool record's words 10 / 11 ready-made
    // (word 10: octant byte | imask-or-0 << 8 | Reps << 16); MASKB, ballots from the lane mask; POPLAST, the advance
    // pops after the restart; EMPTYG, the node phase's empty-group branch writes nothing.
    constexpr bool READY = RESTART && TT_LEAF_READY_STATE != 0;
    constexpr bool MASKB = RESTART && TT_LEAF_MASK_BALLOT != 0;
    constexpr bool POPLAST = RESTART && TT_LEAF_POP_LAST != 0;
    constexpr bool EMPTYG = RESTART && TT_LEAF_EMPTY_GROUP != 0;
    constexpr int tt_lds_depth = lds_depth_of<LEAF>();  // the LDS part of the stack (TT_PUSH / TT_POP)
    static_assert(!POOL || TT_CHUNK_BIG == TT_WAVE, "the prepared-ray pool holds one chunk, one slot per lane");
    __shared__ uint2 s_stack[tt_lds_depth][TT_BLOCK];
    __shared__ uint4 s_pool[POOL ? 3 : 1][TT_BLOCK];
    (void)s_pool;
    // (read before the kernel's first store, so the compiler can prove the loads unclobbered and make them scalar)
    LeafEntry L{};  // LEAF: the LeafMesh record of the one instance
    if (LEAF) L = load_leaf_mesh<true>(A.leaf, A.root.base_tri + firstbithigh(A.root.bits));
    // ROOTSTEP: the wave-uniform words of the BLAS root's step that a refill needs (node_group / tri_group): the child
    // and triangle bases and the imask. The whole node is read again by each chunk setup and lives only there.
    uint32_t root_cg_x = 0, root_tg_x = 0, root_imask = 0;
    if (ROOTSTEP) {
        const NodeWords n = load_node_uniform(A.nodes, A.n_nodes, (uint32_t)L.off.w);
        root_cg_x = n.n1.x + (uint32_t)L.off.y;
        root_tg_x = n.n1.y + (uint32_t)L.off.x;
        root_imask = n.n0.w >> 24;
    }
    const uint32_t tid = threadIdx.x;
    zero_next_control(A.ctl_next, tid);
    const uint32_t gtid = blockIdx.x * TT_BLOCK + tid;
    const uint32_t spill_stride = gridDim.x * TT_BLOCK;
    uint2* __restrict__ spill = A.spill;
    (void)gtid;
    (void)spill_stride;
    (void)spill;
    const uint32_t lane = tid & (TT_WAVE - 1);
#ifdef TT_DIAG_BLOCKS
    if (tid < TT_DB_N) tt_db[tid] = 0ull;
    __syncthreads();
#endif

    // wave-uniform scheduler state: a private pool [pool_next, pool_end) of work indices, refilled
    // from segment `seg` (segments = contiguous 1/TT_SEGS slices of the work range, dealt to XCD
    // groups by blockIdx % TT_SEGS for L2 locality; exhausted segments are stolen from in turn)
    uint32_t pool_next = 0, pool_end = 0, more = 1;
    const uint32_t wave_id = blockIdx.x * (TT_BLOCK / TT_WAVE) + (tid >> 6);
    SegState S{blockIdx.x % TT_SEGS, 0u, 0u};
    const uint32_t n_rays = IND ? launch_ray_count(A) : A.n_rays;
    const uint32_t n_tiles = (n_rays + 63u) >> 6;
    // work index -> ray index in 8x8 screen tiles: full-frame primary batches only (a device count
    // decides at run time)
    const bool swizzle = IND ? (A.tile_swizzle && n_rays == A.n_pixels) : (A.tile_swizzle != 0u);
    const __amdgpu_buffer_rsrc_t nodes = buffer_rsrc(A.nodes, A.n_nodes * (uint32_t)TT_NODE_STRIDE);
    const __amdgpu_buffer_rsrc_t tris = buffer_rsrc(A.tris, A.n_tris * (uint32_t)sizeof(TriPos));

    // lane traversal state (IntersectionKernels.compute:62-77). A lane without a ray (idle, finished or
    // ended) holds tg.y == TT_IDLE: the pending-leaf word of a live ray never has bit 31 set (hit bits
    // 0-23 only), so "active" needs no register of its own and every phase test of the loop is one
    // compare of tg.y: at the loop top (tg.y == 0), leaf triangles pending ((int)tg.y > 0), idle (< 0).
    constexpr uint32_t TT_IDLE = 0x80000000u;
    uint32_t ray_index = 0;
    uint32_t pix = 0;    // RayData.PixelIndex, kept from the ray load
    float col_w = 0.0f;  // GlobalColors[pix].Data.w (INFO == 2), loaded when the ray starts
    bool pending = false;  // finished, record not yet written (TT_DEFER_FINISH)
    LaneRay ray{}, wray{};
    Best best{};
    uint2 cg = make_uint2(0u, 0u), tg = make_uint2(0u, TT_IDLE);
    uint32_t oct = 0;
    int32_t stack_size = 0, tlas_ss = -1;
    int32_t NodeOffset = 0, TriOffset = 0, MatOffset = 0, mesh_id = -1, Reps = 0;
    if (LEAF) {  // wave-uniform for the whole launch
        NodeOffset = L.off.y;
        TriOffset = L.off.x;
        MatOffset = L.off.z;
        mesh_id = L.mesh_id;
    }
    uint32_t c_nodes = 0, c_tris = 0, c_blas = 0, c_acc = 0, c_rays = 0, c_hits = 0, c_reps = 0, c_ovf = 0;
    uint32_t d_iter = 0, d_node_lanes = 0, d_node_iters = 0, d_tri_lanes = 0, d_tri_iters = 0, d_active_lanes = 0;
    uint32_t d_lead_same = 0, d_uniform = 0;  // node-step uniformity (lanes sharing the first lane's node)
    // the world-space ray (ray2, IntersectionKernels.compute:151), kept in registers
    auto world_ray = [&]() -> LaneRay { return wray; };
    // POOL: work index -> ray index (8x8 screen tiles for full-frame primary batches), as the per-lane setup has it
    auto ray_of = [&](uint32_t widx) -> uint32_t {
        uint32_t local = widx;
        if (swizzle) {
            const uint32_t tw = A.width >> 3;
            const uint32_t t = widx >> 6, l = widx & 63u;
            const uint32_t ty = fastdiv(t, A.div_tiles), tx = t - ty * tw;
            local = (ty * 8u + (l >> 3)) * A.width + tx * 8u + (l & 7u);
        }
        return A.ray_offset + local;
    };
    (void)ray_of;
    // RESTART: bit s = slot s of the pool holds a parked result (wave-uniform)
    uint64_t parked = 0ull;
    (void)parked;
    // the ray index of a lane's ray_index word (RESTART keeps the work index there)
    auto ray_index_of = [&](uint32_t v) -> uint32_t {
        if constexpr (RESTART) return ray_of(v);
        return v;
    };

#if TT_ROOT_LEAF
    const bool rl_ok = A.root.ok != 0u;  // a kernel argument: wave-uniform
#endif
    // :194-219 TLAS leaf -> BLAS (the lane is at TLAS level with pending leaf bits in tg)
    auto enter_blas = [&]() {
            TT_DB(8);
            const uint32_t mo = firstbithigh(tg.y);
            tg.y &= ~(1u << mo);
            const LeafEntry e = load_leaf_mesh<true>(A.leaf, tg.x + mo);
            mesh_id = e.mesh_id;
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
                keep_record(A, ray_index);
            }
    };
    // :229-241: the finished ray's hit record and _PrimaryTriangleInfo
    auto finish_ray = [&]() {
        const bool hit = write_record<INFO, LEAF>(A, ray_index_of(ray_index), pix, READY ? -1.0f : col_w, best, world_ray(),
                                                  mesh_id, TriOffset);
        if (STATS) c_hits += hit ? 1u : 0u;
        (void)hit;
        if (ORD) record_chunk_cost(A, swizzle, ray_index, Reps);
    };
    // POOL: a lane's start on work index widx from the pool record of its slot
    // (zero_stack false: the caller knows stack_size is 0 -- a lane that finishes has an empty stack)
    auto start_from = [&](const uint32_t widx, const uint4 p0, const uint4 p1, const uint4 p2, const bool zero_stack) {
        TT_DL(19, true);
        ray_index = RESTART ? widx : ray_of(widx);
        ray.ox = __uint_as_float(p0.x);
        ray.oy = __uint_as_float(p0.y);
        ray.oz = __uint_as_float(p0.z);
        ray.dx = __uint_as_float(p0.w);
        ray.dy = __uint_as_float(p1.x);
        ray.dz = __uint_as_float(p1.y);
        ray.ix = __uint_as_float(p1.z);
        ray.iy = __uint_as_float(p1.w);
        ray.iz = __uint_as_float(p2.x);
        pix = p2.y;
        if (READY) {
            // words 10 / 11 as the setup left them for this: one instruction per value (col_w is not kept: the
            // setup has made write_record's test of Data.w and the record writes pass -1)
            oct = __builtin_amdgcn_perm(p2.z, p2.z, 0u);  // the octant byte in all four
            cg = make_uint2(root_cg_x, __builtin_amdgcn_perm(p2.w, p2.z, 0x070c0c01u));  // hit inner children | imask, or 0
            tg = make_uint2(root_tg_x, p2.w & 0x00ffffffu);
            Reps = (int32_t)(p2.z >> 16);
        } else if (ROOTSTEP) {
            col_w = -1.0f;  // (the setup has made write_record's test of Data.w: see there)
            oct = p2.z & 0x7fffffffu;
            // node_group / tri_group of the setup's step. Without a hit inner child the node group is
            // empty -- in the loop the advance follows such a step at once, here the node phase comes
            // first -- and so is a ray's that missed the root's box (mask 0): the advance finishes it
            const uint32_t inner = p2.w & 0xff000000u;
            cg = make_uint2(root_cg_x, inner ? (inner | root_imask) : 0u);
            tg = make_uint2(root_tg_x, p2.w & 0x00ffffffu);
            Reps = (p2.z & 0x80000000u) ? 2 : 1;
        } else {
            col_w = __uint_as_float(p2.z);
            oct = p2.w & 0x7fffffffu;
            // a ray that missed the root's box starts with the empty group: the advance finishes it
            cg = make_uint2((p2.w & 0x80000000u) ? (uint32_t)L.off.w : 0u, p2.w & 0x80000000u);
        }
        if (LEAF == 2) {  // the world ray of the INFO = 2 record: the chunk's setup has just read the lines
            const uint4* rp = reinterpret_cast<const uint4*>(A.rays + ray_index);
            const uint4 r0 = rp[0], r1 = rp[1];
            wray.ox = __uint_as_float(r0.x);
            wray.oy = __uint_as_float(r0.y);
            wray.oz = __uint_as_float(r0.z);
            wray.dx = __uint_as_float(r1.x);
            wray.dy = __uint_as_float(r1.y);
            wray.dz = __uint_as_float(r1.z);
        }
        best.t = A.far_plane;
        best.u = 0.0f;
        best.v = 0.0f;
        best.mesh_id = 0;
        best.tri_id = -1;
        if (!ROOTSTEP) tg = make_uint2(0u, 0u);
        if (zero_stack) stack_size = 0;
        if (!ROOTSTEP) Reps = 1;
    };
    (void)start_from;
    // (the leaf form's ray start is cheaper, so its refill threshold is a knob of its own)
    constexpr uint32_t REFILL_MIN = LEAF ? TT_LEAF_REFILL_MIN : TT_REFILL_MIN;
    while (true) {
        TT_DB(0);
        // ---------------------------------------------------------------- refill
        const uint64_t idle = lane_mask<MASKB>((int32_t)tg.y < 0);
        // (two 32-bit counts: written as __popcll, the compiler keeps the count 64-bit and tests it with two
        // VALU v_cmp_*_u64 per iteration)
        const uint32_t n_idle = (uint32_t)__builtin_popcount((uint32_t)idle) + (uint32_t)__builtin_popcount((uint32_t)(idle >> 32));
        const bool pool_dry = !more && pool_next >= pool_end;
#if TT_DRAIN_PRIO
        // a draining wave issues ahead of the waves of launches still in their bulk (other parts / frames)
        if (pool_dry) __builtin_amdgcn_s_setprio(TT_DRAIN_PRIO);
#endif
        // the queue is dry and the live rays fit in 2-lane groups: cooperative drain (tt_wide.h)
        const bool to_wide = TT_WIDE && pool_dry && n_idle < TT_WAVE && TT_WAVE - n_idle <= TT_WIDE_ENTER;
        // RESTART: lanes only idle for want of a prepared ray, so the pool-empty case has a threshold of its own
        // (the few lanes a Reps bound or a stack overflow idles wait as before while the pool holds rays)
        const uint32_t refill_min = RESTART && pool_next >= pool_end ? (uint32_t)TT_LEAF_RESTART_MIN : REFILL_MIN;
        // finished rays write their records in batches, right before their lanes are refilled
        if ((n_idle == TT_WAVE && pool_dry) || (n_idle >= refill_min && !pool_dry) || to_wide) {
            if (pending) {
                TT_DB(1);
                finish_ray();
                pending = false;
            }
            if constexpr (RESTART) {
                // the parked results, at full width: lane s writes the record of slot s. Before the refill below
                // overwrites the pool, before the drain regroups the lanes and before the wave ends.
                if (parked != 0ull) {
                    TT_DB(34);
                    if ((parked >> lane) & 1ull) {
                        TT_DL(35, true);
                        const uint4 k0 = s_pool[0][tid];
                        const uint2 k1 = reinterpret_cast<const uint2*>(&s_pool[1][tid])[0];
                        Best kb;
                        kb.tri_id = (int32_t)k0.x;
                        kb.t = __uint_as_float(k0.y);
                        kb.u = __uint_as_float(k0.z);
                        kb.v = __uint_as_float(k0.w);
                        kb.mesh_id = 0;
                        write_record<INFO, LEAF>(A, ray_of(k1.x), k1.y, -1.0f, kb, LaneRay{}, mesh_id, TriOffset);
                    }
                    parked = 0ull;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        if (n_idle == TT_WAVE && pool_dry) break;
#if TT_WIDE
        if (to_wide) {
            TT_DB(13);
            WideState st{{ray, world_ray(), cg, tg, oct, stack_size, tlas_ss, NodeOffset, TriOffset, MatOffset, Reps,
                          ray_index_of(ray_index), tid, gtid, (int32_t)tg.y >= 0},
                         best, mesh_id, pix, READY ? -1.0f : col_w};
            regroup<2, LEAF>(st, __ballot((int32_t)tg.y >= 0), lane);
            auto finish_wide = [&](const WideState& w) {
                const bool hit = write_record<INFO, LEAF>(A, w.ray_index, w.pix, w.col_w, w.best, w.wray, mesh_id, TriOffset);
                if (STATS) c_hits += hit ? 1u : 0u;
                if (ORD) record_chunk_cost(A, swizzle, w.ray_index, w.Reps);
            };
            auto exhaust_wide = [&](const WideState& w, bool overflow) {
                keep_record(A, w.ray_index);
                // (an overflowed ray records no cost, as in the narrow loop: only the Reps bound does)
                if (ORD && !overflow) record_chunk_cost(A, swizzle, w.ray_index, w.Reps);
            };
            wide_phase<STATS, MATCHECK, 2, LEAF>(A, st, s_stack, spill, spill_stride, nodes, tris, lane,
                                           Counters{c_nodes, c_tris, c_blas, c_acc, c_hits, c_reps, c_ovf},
                                           finish_wide, exhaust_wide);
            break;
        }
#endif
        if (n_idle >= refill_min && !pool_dry) {
            TT_DB(2);
#if TT_LONG_PRIO
            // a wave carrying a long ray (>= TT_LONG_PRIO node steps so far) issues ahead of the others until
            // its next refill without one: the long ray's dependent chain, not the wave's share of issue,
            // is what sets a small launch's length (the degenerate-direction rays)
            if (lane_mask<MASKB>((int32_t)tg.y >= 0 && Reps >= TT_LONG_PRIO) != 0ull) __builtin_amdgcn_s_setprio(TT_LONG_PRIO_LEVEL);
            else __builtin_amdgcn_s_setprio(0);
#endif
            // wave-uniform: take from the wave's pool first, then one dequeue for the rest
            const uint32_t avail = pool_end - pool_next;
            uint32_t new_base = 0, new_count = 0;
            if (avail < n_idle && more) {
                new_count = sched_reserve(A.ctl, n_rays, n_tiles, lane, n_idle - avail, wave_id, S, new_base);
                more = new_count > 0 ? 1u : 0u;
                if constexpr (RESTART && TT_LEAF_UNIFORM_SEG != 0) {  // the segment state too is the wave's, not a lane's
                    S.seg = __builtin_amdgcn_readfirstlane(S.seg);
                    S.dead = __builtin_amdgcn_readfirstlane(S.dead);
                }
                // a reservation is one whole 64-ray work chunk (TT_CHUNK_BIG, chunk-aligned segments): the
                // adaptive order maps it to the ray chunk it dequeues (one wave-uniform load)
                if (ORD && A.order && new_count > 0)
                    new_base = (__builtin_amdgcn_readfirstlane(A.order[new_base >> 6]) << 6) | (new_base & 63u);
            }
            const PoolTake pt = pool_take<TT_UNIFORM_POOL != 0>(idle, n_idle, new_base, new_count, pool_next, pool_end, more);
            const uint32_t widx = pt.widx;
            pool_next = pt.pool_next;
            pool_end = pt.pool_end;
            more = pt.more;
            if constexpr (POOL) {
                const uint32_t pcol = tid - lane;  // the wave's pool columns
                const bool take = (int32_t)tg.y < 0 && widx != 0xffffffffu;
                // slots left from the previous chunk are read before the new chunk overwrites the pool
                const bool take_left = take && lane_prefix(idle) < min(avail, n_idle);
                auto start_ray = [&](const uint4 p0, const uint4 p1, const uint4 p2) { start_from(widx, p0, p1, p2, true); };
                uint4 p0 = make_uint4(0u, 0u, 0u, 0u), p1 = p0, p2 = p0;
                if (take_left) {
                    const uint32_t slot = pcol + (widx & 63u);
                    p0 = s_pool[0][slot];
                    p1 = s_pool[1][slot];
                    p2 = s_pool[2][slot];
                    // ROOTSTEP: started here, so that the record is not held in registers across the setup
                    if (ROOTSTEP) start_ray(p0, p1, p2);
                }
                // (one wave owns the pool and its LDS accesses execute in order: these only keep the compiler from
                // moving the reads and writes of different lanes' slots across each other)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (new_count > 0) {  // wave-uniform: every lane, busy or idle, sets up ray new_base + lane
                    TT_DB(4);
                    uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0, q2 = q0;
                    NodeWords rn{};  // ROOTSTEP: the BLAS root, from device memory at every setup, in SGPRs
                    if (ROOTSTEP) rn = load_node_uniform(A.nodes, A.n_nodes, (uint32_t)L.off.w);
                    if (lane < new_count) {  // (all 64 but in a launch's last chunk)
                        const uint4* rp = reinterpret_cast<const uint4*>(A.rays + ray_of(new_base + lane));
                        const uint4 r0 = rp[0], r1 = rp[1];
                        float cw = 0.0f;
                        if (INFO == 2) cw = (r0.w < A.n_pixels) ? A.colors[r0.w].Data[3] : 0.0f;
                        LaneRay r;
                        r.ox = __uint_as_float(r0.x);
                        r.oy = __uint_as_float(r0.y);
                        r.oz = __uint_as_float(r0.z);
                        r.dx = __uint_as_float(r1.x);
                        r.dy = __uint_as_float(r1.y);
                        r.dz = __uint_as_float(r1.z);
                        r.ix = rcp_rn(r.dx);
                        r.iy = rcp_rn(r.dy);
                        r.iz = rcp_rn(r.dz);
                        // the root's node step; a hit is the TLAS leaf -> BLAS switch (nothing to push)
                        uint32_t o = 0u;
                        uint2 g = make_uint2(0u, 0u);
                        const bool root_hit = root_leaf_hit(A.root, r, A.far_plane);
                        TT_DL(29, root_hit);
                        if (root_hit) enter_object_space(L, r, o, g);
                        q0 = make_uint4(__float_as_uint(r.ox), __float_as_uint(r.oy), __float_as_uint(r.oz),
                                        __float_as_uint(r.dx));
                        q1 = make_uint4(__float_as_uint(r.dy), __float_as_uint(r.dz), __float_as_uint(r.ix),
                                        __float_as_uint(r.iy));
                        q2 = make_uint4(__float_as_uint(r.iz), r0.w, __float_as_uint(cw), o | g.y);
                        if (ROOTSTEP) {
                            // write_record's test of Data.w (INFO 2) is made here: where it fails the record carries
                            // no pixel (a PixelIndex past the frame writes no texel either)
                            if (INFO == 2 && !(cw == -1.0f || (float)A.bounce == cw)) q2.y = 0xffffffffu;
                            // READY: Reps is 2 after the step, 1 where the ray missed the root's box (o is 0 there)
                            q2.z = READY ? ((o & 0xffu) | (root_hit ? 0x20000u : 0x10000u)) : (o | g.y);
                            q2.w = 0u;
                            // (the record goes out before the step, which then holds only what it reads; the step
                            // adds its mask)
                            s_pool[0][tid] = q0;
                            s_pool[1][tid] = q1;
                            s_pool[2][tid] = q2;
                            // the BLAS root's node step, as the loop would make it first (best.t is FarPlane there)
                            if (root_hit) {
                                TT_DB(28);
                                const uint32_t hm = node_intersect(rn.n0, rn.n1, rn.n2, rn.n3, rn.n4, r, o, A.far_plane);
                                if (READY) {  // the node group of a step that hit no inner child is empty: no imask
                                    // (the imask of this setup's own read of the root: no lane needs root_imask then)
                                    const uint32_t im = (hm & 0xff000000u) ? (rn.n0.w >> 24) << 8 : 0u;
                                    reinterpret_cast<uint2*>(&s_pool[2][tid])[1] = make_uint2((o & 0xffu) | 0x20000u | im, hm);
                                } else {
                                    s_pool[2][tid].w = hm;
                                }
                            }
                        }
                    }
                    if (!ROOTSTEP) {  // (ROOTSTEP: the slots past a launch's last ray keep their old words, never read)
                        s_pool[0][tid] = q0;
                        s_pool[1][tid] = q1;
                        s_pool[2][tid] = q2;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (take && !take_left) {
                    const uint32_t slot = pcol + (widx & 63u);
                    p0 = s_pool[0][slot];
                    p1 = s_pool[1][slot];
                    p2 = s_pool[2][slot];
                    if (ROOTSTEP) start_ray(p0, p1, p2);
                }
                if (!ROOTSTEP && take) start_ray(p0, p1, p2);
            }
            if (!POOL && (int32_t)tg.y < 0 && widx != 0xffffffffu) {
                TT_DB(4);
                TT_DL(19, true);
                // work index -> ray index (8x8 screen tiles for full-frame primary batches)
                uint32_t local = widx;
                if (swizzle) {
                    const uint32_t tw = A.width >> 3;
                    const uint32_t t = widx >> 6, l = widx & 63u;
                    const uint32_t ty = fastdiv(t, A.div_tiles), tx = t - ty * tw;
                    local = (ty * 8u + (l >> 3)) * A.width + tx * 8u + (l & 7u);
                }
                ray_index = A.ray_offset + local;
                const uint4* rp = reinterpret_cast<const uint4*>(A.rays + ray_index);
                const uint4 r0 = rp[0], r1 = rp[1];
                pix = r0.w;
                if (INFO == 2) col_w = (pix < A.n_pixels) ? A.colors[pix].Data[3] : 0.0f;
                ray.ox = __uint_as_float(r0.x);
                ray.oy = __uint_as_float(r0.y);
                ray.oz = __uint_as_float(r0.z);
                ray.dx = __uint_as_float(r1.x);
                ray.dy = __uint_as_float(r1.y);
                ray.dz = __uint_as_float(r1.z);
                ray.ix = rcp_rn(ray.dx);
                ray.iy = rcp_rn(ray.dy);
                ray.iz = rcp_rn(ray.dz);
                best.t = A.far_plane;
                best.u = 0.0f;
                best.v = 0.0f;
                best.mesh_id = 0;
                best.tri_id = -1;
                tg = make_uint2(0u, 0u);
                stack_size = 0;
                if (LEAF) {
                    if (LEAF == 2) wray = ray;
                    // the root's node step; a hit is the TLAS leaf -> BLAS switch (enter_blas with nothing to
                    // push), a miss leaves an empty group: the advance below finishes the ray with the miss record
                    cg = make_uint2(0u, 0u);
                    Reps = 1;
                    if (root_leaf_hit(A.root, ray, best.t)) enter_object_space(L, ray, oct, cg);
                }
                if (!LEAF) {
                    wray = ray;
                    oct = octant_inv4(ray);
                    cg = make_uint2(A.tlas_base, 0x80000000u);  // the TLAS root: node 0 of the context's TLAS
                    tlas_ss = -1;
                    NodeOffset = (int32_t)A.tlas_base;  // TLAS level (0, or a frame-slot TLAS's region)
                    TriOffset = 0;
                    MatOffset = 0;
                    mesh_id = -1;
                    Reps = 0;
                }
                if (STATS) c_rays++;
#if TT_ROOT_LEAF
                if (!LEAF && rl_ok) {  // the root's node step, then the TLAS leaf -> BLAS switch
                    const RootLeaf& RL = A.root;
                    const bool hit = root_leaf_hit(RL, ray, best.t);
                    cg = make_uint2(RL.base_child, 0u);  // (hitmask & 0xff000000) | imask: both 0
                    tg = make_uint2(RL.base_tri, hit ? RL.bits : 0u);
                    Reps = 1;
                    if (STATS) c_nodes++;
                    // a ray that hits the root's leaf switches to its BLAS before this iteration's node step
                    // (here, with the started lanes only: a TLAS-level lane has no pending leaf bits at the
                    // loop top otherwise, so no per-iteration test is needed)
                    if (hit) enter_blas();
                }
#endif
            }
        }

        TT_DL(30, (int32_t)tg.y < 0);  // lanes that sit this iteration out
        // ------------------------------------------------------------- node phase
        // valu_mix:node:begin
        if (STATS) {  // SIMD-efficiency diagnostics (wave-uniform; lane 0 accumulates)
            const uint64_t nm = __ballot(tg.y == 0u && Reps < TT_MAX_REPS && (cg.y & 0xff000000u));
            const uint64_t am = __ballot((int32_t)tg.y >= 0);  // outside the lane-0 branch: a ballot there sees lane 0 only
            if (lane == 0) {
                d_iter++;
                d_node_lanes += (uint32_t)__popcll(nm);
                d_node_iters += nm ? 1u : 0u;
                d_active_lanes += (uint32_t)__popcll(am);
            }
        }
        // A lane is at the top of the reference's loop exactly when no leaf triangles are pending.
        if (tg.y == 0u) {
            TT_DB(5);
            if (Reps >= TT_MAX_REPS) {
                tg.y = TT_IDLE;  // loop bound hit: the reference writes nothing
                if (STATS) c_reps++;
                keep_record(A, ray_index_of(ray_index));
                if (ORD) record_chunk_cost(A, swizzle, ray_index, Reps);
            } else if (cg.y & 0xff000000u) {  // IntersectionKernels.compute:157-187
                const uint32_t child = take_child(cg, oct);
                bool ok = true;
                if (cg.y & 0xff000000u) {
                    TT_DB(7);
                    TT_PUSH(cg, ok);
                }
                if (ok) {
                    TT_DB(6);
                    TT_DL(17, true);
                    if (STATS) {  // how many node-phase lanes visit the same node as the first one
                        const uint32_t lead = __builtin_amdgcn_readfirstlane(child);
                        const uint64_t same = __ballot(child == lead), all = __ballot(true);
                        d_lead_same += child == lead ? 1u : 0u;
                        d_uniform += (same == all && lane == (uint32_t)__builtin_ctzll(all)) ? 1u : 0u;
                    }
                    const NodeWords n = load_node<TT_NODE_CPOL>(nodes, child);
                    const uint32_t hitmask = node_intersect(n.n0, n.n1, n.n2, n.n3, n.n4, ray, oct, best.t);
                    cg = node_group(hitmask, n, NodeOffset);
                    tg = tri_group(hitmask, n, TriOffset);
                    Reps++;
                    if (STATS) c_nodes++;
                } else {
                    tg.y = TT_IDLE;
                    if (STATS) c_ovf++;
                    TT_REPORT_OVERFLOW(A);
                    keep_record(A, ray_index_of(ray_index));
                }
            } else if (!EMPTYG) {  // :188-191 (EMPTYG: only a lane that started with both groups empty comes here)
                tg = cg;
                cg = make_uint2(0u, 0u);
            }
            if (!LEAF && (int32_t)tg.y > 0 && tlas_ss == -1) enter_blas();  // :194-219 TLAS leaf -> BLAS
        }
        // valu_mix:node:end

        if (STATS) {
            const uint64_t tm = __ballot((int32_t)tg.y > 0);
            if (lane == 0) {
                d_tri_lanes += (uint32_t)__popcll(tm);
                d_tri_iters += tm ? 1u : 0u;
            }
        }
        // --------------------------------------------------------- triangle phase
        // valu_mix:tri:begin
        if ((int32_t)tg.y > 0) {  // :220-226, highest bit first, one triangle per pass
            TT_DB(9);
            TT_DL(18, true);
            const uint32_t ti = firstbithigh(tg.y);
            tg.y &= ~(1u << ti);
            const bool acc = intersect_triangle<MATCHECK>(tris, A.mat, A.bounce == 0, A.flags, (int32_t)(tg.x + ti),
                                                          mesh_id, MatOffset, ray, best);
            if (STATS) {
                c_tris++;
                c_acc += acc ? 1u : 0u;
            }
        }
        // valu_mix:tri:end

        // ----------------------------------------- advance: pop / finish (:228-251)
        // One place for every lane whose group is used up, whether it came from a node step or
        // from its last triangle this pass (equivalent order: the reference pops right after).
        if constexpr (RESTART) {
            // The same advance with the restart. Which lanes finish is balloted outside the divergent block, so that
            // the pool state stays wave-uniform (SGPRs); the path without a finishing lane is one pop.
            const bool used_up = tg.y == 0u && (cg.y & 0xff000000u) == 0u;
            const bool finishing = used_up && stack_size == 0;
            // POPLAST: the lanes that pop, decided here and popped after the restart block (the two touch different
            // lanes and different LDS: the order between them changes nothing)
            const bool popping = used_up && stack_size != 0;
            if (used_up) {
                TT_DB(10);
                TT_DL(31, finishing);
                if (!POPLAST && stack_size != 0) {
                    TT_DB(11);
                    TT_POP(cg);
                }
            }
            // (MASKB: compare by compare -- the ballot of an AND of compares still goes through a 0 / 1 value -- and
            // the masks joined on the scalar side)
            const uint64_t fin = MASKB ? (lane_mask<MASKB>(tg.y == 0u) & lane_mask<MASKB>((cg.y & 0xff000000u) == 0u) &
                                          lane_mask<MASKB>(stack_size == 0))
                                       : lane_mask<false>(finishing);
            if (fin != 0ull) {  // wave-uniform
                TT_DB(32);
                const uint32_t n_fin = (uint32_t)__builtin_popcount((uint32_t)fin) + (uint32_t)__builtin_popcount((uint32_t)(fin >> 32));
                const uint32_t n_take = min(n_fin, pool_end - pool_next);  // (pool_next <= pool_end always)
                if (finishing) {
                    const uint32_t rank = lane_prefix(fin);
                    if (rank < n_take) {
                        TT_DL(33, true);
                        // the next prepared ray's record out of its slot, the finished ray's result into it
                        const uint32_t widx = pool_next + rank;
                        const uint32_t slot = (tid - lane) + (widx & 63u);
                        const uint4 p0 = s_pool[0][slot], p1 = s_pool[1][slot], p2 = s_pool[2][slot];
#ifdef TT_TEST_PARK_SWAP  // (tests only: a wrong parked word must show in the records)
                        const float park_u = best.v, park_v = best.u;
#else
                        const float park_u = best.u, park_v = best.v;
#endif
                        if (READY) {  // word by word: each store takes its value where it lies
                            // (volatile: left to itself the compiler joins them into a b128 and a b64 again and builds
                            // their register tuples)
                            typedef __attribute__((address_space(3))) volatile uint32_t lds_word;
                            lds_word* k0 = (lds_word*)&s_pool[0][slot];
                            lds_word* k1 = (lds_word*)&s_pool[1][slot];
                            k0[0] = (uint32_t)best.tri_id;
                            k0[1] = __float_as_uint(best.t);
                            k0[2] = __float_as_uint(park_u);
                            k0[3] = __float_as_uint(park_v);
                            k1[0] = ray_index;
                            k1[1] = pix;
                        } else {
                            s_pool[0][slot] = make_uint4((uint32_t)best.tri_id, __float_as_uint(best.t), __float_as_uint(park_u),
                                                         __float_as_uint(park_v));
                            reinterpret_cast<uint2*>(&s_pool[1][slot])[0] = make_uint2(ray_index, pix);
                        }
                        start_from(widx, p0, p1, p2, !POPLAST);  // (a finishing lane's stack is empty)
                    } else {
                        pending = true;  // no prepared ray left: written at the next refill (or when the wave drains)
                        tg.y = TT_IDLE;
                    }
                }
                if (n_take != 0u) {  // slots [pool_next, pool_next + n_take) of one chunk-aligned chunk: no wrap
                    const uint64_t m = n_take >= 64u ? ~0ull : ((1ull << n_take) - 1ull);
                    parked |= m << (pool_next & 63u);
                    pool_next += n_take;
                }
            }
            if (POPLAST && popping) {
                TT_DB(11);
                TT_POP(cg);
            }
        } else if (tg.y == 0u && (cg.y & 0xff000000u) == 0u) {
            TT_DB(10);
            TT_DL(31, stack_size == 0);
            if (stack_size == 0) TT_DB(32);
            if (stack_size != 0) {
                TT_DB(11);
                if (!LEAF && stack_size == tlas_ss) {
                    TT_DB(12);
                    leave_blas(A.tlas_base, world_ray(), NodeOffset, TriOffset, tlas_ss, ray, oct);
                }
                TT_POP(cg);
            } else {
                pending = true;  // written at the next refill (or when the wave drains)
                tg.y = TT_IDLE;
            }
        }
    }

#ifdef TT_DIAG_BLOCKS
    __syncthreads();
    if (tid < TT_DB_N && A.diag_times && tt_db[tid]) atomicAdd(A.diag_times + tid, tt_db[tid]);
#endif
    if (STATS) {
        const uint32_t v[8] = {wave_sum(c_rays), wave_sum(c_nodes), wave_sum(c_tris), wave_sum(c_blas),
                               wave_sum(c_hits), wave_sum(c_reps), wave_sum(c_ovf), wave_sum(c_acc)};
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (v[k]) atomicAdd(&A.ctl->stats[k], (unsigned long long)v[k]);
            const uint32_t d[6] = {d_iter, d_node_iters, d_node_lanes, d_tri_iters, d_tri_lanes, d_active_lanes};
#pragma unroll
            for (int k = 0; k < 6; k++) atomicAdd(&A.ctl->diag[k], (unsigned long long)d[k]);
        }
        const uint32_t ls = wave_sum(d_lead_same), un = wave_sum(d_uniform);
        if (lane == 0) {
            atomicAdd(&A.ctl->diag[6], (unsigned long long)ls);
            atomicAdd(&A.ctl->diag[7], (unsigned long long)un);
        }
    }
}

template <bool STATS, bool MATCHECK, int INFO>
__global__ TT_BOUNDS void tt_trace_kernel(TraceArgs A) {
    trace_body<STATS, MATCHECK, INFO, false, false>(A);
}
template <bool MATCHECK, int INFO>
__global__ TT_BOUNDS void tt_trace_kernel_indirect(TraceArgs A) {
    trace_body<false, MATCHECK, INFO, true, false>(A);
}
// (held at 5 waves per SIMD like the direct kernels: the cost record would otherwise cost INFO = 2 a
// wave; the material-check forms keep the default bounds, which do not spill VGPRs)
template <int INFO>
__global__ __launch_bounds__(TT_BLOCK) __attribute__((amdgpu_waves_per_eu(5))) void tt_trace_kernel_ord(TraceArgs A) {
    trace_body<false, false, INFO, false, true>(A);
}
template <int INFO>
__global__ TT_BOUNDS void tt_trace_kernel_ord_mat(TraceArgs A) {
    trace_body<false, true, INFO, false, true>(A);
}
// The leaf-TLAS form (trace_body<LEAF>): its own kernels, so the generic ones keep their code and names.
// Waves per SIMD the register allocation is held to. 6 for every INFO form (73 / 78 / 80 VGPRs, no scratch):
// INFO 0 / 1 also fit 7 waves (71 / 72 VGPRs, no scratch), but the smaller SGPR budget at 7 waves costs 7 / 14
// SGPR spills inside the loop and measured 1.2 % slower on the headline. A 5-wave bound measured 2.7 % slower:
// the sixth resident wave is where the gain over the generic kernels (89 / 93 VGPRs, 5 waves) comes from, the
// VALU instructions per ray barely move (profiles/r07/leaf/). Capping one launch's grid at 5
// waves per SIMD (TT_BLOCKS_PER_CU=20) costs nothing while other frame slots' launches fill the SIMDs.
#ifndef TT_LEAF_WAVES
#define TT_LEAF_WAVES(INFO) 6
#endif
#define TT_LEAF_BOUNDS __launch_bounds__(TT_BLOCK) __attribute__((amdgpu_waves_per_eu(TT_LEAF_WAVES(INFO))))
// TT_LEAF_WRAY_RESIDENT 1: INFO = 2 keeps the world ray's origin and direction in registers (80 VGPRs, still
// 6 waves, no scratch); 0: it re-reads them from RayData for the record (77 VGPRs), measured 1.5 % slower on the
// headline (profiles/r07/leaf/ab.json)
#ifndef TT_LEAF_WRAY_RESIDENT
#define TT_LEAF_WRAY_RESIDENT 1
#endif
// (with TT_LEAF_RESTART no lane keeps it: finished rays' records are written at full width from the pool, where the
// re-read costs one pass per chunk)
#define TT_LEAF_FORM(INFO) \
    ((INFO) == 2 && TT_LEAF_WRAY_RESIDENT && !(TT_LEAF_POOL && TT_LEAF_ROOT_STEP && TT_LEAF_RESTART) ? 2 : 1)
// (IND, INFO: the profile summaries bench.py reads key a kernel by its name's last template argument, INFO)
template <bool IND, int INFO>
__global__ TT_LEAF_BOUNDS void tt_trace_leaf_kernel(TraceArgs A) {
    trace_body<false, false, INFO, IND, false, TT_LEAF_FORM(INFO)>(A);
}

// ------------------------------------------------------------------ launchers
template <bool S, bool M, int I>
static hipError_t launch_one(const TraceArgs& a, bool leaf, uint32_t grid, hipStream_t st) {
    if constexpr (!S && !M) {
        if (leaf) {  // never with stats, the material check or the adaptive order (tt_dispatch.hip decides)
            if (a.n_rays_dev) hipLaunchKernelGGL((tt_trace_leaf_kernel<true, I>), dim3(grid), dim3(TT_BLOCK), 0, st, a);
            else hipLaunchKernelGGL((tt_trace_leaf_kernel<false, I>), dim3(grid), dim3(TT_BLOCK), 0, st, a);
            return hipGetLastError();
        }
    }
    if constexpr (!S) {
        if (a.n_rays_dev) {  // stats launches never take a device count (tt_dispatch.hip refuses them)
            hipLaunchKernelGGL((tt_trace_kernel_indirect<M, I>), dim3(grid), dim3(TT_BLOCK), 0, st, a);
            return hipGetLastError();
        }
        if (a.chunk_cost) {  // TT_TRACE_ADAPTIVE_ORDER (never with stats or a device count)
            if (M) hipLaunchKernelGGL((tt_trace_kernel_ord_mat<I>), dim3(grid), dim3(TT_BLOCK), 0, st, a);
            else hipLaunchKernelGGL((tt_trace_kernel_ord<I>), dim3(grid), dim3(TT_BLOCK), 0, st, a);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((tt_trace_kernel<S, M, I>), dim3(grid), dim3(TT_BLOCK), 0, st, a);
    return hipGetLastError();
}

template <bool S, bool M>
static hipError_t launch_info(const TraceArgs& a, int info, bool leaf, uint32_t grid, hipStream_t st) {
    if (info == 0) return launch_one<S, M, 0>(a, leaf, grid, st);
    if (info == 1) return launch_one<S, M, 1>(a, leaf, grid, st);
    return launch_one<S, M, 2>(a, leaf, grid, st);
}

// leaf: take the leaf-TLAS kernels (the caller has checked root_one_instance(a.root), no stats, no material
// check, no adaptive order)
hipError_t tt_launch_trace(const TraceArgs& a, bool stats, bool matcheck, int info, bool leaf, uint32_t grid,
                           hipStream_t st) {
    if (leaf && (stats || matcheck || a.chunk_cost || !root_one_instance(a.root))) return hipErrorInvalidValue;
    if (stats)
        return matcheck ? launch_info<true, true>(a, info, false, grid, st) : launch_info<true, false>(a, info, false, grid, st);
    return matcheck ? launch_info<false, true>(a, info, false, grid, st) : launch_info<false, false>(a, info, leaf, grid, st);
}

// Occupancy (resident blocks per CU) of every instantiation (occupancy_of, tt_traverse.h).
// index = stats*6 + matcheck*3 + info; 12 + matcheck*3 + info: the adaptive-order kernels;
// 18 + indirect*3 + info: the leaf-TLAS kernels
hipError_t tt_trace_occupancy_table(int* out24) {
    out24[0] = occupancy_of(tt_trace_kernel<false, false, 0>);
    out24[1] = occupancy_of(tt_trace_kernel<false, false, 1>);
    out24[2] = occupancy_of(tt_trace_kernel<false, false, 2>);
    out24[3] = occupancy_of(tt_trace_kernel<false, true, 0>);
    out24[4] = occupancy_of(tt_trace_kernel<false, true, 1>);
    out24[5] = occupancy_of(tt_trace_kernel<false, true, 2>);
    out24[6] = occupancy_of(tt_trace_kernel<true, false, 0>);
    out24[7] = occupancy_of(tt_trace_kernel<true, false, 1>);
    out24[8] = occupancy_of(tt_trace_kernel<true, false, 2>);
    out24[9] = occupancy_of(tt_trace_kernel<true, true, 0>);
    out24[10] = occupancy_of(tt_trace_kernel<true, true, 1>);
    out24[11] = occupancy_of(tt_trace_kernel<true, true, 2>);
    out24[12] = occupancy_of(tt_trace_kernel_ord<0>);
    out24[13] = occupancy_of(tt_trace_kernel_ord<1>);
    out24[14] = occupancy_of(tt_trace_kernel_ord<2>);
    out24[15] = occupancy_of(tt_trace_kernel_ord_mat<0>);
    out24[16] = occupancy_of(tt_trace_kernel_ord_mat<1>);
    out24[17] = occupancy_of(tt_trace_kernel_ord_mat<2>);
    out24[18] = occupancy_of(tt_trace_leaf_kernel<false, 0>);
    out24[19] = occupancy_of(tt_trace_leaf_kernel<false, 1>);
    out24[20] = occupancy_of(tt_trace_leaf_kernel<false, 2>);
    out24[21] = occupancy_of(tt_trace_leaf_kernel<true, 0>);
    out24[22] = occupancy_of(tt_trace_leaf_kernel<true, 1>);
    out24[23] = occupancy_of(tt_trace_leaf_kernel<true, 2>);
    return hipGetLastError();
}

uint32_t tt_trace_block_size() { return TT_BLOCK; }
uint32_t tt_trace_chunk_rays() { return TT_CHUNK_BIG; }
// LDS of one block: the stack entries its form keeps there, plus the leaf-TLAS form's prepared-ray pool
uint32_t tt_trace_lds_bytes(bool leaf) {
    const uint32_t stack = (uint32_t)((leaf ? lds_depth_of<1>() : lds_depth_of<0>()) * TT_BLOCK * sizeof(uint2));
    return stack + (leaf && TT_LEAF_POOL ? (uint32_t)(3 * TT_BLOCK * sizeof(uint4)) : 0u);
}
// (one spill area serves every form: sized for the shallowest LDS part)
uint32_t tt_trace_spill_entries() {
    constexpr int depth = lds_depth_of<1>() < lds_depth_of<0>() ? lds_depth_of<1>() : lds_depth_of<0>();
    return depth >= TT_STACK_SIZE ? 0u : (uint32_t)(TT_STACK_SIZE - depth);
}
