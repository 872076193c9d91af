// tt_trace_leaf.h — the leaf-TLAS closest-hit loop (tt_trace_leaf_kernel<IND, INFO>, tt_trace.hip), for launches
// whose TLAS root is one leaf holding one instance (root_one_instance; C2, C3, C5). Included by tt_trace.hip after
// the record writers and root_leaf_hit, which it uses.
//
// Every ray that hits the root's box switches to the same BLAS through the same LeafMesh record and never leaves it
// (the switch pushes nothing, so a BLAS exit could only come at stack_size 0, where the ray finishes). The record is
// read once per wave at a wave-uniform address (scalar loads; from device memory at every launch, so
// tt_scene_update_meshdata is honoured as in the generic kernel), the offsets and the mesh id are wave-uniform, and
// no lane keeps a TLAS stack mark, best.mesh_id or the world ray: fewer VGPRs (more resident waves), no TLAS-leaf
// test after a node step and no BLAS-exit test in the advance. The arithmetic of a ray and its order are the generic
// kernel's (trace_body), so results are bit-identical. There are no stats, material-check or adaptive-order forms.
//
// The prepared-ray pool. The rays of a dequeued chunk are set up by all 64 lanes at once into s_pool, one 48-B
// record per ray as three 16-B words [word][slot] (slot = work index & 63: a reservation is one chunk-aligned chunk
// of TT_CHUNK_BIG rays): (o.xyz, d.x) (d.yz, i.xy) (i.z, PixelIndex, state, mask), o / d / i the ray in the
// instance's object space. The setup also makes the ray's first node step -- the BLAS root, L.off.w, with t_max =
// FarPlane, the same node for every ray of the launch -- from wave-uniform loads of the node. The step's child base
// and triangle base are wave-uniform (root_cg_x, root_tg_x), so the record carries only `mask`, the step's 32-bit
// hit mask (0 for a ray that missed the root's box), and `state` = octant byte | (the root's imask where the step
// hit an inner child, else 0) << 8 | Reps << 16, ready-made: a starting lane's oct and cg.y are one v_perm_b32 each,
// Reps one shift and tg.y one AND. write_record's test of Data.w (INFO 2) is made by the setup too: a ray that fails
// it carries PixelIndex 0xffffffff, which writes no texel either, and the record writes pass -1 for Data.w.
//
// Parked results. A lane whose ray finishes while the pool holds prepared rays takes the next one in the same advance
// block. The finished ray's result goes into the slot just consumed -- word 0: (tri_id, t, u, v), word 1: (work
// index, PixelIndex) -- and bit `slot` of the wave-uniform mask `parked` is set; lane s writes the record of slot s,
// through write_record, before a chunk setup overwrites the pool, before the cooperative drain and at the loop's
// exit. A lane's ray_index holds the ray's WORK index (ray_of() maps it where a record is written), and the INFO 2
// record's world ray is read back from RayData words 0-1 by write_record, so no lane keeps it.
//
// PIN: this body compiles to the machine code it had as one form of trace_body (profiles/r21/split/: every kernel's
// assembly identical line for line). The compiler's numbering of the loop's values, and with it the order of register
// copies, follows details that carry no meaning; the four lines marked PIN below hold them where they were. Each can
// go with the next change that alters this loop's code anyway.
#ifndef TT_TRACE_LEAF_H
#define TT_TRACE_LEAF_H

// Idle lanes at which the refill block runs while the wave's pool holds prepared rays (only the few lanes a Reps
// bound or a stack overflow idles wait for it). The headline is flat over 14 - 20 and falls below 12 (4: -5 %): a
// refill that only reads a record still costs the wave an iteration with its record writes (profiles/r12/refill/).
#ifndef TT_LEAF_REFILL_MIN
#define TT_LEAF_REFILL_MIN 16
#endif
// ... and when the pool is empty: lanes then idle for want of a prepared ray. The chunk setup is full-width work
// however few lanes wait for it, but 1 / 4 / 8 / 12 measured no better than 16, and 20 and more worse
// (profiles/r15/restart/ab.json).
#ifndef TT_LEAF_RESTART_MIN
#define TT_LEAF_RESTART_MIN 16
#endif

template <bool IND, int INFO>
__device__ __forceinline__ void trace_leaf_body(const TraceArgs& A) {
    constexpr int tt_lds_depth = lds_depth_of<true>();  // the LDS part of the stack (TT_PUSH / TT_POP)
    static_assert(TT_CHUNK_BIG == TT_WAVE, "the prepared-ray pool holds one chunk, one slot per lane");
    __shared__ uint2 s_stack[tt_lds_depth][TT_BLOCK];
    __shared__ uint4 s_pool[3][TT_BLOCK];
    // the LeafMesh record of the one instance
    // (read before the kernel's first store, so the compiler can prove the loads unclobbered and make them scalar)
    const LeafEntry L = load_leaf_mesh<true>(A.leaf, A.root.base_tri + firstbithigh(A.root.bits));
    // the wave-uniform words of the BLAS root's step that a starting lane needs (node_group / tri_group): the child
    // and triangle bases. The whole node is read again by each chunk setup and lives only there.
    uint32_t root_cg_x = 0, root_tg_x = 0;
    {
        const NodeWords n = load_node_uniform(A.nodes, A.n_nodes, (uint32_t)L.off.w);
        root_cg_x = n.n1.x + (uint32_t)L.off.y;
        root_tg_x = n.n1.y + (uint32_t)L.off.x;
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

    // wave-uniform scheduler state, as in trace_body: the pool [pool_next, pool_end) of work indices is also the range
    // of prepared rays that s_pool holds
    uint32_t pool_next = 0, pool_end = 0, more = 1;
    const uint32_t wave_id = blockIdx.x * (TT_BLOCK / TT_WAVE) + (tid >> 6);
    SegState S{blockIdx.x % TT_SEGS, 0u, 0u};
    const uint32_t n_rays = IND ? launch_ray_count(A) : A.n_rays;
    const uint32_t n_tiles = (n_rays + 63u) >> 6;
    const bool swizzle = IND ? (A.tile_swizzle && n_rays == A.n_pixels) : (A.tile_swizzle != 0u);
    const __amdgpu_buffer_rsrc_t nodes = buffer_rsrc(A.nodes, A.n_nodes * (uint32_t)TT_NODE_STRIDE);
    const __amdgpu_buffer_rsrc_t tris = buffer_rsrc(A.tris, A.n_tris * (uint32_t)sizeof(TriPos));

    // lane traversal state, as in trace_body (tg.y == TT_IDLE: a lane without a ray) less what is wave-uniform here
    constexpr uint32_t TT_IDLE = 0x80000000u;
    uint32_t ray_index = 0;  // the ray's WORK index
    uint32_t pix = 0;        // RayData.PixelIndex, or 0xffffffff (see above)
    float col_w = 0.0f;      // PIN: never read (Data.w is not kept, see above); start_from names it
    bool pending = false;    // finished with no prepared ray to take, record not yet written
    LaneRay ray{};
    const LaneRay no_ray{};  // (no lane keeps the world ray: write_record reads it back, the drain never needs it)
    Best best{};
    uint2 cg = make_uint2(0u, 0u), tg = make_uint2(0u, TT_IDLE);
    uint32_t oct = 0;
    int32_t stack_size = 0;
    // the instance's offsets and mesh id, wave-uniform for the whole launch (PIN: declared as trace_body declares its
    // lane values and then set, not initialised in place)
    int32_t NodeOffset = 0, TriOffset = 0, MatOffset = 0, mesh_id = -1, Reps = 0;
    NodeOffset = L.off.y;
    TriOffset = L.off.x;
    MatOffset = L.off.z;
    mesh_id = L.mesh_id;
    // work index -> ray index (8x8 screen tiles for full-frame primary batches), as trace_body's ray start has it
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
    // bit s = slot s of the pool holds a parked result (wave-uniform)
    uint64_t parked = 0ull;
    // :229-241: the hit record and _PrimaryTriangleInfo of a lane's own finished ray
    auto finish_ray = [&]() { write_record<INFO, true>(A, ray_of(ray_index), pix, -1.0f, best, no_ray, mesh_id, TriOffset); };
    // a lane's start on work index widx from the pool record of its slot, after the setup's root step: Reps 2, the
    // hit inner children in cg and the hit leaf triangles in tg, or (the root's box missed: Reps 1) an empty group,
    // with which the advance finishes the ray
    // (zero_stack false: the caller knows stack_size is 0 -- a lane that finishes has an empty stack)
    auto start_from = [&](const uint32_t widx, const uint4 p0, const uint4 p1, const uint4 p2, const bool zero_stack) {
        TT_DL(19, true);
        ray_index = widx;
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
        // `state` and `mask` as the setup left them for this: one instruction per value
        oct = __builtin_amdgcn_perm(p2.z, p2.z, 0u);  // the octant byte in all four
        cg = make_uint2(root_cg_x, __builtin_amdgcn_perm(p2.w, p2.z, 0x070c0c01u));  // hit inner children | imask, or 0
        tg = make_uint2(root_tg_x, p2.w & 0x00ffffffu);
        Reps = (int32_t)(p2.z >> 16);
        (void)col_w;  // PIN: in this closure
        best.t = A.far_plane;
        best.u = 0.0f;
        best.v = 0.0f;
        best.mesh_id = 0;
        best.tri_id = -1;
        if (zero_stack) stack_size = 0;
    };
    while (true) {
        TT_DB(0);
        // ---------------------------------------------------------------- refill
        // (the loop's ballots take the compare's lane mask: HIP's int __ballot makes a 0 / 1 value of it and compares
        // that again)
        const uint64_t idle = __builtin_amdgcn_ballot_w64((int32_t)tg.y < 0);
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
        // lanes only idle for want of a prepared ray, so the pool-empty case has a threshold of its own (the few lanes
        // a Reps bound or a stack overflow idles wait for TT_LEAF_REFILL_MIN of them while the pool holds rays)
        const uint32_t refill_min = pool_next >= pool_end ? (uint32_t)TT_LEAF_RESTART_MIN : (uint32_t)TT_LEAF_REFILL_MIN;
        // finished rays write their records in batches, right before their lanes are refilled
        if ((n_idle == TT_WAVE && pool_dry) || (n_idle >= refill_min && !pool_dry) || to_wide) {
            if (pending) {
                TT_DB(1);
                finish_ray();
                pending = false;
            }
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
                    write_record<INFO, true>(A, ray_of(k1.x), k1.y, -1.0f, kb, no_ray, mesh_id, TriOffset);
                }
                parked = 0ull;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (n_idle == TT_WAVE && pool_dry) break;
#if TT_WIDE
        if (to_wide) {
            TT_DB(13);
            WideState st{{ray, no_ray, cg, tg, oct, stack_size, -1, NodeOffset, TriOffset, MatOffset, Reps,
                          ray_of(ray_index), tid, gtid, (int32_t)tg.y >= 0},
                         best, mesh_id, pix, -1.0f};
            regroup<2, true>(st, __ballot((int32_t)tg.y >= 0), lane);
            auto finish_wide = [&](const WideState& w) {
                write_record<INFO, true>(A, w.ray_index, w.pix, w.col_w, w.best, w.wray, mesh_id, TriOffset);
            };
            auto exhaust_wide = [&](const WideState& w, bool) { keep_record(A, w.ray_index); };
            uint32_t c_none = 0;  // (STATS is false below: the drain never touches its counters, so one stands for all)
            wide_phase<false, false, 2, true>(A, st, s_stack, spill, spill_stride, nodes, tris, lane,
                                              Counters{c_none, c_none, c_none, c_none, c_none, c_none, c_none},
                                              finish_wide, exhaust_wide);
            break;
        }
#endif
        if (n_idle >= refill_min && !pool_dry) {
            TT_DB(2);
#if TT_LONG_PRIO
            // a wave carrying a long ray issues ahead of the others until its next refill without one (trace_body)
            if (__builtin_amdgcn_ballot_w64((int32_t)tg.y >= 0 && Reps >= TT_LONG_PRIO) != 0ull) __builtin_amdgcn_s_setprio(TT_LONG_PRIO_LEVEL);
            else __builtin_amdgcn_s_setprio(0);
#endif
            // wave-uniform: take from the wave's pool first, then one dequeue for the rest
            const uint32_t avail = pool_end - pool_next;
            uint32_t new_base = 0, new_count = 0;
            if (avail < n_idle && more) {
                new_count = sched_reserve(A.ctl, n_rays, n_tiles, lane, n_idle - avail, wave_id, S, new_base);
                more = new_count > 0 ? 1u : 0u;
                // the segment state too is the wave's, not a lane's: as lane values the compiler parked the bits in a
                // register that the triangle pass also uses, with a copy out and a copy in per loop iteration
                S.seg = __builtin_amdgcn_readfirstlane(S.seg);
                S.dead = __builtin_amdgcn_readfirstlane(S.dead);
            }
            const PoolTake pt = pool_take(idle, n_idle, new_base, new_count, pool_next, pool_end, more);
            const uint32_t widx = pt.widx;
            // (readfirstlane: the wave-uniform scheduler state stays in SGPRs and the loop head's tests SALU)
            pool_next = __builtin_amdgcn_readfirstlane(pt.pool_next);
            pool_end = __builtin_amdgcn_readfirstlane(pt.pool_end);
            more = __builtin_amdgcn_readfirstlane(pt.more);
            const uint32_t pcol = tid - lane;  // the wave's pool columns
            const bool take = (int32_t)tg.y < 0 && widx != 0xffffffffu;
            // slots left from the previous chunk are read before the new chunk overwrites the pool
            const bool take_left = take && lane_prefix(idle) < min(avail, n_idle);
            if (take_left) {
                const uint32_t slot = pcol + (widx & 63u);
                const uint4 p0 = s_pool[0][slot], p1 = s_pool[1][slot], p2 = s_pool[2][slot];
                // (and the lane starts at once, so that the record is not held in registers across the setup)
                start_from(widx, p0, p1, p2, true);
            }
            // (one wave owns the pool and its LDS accesses execute in order: these only keep the compiler from
            // moving the reads and writes of different lanes' slots across each other)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (new_count > 0) {  // wave-uniform: every lane, busy or idle, sets up ray new_base + lane
                TT_DB(4);
                // the BLAS root, from device memory at every setup, in SGPRs
                const NodeWords rn = load_node_uniform(A.nodes, A.n_nodes, (uint32_t)L.off.w);
                // (all 64 lanes but in a launch's last chunk, where the slots past the last ray keep their old words,
                // never read)
                if (lane < new_count) {
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
                    // the TLAS root's node step; a hit is the TLAS leaf -> BLAS switch (nothing to push)
                    uint32_t o = 0u;
                    uint2 g = make_uint2(0u, 0u);
                    const bool root_hit = root_leaf_hit(A.root, r, A.far_plane);
                    TT_DL(29, root_hit);
                    if (root_hit) enter_object_space(L, r, o, g);
                    // write_record's test of Data.w (INFO 2) is made here: where it fails the record carries no pixel (a
                    // PixelIndex past the frame writes no texel either)
                    // (the record goes out before the BLAS root's step, which then holds only what it reads; the step
                    // adds its mask. Reps is 2 after the step, 1 where the ray missed the root's box: o is 0 there)
                    const uint4 q0 = make_uint4(__float_as_uint(r.ox), __float_as_uint(r.oy), __float_as_uint(r.oz),
                                                __float_as_uint(r.dx));
                    const uint4 q1 = make_uint4(__float_as_uint(r.dy), __float_as_uint(r.dz), __float_as_uint(r.ix),
                                                __float_as_uint(r.iy));
                    // (PIN: words 10 / 11 first hold Data.w and the TLAS root's hit, then get their own values)
                    uint4 q2 = make_uint4(__float_as_uint(r.iz), r0.w, __float_as_uint(cw), o | g.y);
                    if (INFO == 2 && !(cw == -1.0f || (float)A.bounce == cw)) q2.y = 0xffffffffu;
                    q2.z = (o & 0xffu) | (root_hit ? 0x20000u : 0x10000u);
                    q2.w = 0u;
                    s_pool[0][tid] = q0;
                    s_pool[1][tid] = q1;
                    s_pool[2][tid] = q2;
                    // the BLAS root's node step, as the generic loop makes it first (best.t is FarPlane there)
                    if (root_hit) {
                        TT_DB(28);
                        const uint32_t hm = node_intersect(rn.n0, rn.n1, rn.n2, rn.n3, rn.n4, r, o, A.far_plane);
                        // the node group of a step that hit no inner child is empty: no imask
                        const uint32_t im = (hm & 0xff000000u) ? (rn.n0.w >> 24) << 8 : 0u;
                        reinterpret_cast<uint2*>(&s_pool[2][tid])[1] = make_uint2((o & 0xffu) | 0x20000u | im, hm);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (take && !take_left) {
                const uint32_t slot = pcol + (widx & 63u);
                const uint4 p0 = s_pool[0][slot], p1 = s_pool[1][slot], p2 = s_pool[2][slot];
                start_from(widx, p0, p1, p2, true);
            }
        }

        TT_DL(30, (int32_t)tg.y < 0);  // lanes that sit this iteration out
        // ------------------------------------------------------------- node phase
        // valu_mix:node:begin
        // A lane is at the top of the reference's loop exactly when no leaf triangles are pending.
        if (tg.y == 0u) {
            TT_DB(5);
            if (Reps >= TT_MAX_REPS) {
                tg.y = TT_IDLE;  // loop bound hit: the reference writes nothing
                keep_record(A, ray_of(ray_index));
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
                    const NodeWords n = load_node<TT_NODE_CPOL>(nodes, child);
                    const uint32_t hitmask = node_intersect(n.n0, n.n1, n.n2, n.n3, n.n4, ray, oct, best.t);
                    cg = node_group(hitmask, n, NodeOffset);
                    tg = tri_group(hitmask, n, TriOffset);
                    Reps++;
                } else {
                    tg.y = TT_IDLE;
                    TT_REPORT_OVERFLOW(A);
                    keep_record(A, ray_of(ray_index));
                }
            }
            // (:188-191, "no inner child left: the node group becomes the triangle group", has nothing to write: only a
            // lane that started with both groups empty comes here -- a pop only brings groups with an inner child and
            // the advance takes every other used-up lane)
        }
        // valu_mix:node:end

        // --------------------------------------------------------- triangle phase
        // valu_mix:tri:begin
        if ((int32_t)tg.y > 0) {  // :220-226, highest bit first, one triangle per pass
            TT_DB(9);
            TT_DL(18, true);
            const uint32_t ti = firstbithigh(tg.y);
            tg.y &= ~(1u << ti);
            intersect_triangle<false>(tris, A.mat, A.bounce == 0, A.flags, (int32_t)(tg.x + ti), mesh_id, MatOffset, ray,
                                      best);
        }
        // valu_mix:tri:end

        // ----------------------------------------- advance: pop / restart / finish (:228-251)
        // One place for every lane whose group is used up, whether it came from a node step or from its last triangle
        // this pass (equivalent order: the reference pops right after). Which lanes finish is balloted outside the
        // divergent block, so that the pool state stays wave-uniform (SGPRs); the path without a finishing lane is
        // one pop. The lanes that pop are decided here and popped after the restart block (the two touch different
        // lanes and different LDS: the order between them changes nothing): the pop decrements stack_size in place,
        // and a restarting lane's stack_size, 0 already, is not written.
        const bool used_up = tg.y == 0u && (cg.y & 0xff000000u) == 0u;
        const bool finishing = used_up && stack_size == 0;
        const bool popping = used_up && stack_size != 0;
        if (used_up) {
            TT_DB(10);
            TT_DL(31, finishing);
        }
        // (compare by compare -- the ballot of an AND of compares still goes through a 0 / 1 value -- and the masks
        // joined on the scalar side)
        const uint64_t fin = __builtin_amdgcn_ballot_w64(tg.y == 0u) & __builtin_amdgcn_ballot_w64((cg.y & 0xff000000u) == 0u) &
                             __builtin_amdgcn_ballot_w64(stack_size == 0);
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
                    // word by word: each store takes its value where it lies
                    // (volatile: left to itself the compiler joins them into a b128 and a b64 and builds their register
                    // tuples)
                    typedef __attribute__((address_space(3))) volatile uint32_t lds_word;
                    lds_word* k0 = (lds_word*)&s_pool[0][slot];
                    lds_word* k1 = (lds_word*)&s_pool[1][slot];
                    k0[0] = (uint32_t)best.tri_id;
                    k0[1] = __float_as_uint(best.t);
                    k0[2] = __float_as_uint(park_u);
                    k0[3] = __float_as_uint(park_v);
                    k1[0] = ray_index;
                    k1[1] = pix;
                    start_from(widx, p0, p1, p2, false);  // (a finishing lane's stack is empty)
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
        if (popping) {
            TT_DB(11);
            TT_POP(cg);
        }
    }

#ifdef TT_DIAG_BLOCKS
    __syncthreads();
    if (tid < TT_DB_N && A.diag_times && tt_db[tid]) atomicAdd(A.diag_times + tid, tt_db[tid]);
#endif
}
#endif  // TT_TRACE_LEAF_H
