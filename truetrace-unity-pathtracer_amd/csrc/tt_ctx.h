// tt_ctx.h — internal to the C ABI's translation units (tt_api.hip, tt_scene_api.hip, tt_dispatch.hip,
// tt_build.hip; not installed): the context and object structs, the owning device buffer, error reporting,
// the shared-scene read / write sections, the timing-ring entries and the host-pointer staging helpers.
// The structural checks of what a kernel may reach are host-only headers with no HIP in them:
// tt_scene_check_host.h (the one CWBVH walk, the whole-scene check), tt_assemble_host.h, tt_tlas_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "tt_assemble_host.h"
#include "tt_device.h"
#include "tt_light_refit.h"
#include "tt_light_refit_plan_host.h"
#include "tt_refit.h"

#define TT_RING 256u
// Overlay regions behind a scene's nodes (tt_ctx_share_blas): this many frame-slot TLASes per lender
#ifndef TT_TLAS_SLOTS
#define TT_TLAS_SLOTS 8u
#endif

// A device allocation and its owner: move-only, freed by the destructor. Every DevBuf lives in a heap object
// (a context, an object, a refit plan) or on the stack, never in static storage: none may outlive the exit
// teardown of tt_api.hip (MainThreadExitGuard).
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n), own(o.own) { o.forget(); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            n = o.n;
            own = o.own;
            o.forget();
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count) {
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        n = count;
        return hipSuccess;
    }
    bool own = true;  // false: borrowed from another context's scene (tt_ctx_share_scene), never freed here
    void release() {
        if (p && own) (void)hipFree(p);
        forget();
    }
    void borrow(const DevBuf& o) {
        release();
        p = o.p;
        n = o.n;
        own = false;
    }

  private:
    void forget() {
        p = nullptr;
        n = 0;
        own = true;
    }
};
static_assert(!std::is_copy_constructible<DevBuf<int>>::value, "DevBuf owns its allocation");
static_assert(std::is_nothrow_move_constructible<DevBuf<int>>::value, "DevBuf moves without throwing");

// The host mirror of a scene, with what its last validation established (tt_check::Bookkeeping: blas_ok,
// is_tlas_node, tlas_nodes, is_blas_node) for the incremental per-frame updates (tt_scene_update_*)
struct SceneHost : tt_check::Bookkeeping {
    std::vector<tt_cwbvh_node> nodes;
    std::vector<int32_t> tlas;
    std::vector<tt_mesh_data> mesh;
    uint32_t n_tris = 0;
    uint32_t n_mat = 0;
    bool any_shadow_skip = false;  // IsBackground / ShadowCaster present (shadow material checks)
    bool any_atlas_shadow = false; // specTrans == 1 present (shadow glass tint: needs the texture atlas)
    bool any_cutout = false;       // Cutout materials present (need the alpha atlas)
    std::vector<CutoutMat> cut;    // per material, when any_cutout
    std::vector<GlassMat> glass;   // per material, when any_atlas_shadow
};

// A scene's device buffers. The one list of them: what an upload replaces, what a borrower borrows and what
// a context frees are all stated here.
struct SceneDev {
    DevBuf<tt_cwbvh_node> nodes;
    DevBuf<uint8_t> nodes_k;    // TT_NODE_STRIDE != 80: the kernels' strided copy of `nodes`
    DevBuf<tt_cuda_triangle> tris_raw;
    DevBuf<TriPos> tris;
    DevBuf<uint32_t> mat_tag;
    DevBuf<CutoutMat> mat_cut;
    DevBuf<GlassMat> mat_glass;
    // the TLAS side: an overlay borrower (tt_ctx_share_blas) owns these four
    DevBuf<int32_t> tlas;
    DevBuf<tt_mesh_data> mesh_raw;
    DevBuf<MeshGpu> mesh;
    DevBuf<LeafMesh> leaf;
    DevBuf<uint2> tex;          // _TextureAtlas, decoded RGBA half texels
    uint32_t tex_w = 0, tex_h = 0;
    DevBuf<uint8_t> atlas;      // _AlphaAtlas (R8)
    uint32_t atlas_w = 0, atlas_h = 0;
    // Terrains + the Heightmap atlas (tt_scene_upload_terrains): part of the scene like the atlases
    DevBuf<tt_terrain> terrains;  // device copy (tt_resolve_normals indexes it per hit)
    std::vector<tt_terrain> terrains_host;  // each march launch carries its terrain in the kernel arguments
    DevBuf<uint16_t> hmap;        // binary16 texels
    uint32_t hmap_w = 0, hmap_h = 0;
    // Lights (tt_scene_upload_lights): LightNodes, LightTriangles, _LightMeshes and their host mirrors (what
    // tt_scene_update_light_nodes validates against). They index the geometry, so they go when it is replaced.
    DevBuf<tt_light_node> lnodes;
    DevBuf<tt_light_tri> ltris;
    DevBuf<tt_light_mesh> lmeshes;
    uint32_t n_lnodes = 0;  // 0: no lights
    std::vector<tt_light_node> lnodes_host;
    std::vector<tt_light_tri> ltris_host;
    std::vector<tt_light_mesh> lmeshes_host;
    // tt_lights_refit: the plan of what it climbs (built from the mirrors at tt_scene_upload_lights, again after a
    // tt_scene_update_light_nodes that changed a `left` or a _MeshData update that moved a tree), its device
    // arrays (made by the first refit after either) and the staging of a call's block table and host transforms
    struct LightRefit {
        tt_lplan::Plan plan;
        bool plan_valid = false, dev_valid = false;
        DevBuf<int2> up;
        DevBuf<uint32_t> arrive;
        DevBuf<int32_t> leaf_node, leaf_row;
        DevBuf<LightRefitBlock> blocks;
        DevBuf<tt_light_transform> transforms;
        void release() {
            plan = tt_lplan::Plan();
            plan_valid = dev_valid = false;
            up.release();
            arrive.release();
            leaf_node.release();
            leaf_row.release();
            blocks.release();
            transforms.release();
        }
    };
    LightRefit lrefit;
    void release_lights() {
        lrefit.release();
        lnodes.release();
        ltris.release();
        lmeshes.release();
        n_lnodes = 0;
        lnodes_host.clear();
        ltris_host.clear();
        lmeshes_host.clear();
    }

    // what tt_scene_upload / tt_scene_assemble_objects replace (the atlases and terrains have calls of their own)
    void release_geometry() {
        nodes.release();
        nodes_k.release();
        tris_raw.release();
        tris.release();
        mat_tag.release();
        mat_cut.release();
        mat_glass.release();
        tlas.release();
        mesh_raw.release();
        mesh.release();
        leaf.release();
        release_lights();
    }
    // a borrower's view of a lender's scene: everything but the TLAS side
    void borrow_shared(const SceneDev& o) {
        nodes.borrow(o.nodes);
        nodes_k.borrow(o.nodes_k);
        tris_raw.borrow(o.tris_raw);
        tris.borrow(o.tris);
        mat_tag.borrow(o.mat_tag);
        mat_cut.borrow(o.mat_cut);
        mat_glass.borrow(o.mat_glass);
        tex.borrow(o.tex);
        atlas.borrow(o.atlas);
        terrains.borrow(o.terrains);
        hmap.borrow(o.hmap);
        terrains_host = o.terrains_host;
        lnodes.borrow(o.lnodes);
        ltris.borrow(o.ltris);
        lmeshes.borrow(o.lmeshes);
        n_lnodes = o.n_lnodes;
        hmap_w = o.hmap_w;
        hmap_h = o.hmap_h;
        tex_w = o.tex_w;
        tex_h = o.tex_h;
        atlas_w = o.atlas_w;
        atlas_h = o.atlas_h;
    }
    void borrow_tlas_side(const SceneDev& o) {
        tlas.borrow(o.tlas);
        mesh_raw.borrow(o.mesh_raw);
        mesh.borrow(o.mesh);
        leaf.borrow(o.leaf);
    }
};

struct tt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 0;
    int blocks_per_cu = 0;
    uint32_t grid = 0;
    uint32_t grid_of[24] = {};  // resident persistent grid per kernel instantiation (12..17: adaptive order,
                                // 18..23: the leaf-TLAS kernels, direct and indirect)
    uint32_t last_form = TT_TRACE_FORM_NONE;  // the kernel form of the last closest-hit launch (tt_trace_last_form)
    uint32_t shadow_grid_of[4] = {};  // the same for the any-hit kernel (stats * 2 + matcheck)
    TraceControl* ctl = nullptr;  // two control blocks: a trace launch uses one and zeroes the other
    uint32_t* sticky = nullptr;   // stack overflows of every launch since the last tt_async_overflows
    uint32_t ctl_cur = 0;          // the block the next launch uses
    bool ctl_zero[2] = {false, false};  // known zero when the next launch on the stream runs
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // last launch (aliases into the ring)
    hipEvent_t ring0[256] = {}, ring1[256] = {};
    uint32_t ring_n = 0, ring_base = 0;
    bool timing = true;  // tt_ctx_set_timing: asynchronous launches record their HIP-event pair
    uint32_t frame_pixels = 0;  // tt_ctx_set_frame_pixels: batched frames' bounce random numbers (0: off)
    bool group_member = false;  // a tt_group member's context: groups carry no lights (tt_scene_upload_lights refuses)
    bool lib_stream = false;    // stream is one of tt_stream_create's (tt_shutdown / the exit teardown may end it)
    std::string err;
    // scene
    bool has_scene = false;
    bool any_invisible = false;
    SceneHost host;  // (carries the scene's any_shadow_skip / any_atlas_shadow / any_cutout)
    SceneDev scene;
    uint32_t terrain_grid_of[3] = {};  // resident persistent grids: closest hit, with stats, shadow (0: not sized yet)
    DevBuf<unsigned char> st_touched;  // TT_TRACE_STATS: per ray, its record was rewritten by this call
    // TT_ROOT_LEAF: node 0 as the device holds it is known on the host (upload, node updates); a device
    // refit of the TLAS rewrites it without a read-back, so the fast root step is off until the next update
    bool root_known = false;
    // TLAS refit (f4): plan valid for (scene generation, n_tlas_nodes)
    RefitDev refit;
    uint64_t scene_gen = 0, refit_gen = ~0ull;
    uint32_t refit_n_tlas = 0;
    DevBuf<float> st_boxes;
    // BLAS refit (f4, deforming / skinned meshes): one prepared plan + triangle boxes per mesh
    struct BlasRefit {
        RefitDev dev;
        uint32_t n_nodes = 0;  // nodes the plan covers, from the mesh's first node
        uint64_t gen = ~0ull;
        uint32_t node_base = ~0u;  // the mesh's NodeOffset the plan was built for
        DevBuf<float> boxes;
    };

    std::map<uint32_t, BlasRefit> blas_refit;
    // tt_blas_refit_many: the host plan of each mesh it has seen (a changed list only re-composes), and the
    // composed forest of the last list with its device arrays -- valid for (scene generation, the ordered list of
    // (mesh_index, n_tris, NodeOffset)), so a frame with the same list allocates nothing and builds no plan
    struct BlasPlanHost {
        RefitPlan plan;
        uint32_t n_nodes = 0;
        uint64_t gen = ~0ull;
        uint32_t node_base = ~0u;
    };
    std::map<uint32_t, BlasPlanHost> many_plans;
    struct BlasRefitMany {
        uint64_t gen = ~0ull;
        std::vector<uint32_t> key;       // mesh_index, n_tris, NodeOffset per item, in list order
        std::vector<uint32_t> box_base;  // per item: its first box in the pool
        RefitDev dev;
        DevBuf<float> boxes;             // the pool: every item's triangle boxes
        DevBuf<uint8_t> desc;            // the call's part / item / block descriptors
        DevBuf<float> bounds;            // bounds_out of a host-pointer call
        std::vector<std::pair<uint32_t, uint32_t>> node_ranges;  // [first, end) of the items' BLAS nodes, adjacent ones merged
    };
    BlasRefitMany refit_many;
    DevBuf<float> st_vtx;
    DevBuf<int32_t> st_idx, st_leaf;
    // host-pointer staging
    uint64_t max_rays = 0;
    DevBuf<tt_ray_data> st_rays;
    DevBuf<uint32_t> st_info;
    DevBuf<tt_col_data> st_colors;
    DevBuf<float> st_normals;
    DevBuf<uint32_t> counter;   // bounce enqueue counters: two blocks of counter_words, used in turn
    uint32_t counter_words = 0, counter_cur = 0;
    DevBuf<uint2> spill;        // deep traversal-stack entries (tt_trace_spill_entries() per thread)
    uint32_t spill_threads = 0; // grid threads the spill area is sized for (max over all grids)
    DevBuf<tt_shadow_ray> st_shadow;
    DevBuf<tt_light_sample> st_samples;  // tt_emit_nee with host pointers
    DevBuf<uint32_t> nee_ctl;            // tt_emit_nee: survivor count, tile ticket, one look-back word per tile
    DevBuf<float4> st_vis;
    DevBuf<float4> st_nee;
    DevBuf<tt_cache_data> st_cache;
    unsigned long long last_diag[8] = {};
    // pinned host staging for the asynchronous per-frame updates: two slots, each reused once the
    // copy enqueued from it has completed (its event)
    struct Pinned {
        void* p = nullptr;
        size_t n = 0;
        hipEvent_t ev = nullptr;
        bool pending = false;
    };
    Pinned pin[2];
    uint32_t pin_cur = 0;
    // TT_TRACE_ADAPTIVE_ORDER: per bounce index (min(bounce, 7)), the last flagged launch's per-tile
    // costs and the order buffer the next one dequeues in (tt_order.hip)
    struct OrderSlot {
        DevBuf<uint32_t> cost[2];  // cost[cur]: the last launch's costs (when valid)
        DevBuf<uint32_t> order;
        uint32_t cur = 0, w = 0, h = 0;
        uint32_t n_chunks = 0;     // chunks of the last flagged launch (tt_trace_chunk_costs)
        bool valid = false;
    };
    OrderSlot ord[8];
    // tt_ctx_share_scene: a borrower traces its lender's scene buffers (read-only) on its own stream
    tt_ctx* lender = nullptr;  // set on a borrower
    int borrowers = 0;         // on a lender: contexts currently tracing its scene
    // node array sizes: the scene's nodes, and the device array (+ TT_TLAS_SLOTS overlay regions of
    // ovl_stride nodes each behind them, tt_ctx_share_blas); tlas_res: the reach of the uploaded TLAS
    uint32_t n_nodes_scene = 0, n_nodes_dev = 0, tlas_res = 0;
    // tlas_cap: the scene's own TLAS capacity, the leading nodes no validated BLAS walk reached at upload (an
    // assembled scene: its tlas_region) -- what a rebuilt TLAS (tt_scene_update_tlas) may grow to. ovl_stride:
    // the node distance between overlay regions, max(tlas_cap, tlas_res), so a frame slot's rebuilt TLAS fits too.
    uint32_t tlas_cap = 0, ovl_stride = 0;
    // tt_ctx_share_blas: a borrower with a TLAS of its own (a frame slot's TLAS refit and _MeshData rewrite
    // never wait for, or are seen by, the other slots): its TLAS nodes [0, n_tlas_own) live in overlay region
    // ovl_slot of the lender's node array, at kernel node index tlas_base; TLASBVH8Indices, _MeshData and the
    // derived MeshGpu / LeafMesh records are its own buffers. host.nodes then holds only those TLAS nodes.
    bool ovl = false;
    uint32_t ovl_slot = 0, tlas_base = 0, n_tlas_own = 0;
    uint32_t ovl_used = 0;     // lender: overlay regions in use (bit per slot)
    // Cross-stream order of a shared scene (the reference rewrites the TLAS and _MeshData every frame,
    // then dispatches, AssetManager.cs:1821-1825): a lender mutation waits for the borrowers' launches
    // already enqueued, and a borrower launch waits for the lender's mutations already enqueued. An
    // overlay borrower reads only the lender's BLAS part, so it orders only against BLAS-side mutations.
    // The lender's share state below (and its host node 0, which plain borrowers read for TT_ROOT_LEAF) is
    // guarded by `mu`, so a lender and its borrowers may be driven from different host threads; `mu` is held
    // across each read / write section (SceneRead / SceneWrite), so their enqueues are atomic against each
    // other. Recursive: a section's own calls (the root-leaf copy, the refit's bookkeeping) lock it again.
    std::recursive_mutex mu;
    std::vector<tt_ctx*> borrower_list;  // lender: the contexts tracing its scene
    hipEvent_t ev_scene = nullptr;       // lender: after its last scene mutation (recorded while borrowed)
    uint64_t scene_mut = 0;              // lender: mutations recorded in ev_scene so far
    hipEvent_t ev_blas = nullptr;        // lender: after its last BLAS-side mutation (overlay borrowers wait)
    uint64_t blas_mut = 0;               // lender: BLAS-side mutations recorded in ev_blas so far
    hipEvent_t ev_read = nullptr;        // borrower: recorded on its stream by a lender mutation (SceneWrite)
    uint64_t read_seq = 0;               // borrower: read sections enqueued so far
    uint64_t read_waited = 0;            // borrower: reads the lender's stream already waits for
    uint64_t mut_waited = 0;             // borrower: lender mutations this stream already waits for
};

// A device-resident BLAS (tt_object_create): it belongs to its device, not to a context, and an assembly
// copies it, so it may be destroyed any time after tt_scene_assemble_objects returned.
struct tt_object {
    int device = 0;
    uint32_t n_nodes = 0, n_tris = 0, root = 0;
    DevBuf<tt_cwbvh_node> d_nodes;    // BLAS-local indices, as tt_blas_copy returns them
    DevBuf<tt_cuda_triangle> d_tris;
    DevBuf<TriPos> d_tripos;          // derived once, on the GPU
    std::vector<tt_cwbvh_node> nodes;  // host mirror: an assembled scene's host.nodes is composed from these
    tt_asm::ObjectWalk walk;           // the nodes the BLAS walk reached, the largest MatDat it saw
    // tt_object_build_device only: CWBVHIndicesBufferInverted (source triangle -> leaf position) and the summary
    bool built = false;
    DevBuf<int32_t> d_leaf_of;
    tt_object_build_info build_info{};
};

// Scene-mutating calls are refused on a borrower (update the lender), and reallocating ones on a
// lender that has borrowers (their pointers would dangle). TT_REFUSE_BORROWER_TLAS lets an overlay
// borrower (tt_ctx_share_blas) mutate its own TLAS-side state.
#define TT_REFUSE_BORROWER(c)                                                                              \
    do {                                                                                                   \
        if ((c)->lender) return fail((c), TT_ERR_INVALID_ARG, "this context traces a shared scene: update the context it shares from"); \
    } while (0)
#define TT_REFUSE_BORROWER_TLAS(c)                                                                         \
    do {                                                                                                   \
        if ((c)->lender && !(c)->ovl) return fail((c), TT_ERR_INVALID_ARG, "this context traces a shared scene: update the context it shares from"); \
    } while (0)
#define TT_REFUSE_LENDER(c)                                                                                \
    do {                                                                                                   \
        if ((c)->borrowers > 0) return fail((c), TT_ERR_INVALID_ARG, "other contexts share this scene: destroy them (or re-share) first"); \
    } while (0)

// Per-call timing ring entries (tt_timing_read) around device work issued on the context stream. `on`: the
// entry is recorded -- c->timing (tt_ctx_set_timing) for calls that are asynchronous or report no kernel
// time, c->timing || !async for the launches whose synchronous form reports one.
inline hipError_t ring_open(tt_ctx* c, bool on, uint32_t& slot) {
    slot = c->ring_n % TT_RING;
    if (!on) return hipSuccess;
    return hipEventRecord(c->ring0[slot], c->stream);
}
inline hipError_t ring_close(tt_ctx* c, bool on, uint32_t slot) {
    if (!on) return hipSuccess;
    const hipError_t e = hipEventRecord(c->ring1[slot], c->stream);
    c->ring_n++;
    c->ev0 = c->ring0[slot];
    c->ev1 = c->ring1[slot];
    return e;
}

// Shared-scene ordering (tt_ctx_share_scene / tt_ctx_share_blas). A borrower's enqueues that read the
// lender's scene buffers form a read section, a lender's scene mutation a write section; both hold the
// lender's mutex from first to last enqueue, so sections of the contexts sharing one scene are atomic
// against each other whichever host threads drive them. A read section makes the borrower's stream wait
// for the lender mutations enqueued before it (one wait per new mutation) and counts one read. A write
// section makes the lender's stream wait for every borrower stream with reads counted since the last such
// wait, by recording an event on that stream right then -- one record per borrower per mutation and
// nothing per launch (round 5 recorded one after every borrower launch: with the launch-timing pair, the
// per-launch markers cost 15-20% of a strong-scaled rank's frame, profiles/r05/events/) -- and, at its end,
// records the mutation for later readers. An overlay borrower (tt_ctx_share_blas) reads only the lender's
// BLAS part, so it orders only against BLAS-side mutations.
inline hipError_t lazy_event(hipEvent_t& ev) {
    return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
}
// TT_NO_SCENE_ORDER: a diagnostic variant build only (make variant NAME=noorder VFLAGS=-DTT_NO_SCENE_ORDER): the
// sections take the lock but order nothing, to show the ordering tests fail without them.
#ifndef TT_NO_SCENE_ORDER
#define TT_NO_SCENE_ORDER 0
#endif
class SceneRead {
  public:
    explicit SceneRead(tt_ctx* c) : L_(c->lender) {
        if (!L_) return;
        if (TT_NO_SCENE_ORDER) {
            L_->mu.lock();
            return;
        }
        L_->mu.lock();
        const uint64_t seq = c->ovl ? L_->blas_mut : L_->scene_mut;
        if (seq != c->mut_waited) {
            err = hipStreamWaitEvent(c->stream, c->ovl ? L_->ev_blas : L_->ev_scene, 0);
            if (err == hipSuccess) c->mut_waited = seq;
        }
        c->read_seq++;
    }
    SceneRead(const SceneRead&) = delete;
    SceneRead& operator=(const SceneRead&) = delete;
    ~SceneRead() { end(); }
    void end() {
        if (L_) L_->mu.unlock();
        L_ = nullptr;
    }
    hipError_t err = hipSuccess;

  private:
    tt_ctx* L_;
};
// blas: the mutation touches what overlay borrowers read too (BLAS nodes, triangles); otherwise only the
// lender's TLAS-side state (TLAS nodes, _MeshData), which only plain borrowers read. active = false: no
// section (an overlay borrower's own TLAS-side state is read by nobody else).
class SceneWrite {
  public:
    SceneWrite(tt_ctx* c, bool blas, bool active = true) : c_(active ? c : nullptr), blas_(blas) {
        if (!c_) return;
        c_->mu.lock();
        if (TT_NO_SCENE_ORDER) return;
        for (tt_ctx* b : c_->borrower_list) {
            if (b->read_seq == b->read_waited || (b->ovl && !blas_)) continue;
            if ((err = lazy_event(b->ev_read)) != hipSuccess || (err = hipEventRecord(b->ev_read, b->stream)) != hipSuccess ||
                (err = hipStreamWaitEvent(c_->stream, b->ev_read, 0)) != hipSuccess)
                return;
            b->read_waited = b->read_seq;
        }
    }
    SceneWrite(const SceneWrite&) = delete;
    SceneWrite& operator=(const SceneWrite&) = delete;
    ~SceneWrite() {
        if (c_) c_->mu.unlock();
    }
    // after the mutation is enqueued: records it for the borrowers (a later borrower syncs the stream when
    // it shares, so nothing is recorded without one) and leaves the section
    hipError_t end() {
        if (!c_) return hipSuccess;
        hipError_t e = hipSuccess;
        if (!c_->borrower_list.empty() && !TT_NO_SCENE_ORDER) {
            e = lazy_event(c_->ev_scene);
            if (e == hipSuccess) e = hipEventRecord(c_->ev_scene, c_->stream);
            if (e == hipSuccess) c_->scene_mut++;
            if (e == hipSuccess && blas_) {
                e = lazy_event(c_->ev_blas);
                if (e == hipSuccess) e = hipEventRecord(c_->ev_blas, c_->stream);
                if (e == hipSuccess) c_->blas_mut++;
            }
        }
        c_->mu.unlock();
        c_ = nullptr;
        return e;
    }
    hipError_t err = hipSuccess;

  private:
    tt_ctx* c_;
    bool blas_;
};
// The node array the kernels read: the reference's (80-B stride) or its strided copy, refreshed on the
// context stream after every write to `nodes` (device node indices [first, first + count): a frame slot's
// TLAS sits at tlas_base).
inline const uint4* kernel_nodes(const tt_ctx* c) {
    return TT_NODE_STRIDE == 80 ? reinterpret_cast<const uint4*>(c->scene.nodes.p)
                                : reinterpret_cast<const uint4*>(c->scene.nodes_k.p);
}
inline hipError_t refresh_node_copy(tt_ctx* c, uint32_t first, uint32_t count) {
    if (TT_NODE_STRIDE == 80 || count == 0) return hipSuccess;
    return hipMemcpy2DAsync(c->scene.nodes_k.p + (size_t)first * TT_NODE_STRIDE, TT_NODE_STRIDE, c->scene.nodes.p + first,
                            sizeof(tt_cwbvh_node), sizeof(tt_cwbvh_node), count, hipMemcpyDeviceToDevice, c->stream);
}

inline tt_status fail(tt_ctx* c, tt_status s, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return s;
}

inline tt_status hip_fail(tt_ctx* c, hipError_t e, const char* what) {
    return fail(c, e == hipErrorOutOfMemory ? TT_ERR_OOM : TT_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

#define TT_HIP(c, call)                                   \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hip_fail(c, e_, #call); \
    } while (0)

inline bool is_device_ptr(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// tt_api.hip: the stream registry. A context whose library stream the teardown destroyed refuses every launch;
// a launch on a library stream arms the exit teardown of its thread.
bool stream_dead(hipStream_t s);
void note_stream_launch(hipStream_t s);
#define TT_REFUSE_DEAD_STREAM(c)                                                                            \
    do {                                                                                                    \
        if ((c)->lib_stream && stream_dead((c)->stream))                                                    \
            return fail((c), TT_ERR_INVALID_ARG, "the context's stream was destroyed by tt_shutdown / the exit teardown"); \
    } while (0)

// tt_scene_api.hip: a borrower leaves its lender; the pinned staging slots of the asynchronous per-frame updates
void unlink_borrower(tt_ctx* b);
hipError_t stage_begin(tt_ctx* c, const void* src, size_t bytes, void*& out);
hipError_t stage_end(tt_ctx* c);

// Host-pointer staging of a call's arrays. stage_in grows `buf` to offset + count elements, copies `count`
// of them from host + offset on the stream (host == nullptr: reserves only) and yields the device array;
// stage_out copies the same window back.
template <class T, class U>  // U: T or const T
hipError_t stage_in(tt_ctx* c, DevBuf<T>& buf, const void* host, size_t count, size_t offset, U*& dev) {
    if (buf.n < offset + count) {
        const hipError_t e = buf.alloc(offset + count);
        if (e != hipSuccess) return e;
    }
    dev = buf.p;
    if (!host) return hipSuccess;
    return hipMemcpyAsync(buf.p + offset, static_cast<const T*>(host) + offset, sizeof(T) * count, hipMemcpyHostToDevice, c->stream);
}
template <class T>
hipError_t stage_out(tt_ctx* c, void* host, const T* dev, size_t count, size_t offset = 0) {
    return hipMemcpyAsync(static_cast<T*>(host) + offset, dev + offset, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream);
}

inline void copy_why(const std::string& w, char* why, uint32_t why_len) {
    if (why && why_len) {
        std::strncpy(why, w.c_str(), why_len - 1);
        why[why_len - 1] = 0;
    }
}
