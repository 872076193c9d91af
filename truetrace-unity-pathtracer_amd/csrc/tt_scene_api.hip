// tt_scene_api.hip — the C ABI of include/truetrace_hip.h, part two: everything that installs or changes a
// scene. Structural validation, tt_scene_upload, GPU-resident objects and their on-device assembly, the atlases
// and terrains, scene sharing (tt_ctx_share_scene / tt_ctx_share_blas), the refits, read-backs and the per-frame
// tt_scene_update_* calls.
#include <cmath>
#include <cstdlib>
#include <memory>

#include "tt_assemble.h"
#include "tt_build.h"
#include "tt_ctx.h"
#include "tt_lights_check_host.h"
#include "tt_refit_items_host.h"
#include "tt_tlas_host.h"

namespace {

using tt_check::Validator;

// What the whole-scene check (tt_scene_check_host.h) reads of a context's own scene ...
tt_check::SceneView view_of(const SceneHost& h) {
    const uint32_t n = (uint32_t)h.nodes.size();
    return {h.nodes.data(), n, h.nodes.data(), n, h.tlas.data(), h.tlas.size(), h.mesh.data(), h.mesh.size(), h.n_tris};
}
// ... and of an overlay borrower (tt_ctx_share_blas): its own TLAS side over the lender's nodes
tt_check::SceneView view_of(const SceneHost& own, const SceneHost& blas) {
    tt_check::SceneView v = view_of(own);
    v.bl = blas.nodes.data();
    v.n_bl = (uint32_t)blas.nodes.size();
    return v;
}
tt_check::SceneView view_of(const tt_ctx* c) { return c->ovl ? view_of(c->host, c->lender->host) : view_of(c->host); }

// The material words and the cutout / glass records of a scene's materials (h starts out fresh), shared by the
// two ways a scene arrives: tt_scene_upload and tt_scene_assemble_objects.
void derive_materials(const tt_material* mats, uint32_t n_mat, SceneHost& h, std::vector<uint32_t>& tags,
                      bool& any_invisible) {
    h.n_mat = n_mat;
    any_invisible = false;
    tags.assign(std::max<uint32_t>(n_mat, 1u), 0u);
    for (uint32_t m = 0; m < n_mat; m++) {
        tags[m] = mats[m].Tag & ~((1u << TT_MATWORD_CUTOUT) | (1u << TT_MATWORD_GLASS));
        if (mats[m].specTrans == 1.0f) tags[m] |= 1u << TT_MATWORD_GLASS;  // stained-glass shadow tint
        if (mats[m].MatType == TT_MAT_CUTOUT_INDEX) {  // alpha test, IntersectionKernels.compute:35-40
            tags[m] |= 1u << TT_MATWORD_CUTOUT;
            h.any_cutout = true;
        }
        any_invisible |= ((mats[m].Tag >> TT_FLAG_INVISIBLE) & 1u) != 0;
        h.any_shadow_skip |= (((mats[m].Tag >> TT_FLAG_IS_BACKGROUND) | (mats[m].Tag >> TT_FLAG_SHADOW_CASTER)) & 1u) != 0;
        h.any_atlas_shadow |= mats[m].specTrans == 1.0f;
    }
    if (h.any_cutout) {
        h.cut.assign(n_mat, CutoutMat{});
        for (uint32_t m = 0; m < n_mat; m++) {
            CutoutMat& r = h.cut[m];
            r.alpha_tex[0] = mats[m].AlphaTex[0];
            r.alpha_tex[1] = mats[m].AlphaTex[1];
            r.cutoff = mats[m].AlphaCutoff;
            for (int k = 0; k < 4; k++) r.scale[k] = mats[m].AlbedoTexScale[k];
        }
    }
    if (h.any_atlas_shadow) {
        h.glass.assign(n_mat, GlassMat{});
        for (uint32_t m = 0; m < n_mat; m++) {
            GlassMat& r = h.glass[m];
            r.albedo_tex[0] = mats[m].AlbedoTex[0];
            r.albedo_tex[1] = mats[m].AlbedoTex[1];
            for (int k = 0; k < 3; k++) r.color[k] = mats[m].surfaceColor[k];
            for (int k = 0; k < 4; k++) r.scale[k] = mats[m].AlbedoTexScale[k];
        }
    }
}

const char kOver4GiB[] = "node or triangle array of 4 GiB or more (the trace kernel addresses them with 32-bit offsets)";
bool over_4gib(uint64_t n_nodes, uint64_t n_tris) {
    return n_nodes * std::max<uint64_t>(sizeof(tt_cwbvh_node), TT_NODE_STRIDE) >= (1ull << 32) || n_tris * 48u >= (1ull << 32);
}

// A scene's arrays as tt_scene_upload and tt_scene_validate take them: is one missing?
bool null_or_empty(const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris, uint32_t n_tris,
                   const int32_t* tlas, uint32_t n_tlas, const tt_mesh_data* md, uint32_t n_mesh, const tt_material* mats,
                   uint32_t n_mat) {
    return !nodes || !n_nodes || !tris || !n_tris || !tlas || !n_tlas || !md || !n_mesh || (n_mat && !mats);
}

tt_status check_scene(const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris, uint32_t n_tris,
                      const int32_t* tlas, uint32_t n_tlas, const tt_mesh_data* md, uint32_t n_mesh,
                      const tt_material* mats, uint32_t n_mat, SceneHost& h, std::vector<uint32_t>& tags,
                      bool& any_invisible, std::string& why) {
    if (null_or_empty(nodes, n_nodes, tris, n_tris, tlas, n_tlas, md, n_mesh, mats, n_mat)) {
        why = "null or empty buffer";
        return TT_ERR_INVALID_ARG;
    }
    if (over_4gib(n_nodes, n_tris)) {
        why = kOver4GiB;
        return TT_ERR_INVALID_ARG;
    }
    h.nodes.assign(nodes, nodes + n_nodes);
    h.tlas.assign(tlas, tlas + n_tlas);
    h.mesh.assign(md, md + n_mesh);
    h.n_tris = n_tris;
    derive_materials(mats, n_mat, h, tags, any_invisible);
    Validator v(view_of(h));
    if (!v.run()) {
        why = v.why;
        return TT_ERR_INVALID_ARG;
    }
    tt_check::remember_validation(h, v, n_nodes);
    return TT_OK;
}

__host__ __device__ inline void derive_mesh(const tt_mesh_data& in, MeshGpu& o) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) o.m[r * 4 + c] = in.W2L[c * 4 + r];
    o.TriOffset = in.TriOffset;
    o.NodeOffset = in.NodeOffset;
    o.MaterialOffset = in.MaterialOffset;
    o.root = in.mesh_data_bvh_offsets & 0x7fffffff;
}

// LeafMesh[i] = the mesh record TLASBVH8Indices[i] names (indices were validated at upload)
std::vector<LeafMesh> derive_leaves(const std::vector<int32_t>& tlas, const std::vector<tt_mesh_data>& md) {
    std::vector<LeafMesh> out(std::max<size_t>(1, tlas.size()));
    for (size_t i = 0; i < tlas.size(); i++) {
        LeafMesh& l = out[i];
        std::memset(&l, 0, sizeof(l));
        const int32_t m = tlas[i];
        if (m >= 0 && (size_t)m < md.size()) derive_mesh(md[(size_t)m], l.m);
        l.mesh_id = m;
    }
    return out;
}

void derive_tri(const tt_cuda_triangle& t, TriPos& o) {
    o.p0x = t.pos0[0];
    o.p0y = t.pos0[1];
    o.p0z = t.pos0[2];
    o.e1x = t.posedge1[0];
    o.e1y = t.posedge1[1];
    o.e1z = t.posedge1[2];
    o.e2x = t.posedge2[0];
    o.e2y = t.posedge2[1];
    o.e2z = t.posedge2[2];
    o.matdat = t.MatDat;
    o.pad0 = o.pad1 = 0;
}

// The traversal records of updated _MeshData entries [first, first + count) (derive_mesh), and
// every TLAS leaf record whose TLASBVH8Indices entry names one of them (derive_leaves).
// src: records [first, first + count), read in place from the pinned staging buffer (host memory the
// GPU reads over the bus: no copy operation on the stream), also stored to _MeshData (raw).
__global__ void tt_update_mesh_kernel(const tt_mesh_data* __restrict__ src, tt_mesh_data* __restrict__ raw,
                                      MeshGpu* __restrict__ mesh, LeafMesh* __restrict__ leaf,
                                      const int32_t* __restrict__ tlas, uint32_t n_tlas, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        const tt_mesh_data r = src[i];
        raw[first + i] = r;
        MeshGpu g;
        derive_mesh(r, g);
        mesh[first + i] = g;
    }
    if (i < n_tlas) {
        const int32_t m = tlas[i];
        if (m >= 0 && (uint32_t)m - first < count) {
            LeafMesh l;
            derive_mesh(src[(uint32_t)m - first], l.m);
            l.mesh_id = m;
            l.pad[0] = l.pad[1] = l.pad[2] = 0;
            leaf[i] = l;
        }
    }
}

// A whole TLAS installed as one mutation (tt_scene_update_tlas, tt_tlas_rebuild; the launch's shape: tt_tlas::Plan).
// src_nodes / src_idx are read in place: the pinned staging slot (host memory the GPU reads over the bus) or the
// device builder's arrays. In 16-B units, 5 per node: units [0, copy_units) are copied to the TLAS region
// (dst_nodes = nodes + tlas_base, and the strided copy where there is one), units [copy_units, units) cleared, so
// the region holds what an upload of the host-composed array would. Thread i also stores TLASBVH8Indices[i] and
// its LeafMesh: the mesh's traversal record as the device holds it (derive_mesh of _MeshData, kept current by
// tt_update_mesh_kernel) under its new slot. The host validated every index before the launch.
__global__ void tt_install_tlas_kernel(const uint4* __restrict__ src_nodes, const int32_t* __restrict__ src_idx,
                                       uint4* __restrict__ dst_nodes, uint8_t* __restrict__ dst_k,
                                       int32_t* __restrict__ tlas, const MeshGpu* __restrict__ mesh,
                                       LeafMesh* __restrict__ leaf, uint32_t copy_units, uint32_t units, uint32_t n_idx,
                                       uint32_t n_mesh) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < units) {
        const uint4 v = i < copy_units ? src_nodes[i] : make_uint4(0u, 0u, 0u, 0u);
        dst_nodes[i] = v;
        if (dst_k) {
            uint32_t* k = reinterpret_cast<uint32_t*>(dst_k + (size_t)(i / 5u) * TT_NODE_STRIDE + (i % 5u) * 16u);
            k[0] = v.x;
            k[1] = v.y;
            k[2] = v.z;
            k[3] = v.w;
        }
    }
    if (i < n_idx) {
        const int32_t m = src_idx[i];
        tlas[i] = m;
        if ((uint32_t)m < n_mesh) {
            LeafMesh l;
            l.m = mesh[m];
            l.mesh_id = m;
            l.pad[0] = l.pad[1] = l.pad[2] = 0;
            leaf[i] = l;
        }
    }
}

// The host mirror a borrower keeps of its lender's scene: scalars and material records, never the node array
// or the validation bookkeeping (an overlay borrower adds its own TLAS-side arrays, tt_ctx_share_blas)
void copy_host_light(SceneHost& d, const SceneHost& s) {
    d = SceneHost{};
    d.n_tris = s.n_tris;
    d.n_mat = s.n_mat;
    d.any_shadow_skip = s.any_shadow_skip;
    d.any_atlas_shadow = s.any_atlas_shadow;
    d.any_cutout = s.any_cutout;
    d.cut = s.cut;
    d.glass = s.glass;
}

// Rebuilds the TLAS leaf records from the host mirror (on upload) and uploads them on the stream.
tt_status refresh_leaves(tt_ctx* c) {
    std::vector<LeafMesh> lv = derive_leaves(c->host.tlas, c->host.mesh);
    if (c->scene.leaf.n < lv.size()) {
        const hipError_t e = c->scene.leaf.alloc(lv.size());
        if (e != hipSuccess) return hip_fail(c, e, "TLAS leaf records");
    }
    TT_HIP(c, hipMemcpyAsync(c->scene.leaf.p, lv.data(), sizeof(LeafMesh) * lv.size(), hipMemcpyHostToDevice, c->stream));
    TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

// The gather's form. One batched kernel over all objects (csrc/tt_assemble.hip) is the product;
// TT_ASSEMBLE_FORM=memcpy selects three device-to-device copies per object, kept for A/B measurement
// (tools/assemble_bench.py, profiles/r09/assemble/). Read at every assembly -- a getenv beside a scene's worth of
// copies -- so one process can time both forms in turn. The bytes are identical in both forms.
bool assemble_kernel_form() {
    const char* e = std::getenv("TT_ASSEMBLE_FORM");
    return !(e && std::strcmp(e, "memcpy") == 0);
}

// Installing a scene, the part tt_scene_upload and tt_scene_assemble_objects share: scene_alloc, then the caller
// fills the node and triangle arrays its own way, then scene_commit. Whatever the caller's way, the context ends
// up the same: same buffers, same sizes, same bookkeeping.
struct SceneSizes {
    uint32_t n_nodes = 0, tlas_res = 0, n_nodes_dev = 0, tlas_cap = 0, ovl_stride = 0;
};

// Releases the scene being replaced and allocates the validated scene `h`'s buffers (the cutout / glass records
// and the leaf records come with scene_commit); the strided node copy starts out zero. tlas_region: the TLAS
// region an assembly states (an upload: the node count, so the BLAS walks alone bound the capacity).
tt_status scene_alloc(tt_ctx* c, const SceneHost& h, uint32_t n_nodes, uint32_t n_tris, size_t n_tags, uint32_t tlas_region,
                      SceneSizes& sz) {
    SceneDev& d = c->scene;
    d.release_geometry();
    // the TLAS region (every node the TLAS-level walk reaches lies in [0, tlas_res)) and TT_TLAS_SLOTS overlay
    // regions behind the scene's nodes, for frame slots with TLASes of their own; each holds what the scene's own
    // TLAS region holds (tlas_cap), so a slot's rebuilt TLAS (tt_scene_update_tlas) may outgrow the uploaded one
    sz.n_nodes = n_nodes;
    sz.tlas_res = 0;
    for (uint32_t n : h.tlas_nodes) sz.tlas_res = std::max(sz.tlas_res, n + 1u);
    // (a TLAS over n_mesh records never needs more than the reference's 2 * n_mesh nodes)
    const uint64_t want = std::max<uint64_t>(2ull * h.mesh.size(), sz.tlas_res);
    sz.tlas_cap = tt_tlas::region_capacity(h.is_blas_node, (uint32_t)std::min<uint64_t>(std::min(n_nodes, tlas_region), want));
    sz.ovl_stride = std::max(sz.tlas_cap, sz.tlas_res);
    if (((uint64_t)n_nodes + (uint64_t)TT_TLAS_SLOTS * sz.ovl_stride) * TT_NODE_STRIDE >= (1ull << 32))
        sz.tlas_res = sz.ovl_stride = 0;  // no overlay regions (a node array near the 32-bit limit of the kernels' buffer loads)
    sz.n_nodes_dev = n_nodes + TT_TLAS_SLOTS * sz.ovl_stride;
    hipError_t e;
    if ((e = d.nodes.alloc(sz.n_nodes_dev)) != hipSuccess || (e = d.tris_raw.alloc(n_tris)) != hipSuccess ||
        (e = d.tris.alloc(n_tris)) != hipSuccess || (e = d.tlas.alloc(h.tlas.size())) != hipSuccess ||
        (e = d.mesh_raw.alloc(h.mesh.size())) != hipSuccess || (e = d.mesh.alloc(h.mesh.size())) != hipSuccess ||
        (e = d.mat_tag.alloc(n_tags)) != hipSuccess)
        return hip_fail(c, e, "scene allocation");
    if (TT_NODE_STRIDE != 80) {
        if ((e = d.nodes_k.alloc((size_t)sz.n_nodes_dev * TT_NODE_STRIDE)) != hipSuccess) return hip_fail(c, e, "node copy");
        TT_HIP(c, hipMemsetAsync(d.nodes_k.p, 0, (size_t)sz.n_nodes_dev * TT_NODE_STRIDE, c->stream));
    }
    return TT_OK;
}

// The small uploads (TLAS indices, mesh records, material words and records) on the stream, the host
// bookkeeping, the leaf records; the stream is synchronized (refresh_leaves) before the scene counts as there.
tt_status scene_commit(tt_ctx* c, SceneHost&& h, const std::vector<uint32_t>& tags, const std::vector<MeshGpu>& mg,
                       bool any_invisible, const SceneSizes& sz) {
    SceneDev& d = c->scene;
    hipError_t e;
    TT_HIP(c, hipMemcpyAsync(d.tlas.p, h.tlas.data(), sizeof(int32_t) * h.tlas.size(), hipMemcpyHostToDevice, c->stream));
    TT_HIP(c, hipMemcpyAsync(d.mesh_raw.p, h.mesh.data(), sizeof(tt_mesh_data) * h.mesh.size(), hipMemcpyHostToDevice, c->stream));
    TT_HIP(c, hipMemcpyAsync(d.mesh.p, mg.data(), sizeof(MeshGpu) * mg.size(), hipMemcpyHostToDevice, c->stream));
    TT_HIP(c, hipMemcpyAsync(d.mat_tag.p, tags.data(), sizeof(uint32_t) * tags.size(), hipMemcpyHostToDevice, c->stream));
    if (h.any_cutout) {
        if ((e = d.mat_cut.alloc(h.cut.size())) != hipSuccess) return hip_fail(c, e, "cutout records");
        TT_HIP(c, hipMemcpyAsync(d.mat_cut.p, h.cut.data(), sizeof(CutoutMat) * h.cut.size(), hipMemcpyHostToDevice, c->stream));
    }
    if (h.any_atlas_shadow) {
        if ((e = d.mat_glass.alloc(h.glass.size())) != hipSuccess) return hip_fail(c, e, "glass records");
        TT_HIP(c, hipMemcpyAsync(d.mat_glass.p, h.glass.data(), sizeof(GlassMat) * h.glass.size(), hipMemcpyHostToDevice, c->stream));
    }
    c->host = std::move(h);  // (the vectors the copies above read move with it: their storage stays put)
    c->n_nodes_scene = sz.n_nodes;
    c->n_nodes_dev = sz.n_nodes_dev;
    c->tlas_res = sz.tlas_res;
    c->tlas_cap = sz.tlas_cap;
    c->ovl_stride = sz.ovl_stride;
    c->ovl_used = 0;
    c->root_known = true;
    c->any_invisible = any_invisible;
    c->scene_gen++;
    const tt_status st = refresh_leaves(c);
    if (st != TT_OK) return st;
    c->has_scene = true;
    return TT_OK;
}
}  // namespace

// Copies `bytes` of caller memory into the next pinned staging slot (waiting, if needed, until the
// copy last enqueued from that slot has completed), so the H2D copy can be asynchronous and the
// caller may reuse its buffer as soon as the call returns. stage_end() marks the slot in use by the
// copies enqueued since.
hipError_t stage_begin(tt_ctx* c, const void* src, size_t bytes, void*& out) {
    tt_ctx::Pinned& pn = c->pin[c->pin_cur];
    hipError_t e;
    if (!pn.ev && (e = hipEventCreateWithFlags(&pn.ev, hipEventDisableTiming)) != hipSuccess) return e;
    if (pn.pending) {
        if ((e = hipEventSynchronize(pn.ev)) != hipSuccess) return e;
        pn.pending = false;
    }
    if (pn.n < bytes) {
        if (pn.p) (void)hipHostFree(pn.p);
        pn.p = nullptr;
        pn.n = 0;
        if ((e = hipHostMalloc(&pn.p, bytes, hipHostMallocDefault)) != hipSuccess) return e;
        pn.n = bytes;
    }
    if (src) std::memcpy(pn.p, src, bytes);  // (null: the caller composes the slot's contents itself)
    out = pn.p;
    return hipSuccess;
}
hipError_t stage_end(tt_ctx* c) {
    tt_ctx::Pinned& pn = c->pin[c->pin_cur];
    c->pin_cur ^= 1u;
    const hipError_t e = hipEventRecord(pn.ev, c->stream);
    pn.pending = e == hipSuccess;
    return e;
}

void unlink_borrower(tt_ctx* b) {
    tt_ctx* L = b->lender;
    if (!L) return;
    std::lock_guard<std::recursive_mutex> lk(L->mu);
    L->borrowers--;
    L->borrower_list.erase(std::remove(L->borrower_list.begin(), L->borrower_list.end(), b), L->borrower_list.end());
    if (b->ovl) L->ovl_used &= ~(1u << b->ovl_slot);
    b->lender = nullptr;
    b->ovl = false;
    b->tlas_base = 0;
}

extern "C" {

tt_status tt_scene_upload(tt_ctx* c, const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris,
                          uint32_t n_tris, const int32_t* tlas, uint32_t n_tlas, const tt_mesh_data* md,
                          uint32_t n_mesh, const tt_material* mats, uint32_t n_mat) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER(c);
    TT_REFUSE_LENDER(c);
    if (null_or_empty(nodes, n_nodes, tris, n_tris, tlas, n_tlas, md, n_mesh, mats, n_mat))
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_upload: null or empty buffer");
    TT_HIP(c, hipSetDevice(c->device));
    c->has_scene = false;
    SceneHost h;
    std::vector<uint32_t> tags;
    bool any_invisible = false;
    std::string why;
    const tt_status vs = check_scene(nodes, n_nodes, tris, n_tris, tlas, n_tlas, md, n_mesh, mats, n_mat, h, tags,
                                     any_invisible, why);
    if (vs != TT_OK) return fail(c, vs, "scene validation failed: %s", why.c_str());
    std::vector<TriPos> tp(n_tris);
    for (uint32_t t = 0; t < n_tris; t++) derive_tri(tris[t], tp[t]);
    std::vector<MeshGpu> mg(n_mesh);
    for (uint32_t m = 0; m < n_mesh; m++) derive_mesh(md[m], mg[m]);
    SceneSizes sz;
    {
        const tt_status st = scene_alloc(c, h, n_nodes, n_tris, tags.size(), n_nodes, sz);
        if (st != TT_OK) return st;
    }
    TT_HIP(c, hipMemcpy(c->scene.nodes.p, nodes, sizeof(tt_cwbvh_node) * n_nodes, hipMemcpyHostToDevice));
    if (TT_NODE_STRIDE != 80) {
        TT_HIP(c, refresh_node_copy(c, 0, n_nodes));
        TT_HIP(c, hipStreamSynchronize(c->stream));
    }
    TT_HIP(c, hipMemcpy(c->scene.tris_raw.p, tris, sizeof(tt_cuda_triangle) * n_tris, hipMemcpyHostToDevice));
    TT_HIP(c, hipMemcpy(c->scene.tris.p, tp.data(), sizeof(TriPos) * n_tris, hipMemcpyHostToDevice));
    return scene_commit(c, std::move(h), tags, mg, any_invisible, sz);
}

tt_status tt_object_validate(const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris, uint32_t n_tris,
                             uint32_t root, char* why, uint32_t why_len) {
    tt_asm::ObjectWalk w;
    const tt_status st = tt_asm::validate_object(nodes, n_nodes, tris, n_tris, root, w);
    copy_why(w.why, why, why_len);
    return st;
}

tt_status tt_object_create(tt_ctx* c, const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris,
                           uint32_t n_tris, uint32_t root, tt_object** out) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (!out) return fail(c, TT_ERR_INVALID_ARG, "tt_object_create: null output handle");
    *out = nullptr;
    TT_REFUSE_DEAD_STREAM(c);
    std::unique_ptr<tt_object> o(new tt_object);
    const tt_status vs = tt_asm::validate_object(nodes, n_nodes, tris, n_tris, root, o->walk);
    if (vs != TT_OK) return fail(c, vs, "object validation failed: %s", o->walk.why.c_str());
    if (over_4gib(n_nodes, n_tris)) return fail(c, TT_ERR_INVALID_ARG, "%s", kOver4GiB);
    TT_HIP(c, hipSetDevice(c->device));
    hipError_t e;
    if ((e = o->d_nodes.alloc(n_nodes)) != hipSuccess || (e = o->d_tris.alloc(n_tris)) != hipSuccess ||
        (e = o->d_tripos.alloc(n_tris)) != hipSuccess)
        return hip_fail(c, e, "object allocation");
    TT_HIP(c, hipMemcpy(o->d_nodes.p, nodes, sizeof(tt_cwbvh_node) * n_nodes, hipMemcpyHostToDevice));
    TT_HIP(c, hipMemcpy(o->d_tris.p, tris, sizeof(tt_cuda_triangle) * n_tris, hipMemcpyHostToDevice));
    TT_HIP(c, tt_launch_derive_tripos(o->d_tris.p, o->d_tripos.p, n_tris, c->stream));
    TT_HIP(c, hipStreamSynchronize(c->stream));  // any context's stream may read the object from here on
    o->nodes.assign(nodes, nodes + n_nodes);
    o->device = c->device;
    o->n_nodes = n_nodes;
    o->n_tris = n_tris;
    o->root = root;
    *out = o.release();
    return TT_OK;
}

tt_status tt_object_get_info(const tt_object* o, tt_object_info* info) {
    if (!o || !info) return TT_ERR_INVALID_ARG;
    info->n_nodes = o->n_nodes;
    info->n_tris = o->n_tris;
    info->device = o->device;
    info->root = o->root;
    info->bytes = (uint64_t)o->n_nodes * sizeof(tt_cwbvh_node) + (uint64_t)o->n_tris * (sizeof(tt_cuda_triangle) + sizeof(TriPos));
    return TT_OK;
}

tt_status tt_object_destroy(tt_object* o) {
    if (!o) return TT_ERR_INVALID_ARG;
    delete o;
    return TT_OK;
}

tt_status tt_scene_layout_counts(const uint32_t* n_nodes, const uint32_t* n_tris, uint32_t n, uint32_t tlas_region,
                                 uint32_t* node_offsets, uint32_t* tri_offsets, uint32_t* n_nodes_total,
                                 uint32_t* n_tris_total) {
    std::string why;
    return tt_asm::layout_counts(n_nodes, n_tris, n, tlas_region, node_offsets, tri_offsets, n_nodes_total, n_tris_total, why);
}

tt_status tt_scene_layout_objects(const tt_object* const* objects, uint32_t n, uint32_t tlas_region, uint32_t* node_offsets,
                                  uint32_t* tri_offsets, uint32_t* n_nodes_total, uint32_t* n_tris_total) {
    if (!objects || !n) return TT_ERR_INVALID_ARG;
    std::vector<uint32_t> nn(n), nt(n);
    for (uint32_t i = 0; i < n; i++) {
        if (!objects[i]) return TT_ERR_INVALID_ARG;
        nn[i] = objects[i]->n_nodes;
        nt[i] = objects[i]->n_tris;
    }
    return tt_scene_layout_counts(nn.data(), nt.data(), n, tlas_region, node_offsets, tri_offsets, n_nodes_total, n_tris_total);
}

tt_status tt_scene_assemble_objects(tt_ctx* c, const tt_object* const* objects, uint32_t n_objects,
                                    const tt_cwbvh_node* tlas_nodes, uint32_t tlas_region, const int32_t* tlas,
                                    uint32_t n_tlas, const tt_mesh_data* md, uint32_t n_mesh, const tt_material* mats,
                                    uint32_t n_mat) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER(c);
    TT_REFUSE_LENDER(c);
    c->has_scene = false;
    if (!objects || !n_objects || !tlas_nodes || !tlas_region || !tlas || !n_tlas || !md || !n_mesh || (n_mat && !mats))
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_assemble_objects: null or empty buffer");
    // ---- host: O(objects + TLAS + meshes) checks, nothing per triangle, and no BLAS is walked again
    std::vector<uint32_t> cnt_n(n_objects), cnt_t(n_objects), off_n(n_objects), off_t(n_objects);
    for (uint32_t i = 0; i < n_objects; i++) {
        const tt_object* o = objects[i];
        if (!o) return fail(c, TT_ERR_INVALID_ARG, "tt_scene_assemble_objects: object %u is null", i);
        if (o->device != c->device)
            return fail(c, TT_ERR_INVALID_ARG, "tt_scene_assemble_objects: object %u lives on device %d, the context on %d", i,
                        o->device, c->device);
        cnt_n[i] = o->n_nodes;
        cnt_t[i] = o->n_tris;
    }
    uint32_t n_nodes = 0, n_tris = 0;
    std::string why;
    if (tt_asm::layout_counts(cnt_n.data(), cnt_t.data(), n_objects, tlas_region, off_n.data(), off_t.data(), &n_nodes,
                              &n_tris, why) != TT_OK)
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_assemble_objects: %s", why.c_str());
    if (over_4gib(n_nodes, n_tris)) return fail(c, TT_ERR_INVALID_ARG, "scene validation failed: %s", kOver4GiB);
    for (uint32_t i = 0; i < n_tlas; i++)
        if (tlas[i] < 0 || (uint32_t)tlas[i] >= n_mesh)
            return fail(c, TT_ERR_INVALID_ARG, "scene validation failed: TLASBVH8Indices entry %u (%d) out of range", i, tlas[i]);
    // every mesh record names one object by its (NodeOffset, TriOffset) pair of the layout, and a root that
    // object's own walk reached (so the subtree below it was validated against the object's counts)
    std::vector<uint8_t> used(n_objects, 0u);
    std::vector<tt_check::BlasKey> keys;
    for (uint32_t m = 0; m < n_mesh; m++) {
        const tt_mesh_data& r = md[m];
        if (r.NodeOffset < 0 || r.TriOffset < 0) return fail(c, TT_ERR_INVALID_ARG, "scene validation failed: negative mesh offsets");
        // (node offsets strictly increase: every object has nodes)
        const uint32_t i = (uint32_t)(std::upper_bound(off_n.begin(), off_n.end(), (uint32_t)r.NodeOffset) - off_n.begin());
        if (i == 0 || off_n[i - 1] != (uint32_t)r.NodeOffset || off_t[i - 1] != (uint32_t)r.TriOffset)
            return fail(c, TT_ERR_INVALID_ARG, "scene validation failed: mesh record %u (NodeOffset %d, TriOffset %d) matches no "
                                               "object of the layout", m, r.NodeOffset, r.TriOffset);
        const tt_object* o = objects[i - 1];
        const uint32_t root = (uint32_t)(r.mesh_data_bvh_offsets & 0x7fffffff);
        if (root < off_n[i - 1] || root - off_n[i - 1] >= o->n_nodes || !o->walk.reach[root - off_n[i - 1]])
            return fail(c, TT_ERR_INVALID_ARG, "scene validation failed: mesh record %u: root %u is not a validated node of its "
                                               "object (nodes [%u, %u))", m, root, off_n[i - 1], off_n[i - 1] + o->n_nodes);
        used[i - 1] = 1u;
        keys.push_back(tt_check::key_of(r));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    // the host mirror, composed by memcpy; then the TLAS-level walk over the supplied nodes only
    SceneHost h;
    h.nodes.reserve(n_nodes);
    h.nodes.assign(tlas_nodes, tlas_nodes + tlas_region);
    for (uint32_t i = 0; i < n_objects; i++) h.nodes.insert(h.nodes.end(), objects[i]->nodes.begin(), objects[i]->nodes.end());
    h.tlas.assign(tlas, tlas + n_tlas);
    h.mesh.assign(md, md + n_mesh);
    h.n_tris = n_tris;
    std::vector<uint32_t> tags;
    bool any_invisible = false;
    derive_materials(mats, n_mat, h, tags, any_invisible);
    {
        tt_check::SceneView s = view_of(h);
        s.n_tl = tlas_region;
        Validator v(s);
        if (!v.walk_tlas()) return fail(c, TT_ERR_INVALID_ARG, "scene validation failed: TLAS: %s", v.why.c_str());
        h.blas_ok = keys;
        tt_check::replace_tlas_reach(h.is_tlas_node, h.tlas_nodes, v.tlas_visit, n_nodes);
    }
    h.is_blas_node.assign(n_nodes, 0u);
    for (uint32_t i = 0; i < n_objects; i++)
        if (used[i]) std::memcpy(h.is_blas_node.data() + off_n[i], objects[i]->walk.reach.data(), objects[i]->n_nodes);
    // ---- device: the buffers tt_scene_upload would hold
    TT_HIP(c, hipSetDevice(c->device));
    TT_HIP(c, hipStreamSynchronize(c->stream));  // nothing enqueued still reads the scene being replaced
    std::vector<MeshGpu> mg(n_mesh);
    for (uint32_t m = 0; m < n_mesh; m++) derive_mesh(md[m], mg[m]);
    SceneSizes sz;
    {
        const tt_status st = scene_alloc(c, h, n_nodes, n_tris, tags.size(), tlas_region, sz);
        if (st != TT_OK) return st;
    }
    hipError_t e;
    // the TLAS region from the host; the overlay regions behind the nodes stay as upload leaves them (unwritten
    // in `nodes`, zero in the strided copy)
    TT_HIP(c, hipMemcpy(c->scene.nodes.p, tlas_nodes, sizeof(tt_cwbvh_node) * tlas_region, hipMemcpyHostToDevice));
    TT_HIP(c, refresh_node_copy(c, 0, tlas_region));
    DevBuf<AsmSegment> table;
    std::vector<AsmSegment> seg;  // (outlives the asynchronous table copy: the stream is synchronized below)
    uint32_t ring_slot;
    TT_HIP(c, ring_open(c, c->timing, ring_slot));  // tt_timing_read: the gather's GPU time, in either form
    if (assemble_kernel_form()) {
        seg.reserve((size_t)3 * n_objects);
        uint64_t units = 0;
        auto add = [&](const void* src, void* dst, void* dst_k, uint64_t bytes) {
            AsmSegment g;
            g.src = static_cast<const uint8_t*>(src);
            g.dst = static_cast<uint8_t*>(dst);
            g.dst_k = static_cast<uint8_t*>(dst_k);
            g.bytes = bytes;
            g.pad = 0;
            g.wide = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0 ? 1u : 0u;
            units += (bytes + 15u) / 16u;
            g.unit_end = units;
            seg.push_back(g);
        };
        for (uint32_t i = 0; i < n_objects; i++) {
            const tt_object* o = objects[i];
            add(o->d_nodes.p, c->scene.nodes.p + off_n[i],
                TT_NODE_STRIDE != 80 ? c->scene.nodes_k.p + (size_t)off_n[i] * TT_NODE_STRIDE : nullptr,
                (uint64_t)o->n_nodes * sizeof(tt_cwbvh_node));
            add(o->d_tris.p, c->scene.tris_raw.p + off_t[i], nullptr, (uint64_t)o->n_tris * sizeof(tt_cuda_triangle));
            add(o->d_tripos.p, c->scene.tris.p + off_t[i], nullptr, (uint64_t)o->n_tris * sizeof(TriPos));
        }
        if ((e = table.alloc(seg.size())) != hipSuccess) return hip_fail(c, e, "assembly table");
        TT_HIP(c, hipMemcpyAsync(table.p, seg.data(), sizeof(AsmSegment) * seg.size(), hipMemcpyHostToDevice, c->stream));
        TT_HIP(c, tt_launch_assemble(table.p, (uint32_t)seg.size(), units, c->stream));
    } else {
        for (uint32_t i = 0; i < n_objects; i++) {
            const tt_object* o = objects[i];
            TT_HIP(c, hipMemcpyAsync(c->scene.nodes.p + off_n[i], o->d_nodes.p, sizeof(tt_cwbvh_node) * o->n_nodes,
                                     hipMemcpyDeviceToDevice, c->stream));
            TT_HIP(c, hipMemcpyAsync(c->scene.tris_raw.p + off_t[i], o->d_tris.p, sizeof(tt_cuda_triangle) * o->n_tris,
                                     hipMemcpyDeviceToDevice, c->stream));
            TT_HIP(c, hipMemcpyAsync(c->scene.tris.p + off_t[i], o->d_tripos.p, sizeof(TriPos) * o->n_tris,
                                     hipMemcpyDeviceToDevice, c->stream));
        }
        TT_HIP(c, refresh_node_copy(c, tlas_region, n_nodes - tlas_region));
    }
    TT_HIP(c, ring_close(c, c->timing, ring_slot));
    // (scene_commit synchronizes the stream: after it the objects may be destroyed, the host arrays reused)
    return scene_commit(c, std::move(h), tags, mg, any_invisible, sz);
}

tt_status tt_scene_upload_alpha_atlas(tt_ctx* c, const uint8_t* texels, uint32_t width, uint32_t height) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_BORROWER(c);
    TT_REFUSE_LENDER(c);
    if (!texels || width == 0 || height == 0 || (uint64_t)width * height > 0x7fffffffull)
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_upload_alpha_atlas: empty or oversized atlas");
    TT_HIP(c, hipSetDevice(c->device));
    c->scene.atlas.release();
    c->scene.atlas_w = c->scene.atlas_h = 0;
    TT_HIP(c, c->scene.atlas.alloc((size_t)width * height));
    TT_HIP(c, hipMemcpy(c->scene.atlas.p, texels, (size_t)width * height, hipMemcpyHostToDevice));
    c->scene.atlas_w = width;
    c->scene.atlas_h = height;
    return TT_OK;
}

tt_status tt_scene_upload_texture_atlas(tt_ctx* c, const uint16_t* rgba_half, uint32_t width, uint32_t height) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_BORROWER(c);
    TT_REFUSE_LENDER(c);
    if (!rgba_half || width == 0 || height == 0 || (uint64_t)width * height > 0x7fffffffull / 8u)
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_upload_texture_atlas: empty or oversized atlas");
    TT_HIP(c, hipSetDevice(c->device));
    c->scene.tex.release();
    c->scene.tex_w = c->scene.tex_h = 0;
    TT_HIP(c, c->scene.tex.alloc((size_t)width * height));
    TT_HIP(c, hipMemcpy(c->scene.tex.p, rgba_half, (size_t)width * height * 8u, hipMemcpyHostToDevice));
    c->scene.tex_w = width;
    c->scene.tex_h = height;
    return TT_OK;
}

}  // extern "C"

namespace {
// The refusals tt_ctx_share_scene and tt_ctx_share_blas have in common
tt_status share_refusal(tt_ctx* dst, tt_ctx* src) {
    if (dst == src) return fail(dst, TT_ERR_INVALID_ARG, "a context cannot share its own scene");
    if (!src->has_scene) return fail(dst, TT_ERR_NO_SCENE, "the source context has no scene");
    if (src->lender) return fail(dst, TT_ERR_INVALID_ARG, "the source context shares another context's scene");
    if (dst->borrowers > 0) return fail(dst, TT_ERR_INVALID_ARG, "other contexts share this context's scene");
    if (dst->device != src->device) return fail(dst, TT_ERR_INVALID_ARG, "the contexts are on different devices");
    return TT_OK;
}

// share_refusal; then dst's previous scene ties are cut and the lender's read-only buffers borrowed (everything
// but the TLAS-side buffers an overlay owns).
tt_status share_begin(tt_ctx* dst, tt_ctx* src) {
    const tt_status rs = share_refusal(dst, src);
    if (rs != TT_OK) return rs;
    TT_HIP(dst, hipSetDevice(dst->device));
    TT_HIP(dst, hipStreamSynchronize(dst->stream));  // nothing of dst's still reads its old scene
    TT_HIP(dst, hipStreamSynchronize(src->stream));  // src's upload / updates have landed
    unlink_borrower(dst);
    dst->scene.borrow_shared(src->scene);
    dst->any_invisible = src->any_invisible;
    dst->n_nodes_scene = src->n_nodes_scene;
    dst->n_nodes_dev = src->n_nodes_dev;
    dst->tlas_res = dst->tlas_cap = dst->ovl_stride = 0;  // a borrower never lends
    dst->ovl = false;
    dst->tlas_base = 0;
    dst->n_tlas_own = 0;
    dst->root_known = false;
    return TT_OK;
}

void share_link(tt_ctx* dst, tt_ctx* src) {
    std::lock_guard<std::recursive_mutex> lk(src->mu);
    dst->has_scene = true;
    dst->scene_gen++;
    dst->lender = src;
    src->borrowers++;
    src->borrower_list.push_back(dst);
    if (dst->ovl) src->ovl_used |= 1u << dst->ovl_slot;
    dst->mut_waited = dst->ovl ? src->blas_mut : src->scene_mut;  // src's stream was synchronized above
    dst->read_waited = dst->read_seq;
}
}  // namespace

extern "C" {

// Traces on `dst` read `src`'s scene buffers (nodes, triangles, TLAS, mesh and leaf records, materials,
// atlases) instead of a copy: two contexts tracing concurrently (the two-part layout) then share one
// cache footprint. The borrowed buffers are read-only for `dst`.
tt_status tt_ctx_share_scene(tt_ctx* dst, tt_ctx* src) {
    if (!dst || !src) return TT_ERR_INVALID_ARG;
    const tt_status st = share_begin(dst, src);
    if (st != TT_OK) return st;
    dst->scene.borrow_tlas_side(src->scene);
    copy_host_light(dst->host, src->host);
    share_link(dst, src);
    return TT_OK;
}

// A frame slot's own TLAS over `src`'s BLASes (include/truetrace_hip.h). The TLAS nodes [0, n_tlas_nodes) are
// copied from src's device array into a free overlay region behind the scene's nodes, TLASBVH8Indices and
// _MeshData (+ MeshGpu, LeafMesh) into buffers of dst's own; the kernels address the copy through
// TraceArgs::tlas_base (the TLAS-level NodeOffset), so the BLAS nodes and triangles stay one shared copy.
tt_status tt_ctx_share_blas(tt_ctx* dst, tt_ctx* src, uint32_t n_tlas_nodes) {
    if (!dst || !src) return TT_ERR_INVALID_ARG;
    {
        const tt_status rs = share_refusal(dst, src);
        if (rs != TT_OK) return rs;
    }
    if (src->tlas_res == 0)
        return fail(dst, TT_ERR_UNSUPPORTED, "the source scene has no overlay regions (TT_NODE_STRIDE != 80, or a node "
                                             "array near the 32-bit offset limit)");
    if (n_tlas_nodes == 0 || n_tlas_nodes > src->tlas_res)
        return fail(dst, TT_ERR_INVALID_ARG, "tt_ctx_share_blas: n_tlas_nodes %u outside (0, %u] (the TLAS region)",
                    n_tlas_nodes, src->tlas_res);
    // Everything that can fail on src's side -- the TLAS read-back and walk, the overlay buffers -- happens
    // before dst is touched, so a refused call leaves dst as it was. The TLAS-side state is taken
    // as the device holds it now (a device TLAS refit leaves src's host copy stale).
    TT_HIP(dst, hipSetDevice(dst->device));
    TT_HIP(dst, hipStreamSynchronize(src->stream));
    SceneHost h;
    {
        std::lock_guard<std::recursive_mutex> lk(src->mu);
        copy_host_light(h, src->host);
        h.tlas = src->host.tlas;
        h.mesh = src->host.mesh;
        h.blas_ok = src->host.blas_ok;
    }
    h.nodes.resize(n_tlas_nodes);
    TT_HIP(dst, hipMemcpy(h.nodes.data(), src->scene.nodes.p, sizeof(tt_cwbvh_node) * n_tlas_nodes, hipMemcpyDeviceToHost));
    {
        std::lock_guard<std::recursive_mutex> lk(src->mu);
        Validator v(view_of(h, src->host));
        if (!v.walk_tlas())
            return fail(dst, TT_ERR_INVALID_ARG, "tt_ctx_share_blas: the TLAS leaves [0, %u): %s", n_tlas_nodes, v.why.c_str());
        tt_check::replace_tlas_reach(h.is_tlas_node, h.tlas_nodes, v.tlas_visit, n_tlas_nodes);
    }
    const uint32_t n_tlas = (uint32_t)h.tlas.size(), n_mesh = (uint32_t)h.mesh.size();
    struct Fresh {  // dst's own TLAS-side buffers, adopted once nothing can fail any more
        DevBuf<int32_t> tlas;
        DevBuf<tt_mesh_data> mesh_raw;
        DevBuf<MeshGpu> mesh;
        DevBuf<LeafMesh> leaf;
    } fr;
    hipError_t e;
    if ((e = fr.tlas.alloc(n_tlas)) != hipSuccess || (e = fr.mesh_raw.alloc(n_mesh)) != hipSuccess ||
        (e = fr.mesh.alloc(n_mesh)) != hipSuccess || (e = fr.leaf.alloc(src->scene.leaf.n)) != hipSuccess)
        return hip_fail(dst, e, "overlay TLAS-side buffers");
    // the overlay region: picked and reserved in one locked section (two frame slots made concurrently
    // over one lender never get the same region); a re-share over the same lender keeps its region
    uint32_t slot = TT_TLAS_SLOTS;
    const bool same_slot = dst->ovl && dst->lender == src;
    {
        std::lock_guard<std::recursive_mutex> lk(src->mu);
        if (same_slot) {
            slot = dst->ovl_slot;
        } else {
            for (uint32_t k = 0; k < TT_TLAS_SLOTS; k++)
                if (!((src->ovl_used >> k) & 1u)) {
                    slot = k;
                    break;
                }
            if (slot == TT_TLAS_SLOTS)
                return fail(dst, TT_ERR_UNSUPPORTED, "all %u overlay regions of the source scene are in use", TT_TLAS_SLOTS);
            src->ovl_used |= 1u << slot;
        }
    }
    auto release_slot = [&] {
        if (same_slot) return;
        std::lock_guard<std::recursive_mutex> lk(src->mu);
        src->ovl_used &= ~(1u << slot);
    };
    if (same_slot) {
        // unlink_borrower (in share_begin) frees the region bit: keep it reserved across the re-share
        std::lock_guard<std::recursive_mutex> lk(src->mu);
        dst->ovl = false;
    }
    const tt_status st = share_begin(dst, src);
    if (st != TT_OK) {
        if (same_slot) {
            std::lock_guard<std::recursive_mutex> lk(src->mu);
            if (dst->lender == src)
                dst->ovl = true;  // failed before unlinking: dst keeps its frame slot as it was
            else
                src->ovl_used &= ~(1u << slot);  // unlinked, then failed: the region goes with it
        } else {
            release_slot();
        }
        return st;
    }
    dst->scene.tlas = std::move(fr.tlas);
    dst->scene.mesh_raw = std::move(fr.mesh_raw);
    dst->scene.mesh = std::move(fr.mesh);
    dst->scene.leaf = std::move(fr.leaf);
    dst->host = std::move(h);
    dst->ovl = true;
    dst->ovl_slot = slot;
    dst->n_tlas_own = n_tlas_nodes;
    dst->tlas_base = src->n_nodes_scene + slot * src->ovl_stride;
    // device copies: a failure here leaves dst with no scene at all (never a half-linked one)
    auto abort_share = [&](hipError_t err, const char* what) {
        (void)hipStreamSynchronize(dst->stream);
        dst->has_scene = false;
        dst->ovl = false;
        dst->tlas_base = 0;
        dst->n_tlas_own = 0;
        dst->root_known = false;
        dst->host = SceneHost{};
        dst->scene = SceneDev{};
        release_slot();
        return hip_fail(dst, err, what);
    };
    if ((e = hipMemcpyAsync(dst->scene.nodes.p + dst->tlas_base, src->scene.nodes.p, sizeof(tt_cwbvh_node) * n_tlas_nodes,
                            hipMemcpyDeviceToDevice, dst->stream)) != hipSuccess ||
        (e = refresh_node_copy(dst, dst->tlas_base, n_tlas_nodes)) != hipSuccess ||
        (e = hipMemcpyAsync(dst->scene.tlas.p, src->scene.tlas.p, sizeof(int32_t) * n_tlas, hipMemcpyDeviceToDevice, dst->stream)) !=
            hipSuccess ||
        (e = hipMemcpyAsync(dst->scene.mesh_raw.p, src->scene.mesh_raw.p, sizeof(tt_mesh_data) * n_mesh, hipMemcpyDeviceToDevice,
                            dst->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(dst->scene.mesh.p, src->scene.mesh.p, sizeof(MeshGpu) * n_mesh, hipMemcpyDeviceToDevice, dst->stream)) !=
            hipSuccess ||
        (e = hipMemcpyAsync(dst->scene.leaf.p, src->scene.leaf.p, sizeof(LeafMesh) * src->scene.leaf.n, hipMemcpyDeviceToDevice,
                            dst->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(dst->stream)) != hipSuccess)
        return abort_share(e, "tt_ctx_share_blas: overlay copies");
    dst->root_known = true;  // its host TLAS copy is what the device holds
    share_link(dst, src);
    return TT_OK;
}

tt_status tt_tlas_refit(tt_ctx* c, uint32_t n_tlas_nodes, const float* mesh_aabbs, uint32_t n_mesh, uint32_t flags) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER_TLAS(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    // (an overlay borrower's host.nodes are its own TLAS nodes: it refits those, in its overlay region)
    if (!mesh_aabbs || n_tlas_nodes == 0 || n_tlas_nodes > c->host.nodes.size())
        return fail(c, TT_ERR_INVALID_ARG, "tt_tlas_refit: null boxes or n_tlas_nodes out of range");
    if (n_mesh < c->host.mesh.size())
        return fail(c, TT_ERR_INVALID_ARG, "tt_tlas_refit: need one AABB per _MeshData record (%zu)", c->host.mesh.size());
    TT_HIP(c, hipSetDevice(c->device));
    if (c->refit_gen != c->scene_gen || c->refit_n_tlas != n_tlas_nodes) {
        RefitPlan plan;
        if (!tt_refit_build_plan(c->host.nodes.data(), n_tlas_nodes, plan))
            return fail(c, TT_ERR_INVALID_ARG, "tt_tlas_refit: a TLAS child index leaves [0, n_tlas_nodes)");
        TT_HIP(c, hipStreamSynchronize(c->stream));  // the old plan's buffers may be in use
        TT_HIP(c, tt_refit_prepare(plan, c->host.nodes.data(), n_tlas_nodes, c->refit));
        c->refit_gen = c->scene_gen;
        c->refit_n_tlas = n_tlas_nodes;
    }
    const float* d_boxes = mesh_aabbs;
    if (flags & TT_TRACE_DEVICE_PTRS) {
        if (!is_device_ptr(mesh_aabbs)) return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but boxes are not device memory");
    } else {
        TT_HIP(c, stage_in(c, c->st_boxes, mesh_aabbs, (size_t)6 * n_mesh, 0, d_boxes));
    }
    uint32_t slot;
    SceneWrite sw(c, false, !c->ovl);  // (an overlay's TLAS is read by nobody else)
    TT_HIP(c, sw.err);
    TT_HIP(c, ring_open(c, c->timing, slot));
    TT_HIP(c, tt_refit_run(c->refit, d_boxes, c->scene.tlas.p, c->scene.nodes.p + c->tlas_base, c->stream));
    TT_HIP(c, refresh_node_copy(c, c->tlas_base, n_tlas_nodes));
    {
        std::lock_guard<std::recursive_mutex> lk(c->mu);
        c->root_known = false;  // node 0 was rewritten on the device
    }
    TT_HIP(c, ring_close(c, c->timing, slot));
    TT_HIP(c, sw.end());
    if (!(flags & TT_TRACE_ASYNC) || !(flags & TT_TRACE_DEVICE_PTRS)) TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_blas_refit(tt_ctx* c, const tt_blas_refit_params* p, const float* vertices, const int32_t* indices,
                        const int32_t* leaf_of_triangle) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    if (!p || !vertices || !indices || !leaf_of_triangle || !p->n_tris || !p->n_vertices || p->vertex_stride < 6)
        return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit: null array, empty mesh or vertex_stride < 6");
    if (p->mesh_index >= c->host.mesh.size())
        return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit: mesh_index %u out of range", p->mesh_index);
    const tt_mesh_data& md = c->host.mesh[p->mesh_index];
    const uint32_t node_base = (uint32_t)md.NodeOffset, tri_base = (uint32_t)md.TriOffset;
    if ((uint32_t)(md.mesh_data_bvh_offsets & 0x7fffffff) != node_base || node_base >= c->host.nodes.size())
        return fail(c, TT_ERR_UNSUPPORTED, "tt_blas_refit: the mesh's BLAS root is not its first node");
    if ((uint64_t)tri_base + p->n_tris > c->host.n_tris)
        return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit: TriOffset + n_tris exceeds the scene's triangles");
    const bool dev = (p->flags & TT_TRACE_DEVICE_PTRS) != 0;
    if (dev && !(is_device_ptr(vertices) && is_device_ptr(indices) && is_device_ptr(leaf_of_triangle)))
        return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but an array is not device memory");
    if (!dev) {
        for (uint64_t i = 0; i < 3ull * p->n_tris; i++)
            if (indices[i] < 0 || (uint32_t)indices[i] >= p->n_vertices)
                return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit: index %d out of range", indices[i]);
        for (uint32_t i = 0; i < p->n_tris; i++)
            if (leaf_of_triangle[i] < 0 || (uint32_t)leaf_of_triangle[i] >= p->n_tris)
                return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit: leaf_of_triangle[%u] out of range", i);
    }
    TT_HIP(c, hipSetDevice(c->device));
    tt_ctx::BlasRefit& R = c->blas_refit[p->mesh_index];
    if (R.gen != c->scene_gen || R.node_base != node_base || R.boxes.n < (size_t)6 * p->n_tris) {
        RefitPlan plan;
        const tt_cwbvh_node* base = c->host.nodes.data() + node_base;
        if (!tt_refit_build_plan(base, (uint32_t)(c->host.nodes.size() - node_base), plan))
            return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit: a BLAS child index leaves the node array");
        if ((uint32_t)plan.leaf_end > p->n_tris)
            return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit: the BLAS references triangle %d beyond n_tris", plan.leaf_end - 1);
        uint32_t n_used = 0;
        for (int32_t b : plan.pair_bvh) n_used = std::max(n_used, (uint32_t)b + 1u);
        TT_HIP(c, hipStreamSynchronize(c->stream));  // the old plan's buffers may be in use
        TT_HIP(c, tt_refit_prepare(plan, base, n_used, R.dev));
        R.n_nodes = n_used;
        if (R.boxes.n < (size_t)6 * p->n_tris) TT_HIP(c, R.boxes.alloc((size_t)6 * p->n_tris));
        R.gen = c->scene_gen;
        R.node_base = node_base;
    }
    BlasConstructArgs a{};
    a.vertices = vertices;
    a.indices = indices;
    a.leaf_of = leaf_of_triangle;
    if (!dev) {
        TT_HIP(c, stage_in(c, c->st_vtx, vertices, (size_t)p->n_vertices * p->vertex_stride, 0, a.vertices));
        TT_HIP(c, stage_in(c, c->st_idx, indices, (size_t)3 * p->n_tris, 0, a.indices));
        TT_HIP(c, stage_in(c, c->st_leaf, leaf_of_triangle, p->n_tris, 0, a.leaf_of));
    }
    a.n_tris = p->n_tris;
    a.n_vertices = p->n_vertices;
    a.vertex_stride = p->vertex_stride;
    std::memcpy(a.m, p->transform, sizeof(a.m));
    a.boxes = R.boxes.p;
    a.tris88 = c->scene.tris_raw.p + tri_base;
    a.tripos = c->scene.tris.p + tri_base;
    uint32_t slot;
    SceneWrite sw(c, true);
    TT_HIP(c, sw.err);
    TT_HIP(c, ring_open(c, c->timing, slot));
    TT_HIP(c, tt_blas_construct(a, c->stream));
    TT_HIP(c, tt_refit_run(R.dev, R.boxes.p, nullptr, c->scene.nodes.p + node_base, c->stream));
    TT_HIP(c, refresh_node_copy(c, node_base, R.n_nodes));
    TT_HIP(c, ring_close(c, c->timing, slot));
    TT_HIP(c, sw.end());
    if (!(p->flags & TT_TRACE_ASYNC) || !dev) TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_blas_refit_items_validate(const tt_blas_refit_item* items, uint32_t n_items, const tt_mesh_data* md,
                                       uint32_t n_mesh, uint32_t n_scene_tris, uint32_t flags, char* why, uint32_t why_len) {
    std::string w;
    const tt_status st = tt_refit_items::check(items, n_items, md, n_mesh, n_scene_tris, flags, w);
    copy_why(w, why, why_len);
    return st;
}

namespace {
// The composed plan of an item list: per-mesh host plans (built once per scene generation), one forest on the
// device, the box pool. Called only when the list or the scene changed; nothing is enqueued by it.
tt_status compose_refit_many(tt_ctx* c, const tt_blas_refit_item* items, uint32_t n_items, const std::vector<uint32_t>& key) {
    tt_ctx::BlasRefitMany& M = c->refit_many;
    std::vector<RefitForestItem> forest(n_items);
    std::vector<uint32_t> box_base(n_items);
    uint64_t n_pairs = 0;
    uint32_t total = 0;
    std::vector<std::pair<uint32_t, uint32_t>> spans;  // [first node, end) of each item's BLAS
    for (uint32_t i = 0; i < n_items; i++) {
        const tt_mesh_data& md = c->host.mesh[items[i].mesh_index];
        const uint32_t node_base = (uint32_t)md.NodeOffset;
        tt_ctx::BlasPlanHost& P = c->many_plans[items[i].mesh_index];
        if (P.gen != c->scene_gen || P.node_base != node_base) {
            P.gen = ~0ull;
            if (!tt_refit_build_plan(c->host.nodes.data() + node_base, (uint32_t)(c->host.nodes.size() - node_base), P.plan))
                return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit_many: item %u: a BLAS child index leaves the node array", i);
            P.n_nodes = 0;
            for (int32_t b : P.plan.pair_bvh) P.n_nodes = std::max(P.n_nodes, (uint32_t)b + 1u);
            P.gen = c->scene_gen;
            P.node_base = node_base;
        }
        if ((uint32_t)P.plan.leaf_end > items[i].n_tris)
            return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit_many: item %u: the BLAS references triangle %d beyond n_tris", i,
                        P.plan.leaf_end - 1);
        forest[i] = RefitForestItem{&P.plan, node_base, P.n_nodes, total};
        box_base[i] = total;
        total += items[i].n_tris;
        n_pairs += P.plan.pair_bvh.size();
        spans.emplace_back(node_base, node_base + P.n_nodes);
    }
    // the kernel-layout node copy is refreshed per BLAS, adjacent ones as one range: never the BLASes in between
    std::sort(spans.begin(), spans.end());
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    for (const auto& s : spans) {
        if (!ranges.empty() && s.first <= ranges.back().second)
            ranges.back().second = std::max(ranges.back().second, s.second);
        else
            ranges.push_back(s);
    }
    if (n_pairs >= (1ull << 26))
        return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit_many: the composed plan has %llu NodePairs (limit 2^26)",
                    (unsigned long long)n_pairs);
    M.gen = ~0ull;
    TT_HIP(c, hipStreamSynchronize(c->stream));  // the old plan's buffers may be in use
    TT_HIP(c, tt_refit_prepare_forest(forest, M.dev));
    if (M.boxes.n < (size_t)6 * total) TT_HIP(c, M.boxes.alloc((size_t)6 * total));
    M.key = key;
    M.box_base = std::move(box_base);
    M.node_ranges = std::move(ranges);
    M.gen = c->scene_gen;
    return TT_OK;
}
}  // namespace

tt_status tt_blas_refit_many(tt_ctx* c, const tt_blas_refit_item* items, uint32_t n_items, uint32_t flags, float* bounds_out,
                             float* mesh_aabbs) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    if (flags & ~(uint32_t)(TT_TRACE_DEVICE_PTRS | TT_TRACE_ASYNC)) return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit_many: unknown flag");
    {
        std::string why;
        const tt_status st = tt_refit_items::check(items, n_items, c->host.mesh.data(), (uint32_t)c->host.mesh.size(),
                                                   c->host.n_tris, flags, why);
        if (st != TT_OK) return fail(c, st, "tt_blas_refit_many: %s", why.c_str());
    }
    const bool dev = (flags & TT_TRACE_DEVICE_PTRS) != 0;
    uint32_t n_parts = 0, n_blocks = 0;
    size_t n_vtx = 0, n_idx = 0, n_leaf = 0;  // what a host-pointer call stages, in elements
    for (uint32_t i = 0; i < n_items; i++) {
        const tt_blas_refit_item& it = items[i];
        if ((uint32_t)c->host.mesh[it.mesh_index].NodeOffset >= c->host.nodes.size())
            return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit_many: item %u: the record's NodeOffset %d lies beyond the scene's %zu nodes", i,
                        c->host.mesh[it.mesh_index].NodeOffset, c->host.nodes.size());
        if (dev && !is_device_ptr(it.leaf_of_triangle))
            return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit_many: item %u: TT_TRACE_DEVICE_PTRS set but leaf_of_triangle is not device memory", i);
        n_leaf += it.n_tris;
        for (uint32_t k = 0; k < it.n_parts; k++) {
            const tt_blas_refit_part& p = it.parts[k];
            if (dev && !(is_device_ptr(p.vertices) && is_device_ptr(p.indices)))
                return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit_many: item %u part %u: TT_TRACE_DEVICE_PTRS set but an array is not device memory", i, k);
            n_blocks += (p.n_tris + 255u) / 256u;
            n_vtx += (size_t)p.n_vertices * p.vertex_stride;
            n_idx += (size_t)3 * p.n_tris;
        }
        n_parts += it.n_parts;
    }
    if (dev && ((bounds_out && !is_device_ptr(bounds_out)) || (mesh_aabbs && !is_device_ptr(mesh_aabbs))))
        return fail(c, TT_ERR_INVALID_ARG, "tt_blas_refit_many: TT_TRACE_DEVICE_PTRS set but bounds_out or mesh_aabbs is not device memory");
    TT_HIP(c, hipSetDevice(c->device));
    tt_ctx::BlasRefitMany& M = c->refit_many;
    {
        // (the record's NodeOffset is part of the key: tt_scene_update_meshdata may re-point a record at another
        // BLAS without a new scene generation, and the forest addresses nodes)
        bool same = M.gen == c->scene_gen && M.key.size() == (size_t)3 * n_items;
        for (uint32_t i = 0; same && i < n_items; i++)
            same = M.key[3 * i] == items[i].mesh_index && M.key[3 * i + 1] == items[i].n_tris &&
                   M.key[3 * i + 2] == (uint32_t)c->host.mesh[items[i].mesh_index].NodeOffset;
        if (!same) {
            std::vector<uint32_t> key((size_t)3 * n_items);
            for (uint32_t i = 0; i < n_items; i++) {
                key[3 * i] = items[i].mesh_index;
                key[3 * i + 1] = items[i].n_tris;
                key[3 * i + 2] = (uint32_t)c->host.mesh[items[i].mesh_index].NodeOffset;
            }
            const tt_status st = compose_refit_many(c, items, n_items, key);
            if (st != TT_OK) return st;
        }
    }
    // ---- host arrays: staged into the context's buffers (sized first: growing one drops what it held)
    const float* d_vtx = nullptr;
    const int32_t *d_idx = nullptr, *d_leaf = nullptr;
    float *d_bounds = bounds_out, *d_aabbs = mesh_aabbs;
    const size_t n_mesh = c->host.mesh.size();
    if (!dev) {
        TT_HIP(c, stage_in(c, c->st_vtx, nullptr, n_vtx, 0, d_vtx));
        TT_HIP(c, stage_in(c, c->st_idx, nullptr, n_idx, 0, d_idx));
        TT_HIP(c, stage_in(c, c->st_leaf, nullptr, n_leaf, 0, d_leaf));
        if (bounds_out) {
            if (M.bounds.n < (size_t)6 * n_items) TT_HIP(c, M.bounds.alloc((size_t)6 * n_items));
            d_bounds = M.bounds.p;
        }
        if (mesh_aabbs) {
            const float* in = nullptr;
            TT_HIP(c, stage_in(c, c->st_boxes, mesh_aabbs, 6 * n_mesh, 0, in));  // the slots no item writes keep their values
            d_aabbs = c->st_boxes.p;
        }
    }
    // ---- the call's descriptors, composed in the pinned slot and copied to the device on the stream. One mesh of
    // one renderer takes tt_blas_refit's own Construct kernel and carries its item in the refit's kernel arguments:
    // no staging and no copy, so the batch form costs the one-mesh case nothing (profiles/r19/refit_batch)
    const bool direct = n_items == 1 && n_parts == 1;
    const size_t items_off = (size_t)n_parts * sizeof(RefitManyPart), blocks_off = items_off + (size_t)n_items * sizeof(RefitManyItem);
    const size_t bytes = blocks_off + (size_t)n_blocks * sizeof(RefitManyBlock);
    RefitManyPart one_part;
    RefitManyItem one_item;
    void* pinned = nullptr;
    if (!direct) {
        if (M.desc.n < bytes) TT_HIP(c, M.desc.alloc(bytes + bytes / 2));
        TT_HIP(c, stage_begin(c, nullptr, bytes, pinned));
    }
    RefitManyPart* hp = direct ? &one_part : static_cast<RefitManyPart*>(pinned);
    RefitManyItem* hi = direct ? &one_item : reinterpret_cast<RefitManyItem*>(static_cast<uint8_t*>(pinned) + items_off);
    RefitManyBlock* hb = direct ? nullptr : reinterpret_cast<RefitManyBlock*>(static_cast<uint8_t*>(pinned) + blocks_off);
    size_t o_vtx = 0, o_idx = 0, o_leaf = 0;
    uint32_t part = 0, block = 0;
    for (uint32_t i = 0; i < n_items; i++) {
        const tt_blas_refit_item& it = items[i];
        const uint32_t tri_base = (uint32_t)c->host.mesh[it.mesh_index].TriOffset;
        const int32_t* leaf = it.leaf_of_triangle;
        if (!dev) {
            TT_HIP(c, hipMemcpyAsync(c->st_leaf.p + o_leaf, it.leaf_of_triangle, sizeof(int32_t) * it.n_tris, hipMemcpyHostToDevice, c->stream));
            leaf = d_leaf + o_leaf;
            o_leaf += it.n_tris;
        }
        for (uint32_t k = 0; k < it.n_parts; k++, part++) {
            const tt_blas_refit_part& p = it.parts[k];
            RefitManyPart& a = hp[part];
            a.vertices = p.vertices;
            a.indices = p.indices;
            if (!dev) {
                const size_t nv = (size_t)p.n_vertices * p.vertex_stride, ni = (size_t)3 * p.n_tris;
                TT_HIP(c, hipMemcpyAsync(c->st_vtx.p + o_vtx, p.vertices, sizeof(float) * nv, hipMemcpyHostToDevice, c->stream));
                TT_HIP(c, hipMemcpyAsync(c->st_idx.p + o_idx, p.indices, sizeof(int32_t) * ni, hipMemcpyHostToDevice, c->stream));
                a.vertices = d_vtx + o_vtx;
                a.indices = d_idx + o_idx;
                o_vtx += nv;
                o_idx += ni;
            }
            a.leaf_of = leaf + p.first_tri;
            a.boxes = M.boxes.p + (size_t)6 * M.box_base[i];
            a.tris88 = c->scene.tris_raw.p + tri_base;
            a.tripos = c->scene.tris.p + tri_base;
            a.n_tris = p.n_tris;
            a.n_vertices = p.n_vertices;
            a.vertex_stride = p.vertex_stride;
            a.leaf_bound = it.n_tris;
            std::memcpy(a.m, p.transform, sizeof(a.m));
            for (uint32_t first = 0; hb && first < p.n_tris; first += 256u) hb[block++] = RefitManyBlock{part, first};
        }
        RefitManyItem& r = hi[i];
        std::memset(&r, 0, sizeof(r));
        r.mesh_index = it.mesh_index;
        r.has_l2w = it.local_to_world != nullptr;
        if (it.local_to_world) std::memcpy(r.l2w, it.local_to_world, sizeof(r.l2w));
    }
    if (!direct) {
        TT_HIP(c, hipMemcpyAsync(M.desc.p, pinned, bytes, hipMemcpyHostToDevice, c->stream));
        TT_HIP(c, stage_end(c));
    }
    uint32_t slot;
    SceneWrite sw(c, true);
    TT_HIP(c, sw.err);
    TT_HIP(c, ring_open(c, c->timing, slot));
    if (direct) {
        BlasConstructArgs a{};
        a.vertices = one_part.vertices;
        a.indices = one_part.indices;
        a.leaf_of = one_part.leaf_of;
        a.n_tris = one_part.n_tris;  // (= the item's count: the one part tiles the mesh)
        a.n_vertices = one_part.n_vertices;
        a.vertex_stride = one_part.vertex_stride;
        std::memcpy(a.m, one_part.m, sizeof(a.m));
        a.boxes = one_part.boxes;
        a.tris88 = one_part.tris88;
        a.tripos = one_part.tripos;
        TT_HIP(c, tt_blas_construct(a, c->stream));
        TT_HIP(c, tt_refit_run_forest(M.dev, M.boxes.p, c->scene.nodes.p, nullptr, &one_item, d_bounds, d_aabbs, c->stream));
    } else {
        TT_HIP(c, tt_blas_construct_many(reinterpret_cast<const RefitManyPart*>(M.desc.p),
                                         reinterpret_cast<const RefitManyBlock*>(M.desc.p + blocks_off), n_blocks, c->stream));
        TT_HIP(c, tt_refit_run_forest(M.dev, M.boxes.p, c->scene.nodes.p, reinterpret_cast<const RefitManyItem*>(M.desc.p + items_off),
                                      nullptr, d_bounds, d_aabbs, c->stream));
    }
    if (TT_NODE_STRIDE != 80)
        for (const auto& r : M.node_ranges) TT_HIP(c, refresh_node_copy(c, r.first, r.second - r.first));
    TT_HIP(c, ring_close(c, c->timing, slot));
    TT_HIP(c, sw.end());
    if (!dev) {
        if (bounds_out) TT_HIP(c, stage_out(c, bounds_out, d_bounds, (size_t)6 * n_items));
        if (mesh_aabbs) TT_HIP(c, stage_out(c, mesh_aabbs, d_aabbs, 6 * n_mesh));
    }
    if (!(flags & TT_TRACE_ASYNC) || !dev) TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_scene_read_tris(tt_ctx* c, uint32_t first, uint32_t count, tt_cuda_triangle* out) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    if (!out || (uint64_t)first + count > c->host.n_tris)
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_read_tris: range out of bounds");
    TT_HIP(c, hipSetDevice(c->device));
    SceneRead sr(c);
    TT_HIP(c, sr.err);
    TT_HIP(c, hipMemcpyAsync(out, c->scene.tris_raw.p + first, sizeof(tt_cuda_triangle) * count, hipMemcpyDeviceToHost, c->stream));
    sr.end();
    TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_scene_read_nodes(tt_ctx* c, uint32_t first, uint32_t count, tt_cwbvh_node* out) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    if (!out || (uint64_t)first + count > c->n_nodes_scene)
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_read_nodes: range out of bounds");
    TT_HIP(c, hipSetDevice(c->device));
    SceneRead sr(c);
    TT_HIP(c, sr.err);
    // the scene as this context traces it: an overlay borrower's TLAS nodes [0, n_tlas_own) from its region
    const uint32_t own_end = c->ovl ? std::max(first, std::min(first + count, c->n_tlas_own)) : first;
    if (own_end > first)
        TT_HIP(c, hipMemcpyAsync(out, c->scene.nodes.p + c->tlas_base + first, sizeof(tt_cwbvh_node) * (own_end - first),
                                 hipMemcpyDeviceToHost, c->stream));
    if (first + count > own_end)
        TT_HIP(c, hipMemcpyAsync(out + (own_end - first), c->scene.nodes.p + own_end,
                                 sizeof(tt_cwbvh_node) * (first + count - own_end), hipMemcpyDeviceToHost, c->stream));
    sr.end();
    TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_scene_validate(const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris, uint32_t n_tris,
                            const int32_t* tlas, uint32_t n_tlas, const tt_mesh_data* md, uint32_t n_mesh,
                            const tt_material* mats, uint32_t n_mat, char* why, uint32_t why_len) {
    SceneHost h;
    std::vector<uint32_t> tags;
    bool any_invisible = false;
    std::string w;
    const tt_status st = check_scene(nodes, n_nodes, tris, n_tris, tlas, n_tlas, md, n_mesh, mats, n_mat, h, tags,
                                     any_invisible, w);
    copy_why(w, why, why_len);
    return st;
}

tt_status tt_scene_update_nodes(tt_ctx* c, uint32_t first, uint32_t count, const tt_cwbvh_node* nodes) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER_TLAS(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    if (!nodes || (uint64_t)first + count > c->host.nodes.size())
        return fail(c, TT_ERR_INVALID_ARG, c->ovl ? "node update range out of bounds: a frame-slot TLAS (tt_ctx_share_blas) "
                                                    "rewrites only its own TLAS nodes"
                                                  : "node update range out of bounds");
    if (count == 0) return TT_OK;
    SceneHost& h = c->host;
    tt_ctx* L = c->ovl ? c->lender : nullptr;
    bool tlas_only = true, blas_side = false;
    {
        std::lock_guard<std::recursive_mutex> lk(L ? L->mu : c->mu);  // the nodes the walks read; node 0 (TT_ROOT_LEAF)
        std::vector<tt_cwbvh_node> saved(h.nodes.begin() + first, h.nodes.begin() + first + count);
        std::copy(nodes, nodes + count, h.nodes.begin() + first);
        // A rewrite of TLAS-level nodes only (the per-frame case: BVH8AggregatedBuffer.SetData of the
        // TLAS region) re-walks the TLAS level; the BLASes were validated at upload and are unchanged.
        // Any other rewrite re-validates the whole scene.
        // (a node that a validated BLAS also reaches -- a TLAS rewrite may have re-pointed a child into one
        // -- takes the full check: its triangle indices matter at BLAS level)
        // blas_side: the rewrite touches what frame-slot TLASes read too (a BLAS node, or a node outside the
        // TLAS region); on a frame slot every node of its range is its own TLAS region's
        const std::vector<uint8_t>& blas_nodes = L ? L->host.is_blas_node : h.is_blas_node;
        for (uint32_t i = first; i < first + count; i++) {
            tlas_only = tlas_only && (L || h.is_tlas_node[i] != 0) && blas_nodes[i] == 0;
            blas_side = blas_side || blas_nodes[i] != 0 || (!L && i >= c->tlas_res);
        }
        const char* refuse = nullptr;
        if (!tlas_only && L) refuse = "a frame-slot TLAS (tt_ctx_share_blas) rewrites TLAS nodes only";
        if (blas_side && !L && c->ovl_used)
            refuse = "a BLAS-side node rewrite while frame-slot TLASes (tt_ctx_share_blas) share this scene";
        if (refuse) {
            std::copy(saved.begin(), saved.end(), h.nodes.begin() + first);
            return fail(c, L ? TT_ERR_INVALID_ARG : TT_ERR_UNSUPPORTED, "%s", refuse);
        }
        Validator v(view_of(c));
        const bool ok = tlas_only ? v.walk_tlas() : v.run();
        if (!ok) {
            std::copy(saved.begin(), saved.end(), h.nodes.begin() + first);
            return fail(c, TT_ERR_INVALID_ARG, "scene validation failed after node update: %s", v.why.c_str());
        }
        if (tlas_only) tt_check::replace_tlas_reach(h.is_tlas_node, h.tlas_nodes, v.tlas_visit, 0);
        else tt_check::remember_validation(h, v, h.nodes.size());
        if (first == 0) c->root_known = true;  // node 0 is the host's again
    }
    TT_HIP(c, hipSetDevice(c->device));
    void* pinned = nullptr;
    TT_HIP(c, stage_begin(c, nodes, sizeof(tt_cwbvh_node) * count, pinned));
    SceneWrite sw(c, blas_side, !c->ovl);
    TT_HIP(c, sw.err);
    TT_HIP(c, hipMemcpyAsync(c->scene.nodes.p + c->tlas_base + first, pinned, sizeof(tt_cwbvh_node) * count,
                             hipMemcpyHostToDevice, c->stream));
    TT_HIP(c, stage_end(c));
    TT_HIP(c, refresh_node_copy(c, c->tlas_base + first, count));
    TT_HIP(c, sw.end());
    c->scene_gen++;  // a rewritten TLAS may have a new topology: the refit plan is rebuilt
    return TT_OK;
}

tt_status tt_scene_update_meshdata(tt_ctx* c, uint32_t first, uint32_t count, const tt_mesh_data* md) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER_TLAS(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    if (!md || (uint64_t)first + count > c->host.mesh.size())
        return fail(c, TT_ERR_INVALID_ARG, "meshdata update range out of bounds");
    if (count == 0) return TT_OK;
    SceneHost& h = c->host;
    tt_ctx* L = c->ovl ? c->lender : nullptr;  // a frame-slot TLAS: its records, the lender's BLASes
    // Only records whose BLAS reference (root, NodeOffset, TriOffset) changed need a check, and only
    // against the BLASes validated so far; a BLAS never seen is walked once and remembered. The
    // per-frame transform update (MeshDataBuffer.SetData, AssetManager.cs:1825) changes none.
    std::vector<tt_check::BlasKey> added;
    for (uint32_t i = 0; i < count; i++) {
        const tt_mesh_data& r = md[i];
        const tt_mesh_data& o = h.mesh[first + i];
        if (r.NodeOffset == o.NodeOffset && r.TriOffset == o.TriOffset &&
            ((r.mesh_data_bvh_offsets ^ o.mesh_data_bvh_offsets) & 0x7fffffff) == 0)
            continue;
        if (r.NodeOffset < 0 || r.TriOffset < 0)
            return fail(c, TT_ERR_INVALID_ARG, "scene validation failed after meshdata update: negative mesh offsets");
        const tt_check::BlasKey k = tt_check::key_of(r);
        if (std::binary_search(h.blas_ok.begin(), h.blas_ok.end(), k) ||
            std::find(added.begin(), added.end(), k) != added.end())
            continue;
        std::lock_guard<std::recursive_mutex> lk(L ? L->mu : c->mu);
        Validator v(view_of(c));
        if (!v.walk_mesh(r))
            return fail(c, TT_ERR_INVALID_ARG, "scene validation failed after meshdata update: %s", v.why.c_str());
        added.push_back(k);
        // (kept even if a later record fails: conservative; an overlay's BLASes are marked in the lender's
        // bookkeeping, so a later lender rewrite of those nodes is refused while overlays exist)
        std::vector<uint8_t>& blas_nodes = L ? L->host.is_blas_node : h.is_blas_node;
        for (uint32_t n : v.blas_visit) blas_nodes[n] = 1u;
    }
    if (!added.empty()) {
        h.blas_ok.insert(h.blas_ok.end(), added.begin(), added.end());
        std::sort(h.blas_ok.begin(), h.blas_ok.end());
    }
    // the lights index _MeshData (LightNodeOffset, TriOffset): a record that moves either is checked with them
    if (c->scene.n_lnodes != 0 && !c->ovl) {
        bool moved = false;
        for (uint32_t i = 0; i < count && !moved; i++)
            moved = md[i].LightNodeOffset != h.mesh[first + i].LightNodeOffset || md[i].TriOffset != h.mesh[first + i].TriOffset;
        if (moved) {
            std::vector<tt_mesh_data> next = h.mesh;
            std::memcpy(next.data() + first, md, sizeof(tt_mesh_data) * count);
            const SceneDev& d = c->scene;
            std::string why;
            if (tt_lcheck::validate(tt_lcheck::Lights{d.lnodes_host.data(), (uint32_t)d.lnodes_host.size(), d.ltris_host.data(),
                                                      (uint32_t)d.ltris_host.size(), d.lmeshes_host.data(),
                                                      (uint32_t)d.lmeshes_host.size()},
                                    next.data(), (uint32_t)next.size(), h.n_tris, why) != TT_OK)
                return fail(c, TT_ERR_INVALID_ARG, "light validation failed after meshdata update: %s", why.c_str());
            c->scene.lrefit.plan_valid = false;  // a tree moved: the next tt_lights_refit rebuilds its plan
        }
    }
    std::memcpy(h.mesh.data() + first, md, sizeof(tt_mesh_data) * count);
    TT_HIP(c, hipSetDevice(c->device));
    // one small kernel on the stream reads the records in place from the pinned staging slot, stores them
    // to _MeshData in HBM, derives the traversal records (MeshGpu) and patches the TLAS leaf records that
    // name an updated mesh (no copy operation: each one waits for a free CU slot beside the trace grids)
    void* pinned = nullptr;
    TT_HIP(c, stage_begin(c, md, sizeof(tt_mesh_data) * count, pinned));
    SceneWrite sw(c, false, !c->ovl);  // (an overlay's records are read by nobody else)
    TT_HIP(c, sw.err);
    void* src = nullptr;
    TT_HIP(c, hipHostGetDevicePointer(&src, pinned, 0));
    const uint32_t n_tlas = (uint32_t)h.tlas.size();
    const uint32_t n = std::max(count, n_tlas);
    hipLaunchKernelGGL(tt_update_mesh_kernel, dim3((n + 255u) / 256u), dim3(256), 0, c->stream,
                       static_cast<const tt_mesh_data*>(src), c->scene.mesh_raw.p, c->scene.mesh.p, c->scene.leaf.p, c->scene.tlas.p, n_tlas, first,
                       count);
    TT_HIP(c, hipGetLastError());
    TT_HIP(c, stage_end(c));  // (after the kernel: it reads the staging slot)
    TT_HIP(c, sw.end());
    return TT_OK;
}

}  // extern "C"

namespace {
// What a TLAS installation on `c` may write: the capacity of its TLAS region and the nodes of it in use now.
// A scene of its own: the leading nodes no validated BLAS walk reaches (a _MeshData update since the upload may
// have claimed some); a frame slot: its overlay region, and its own TLAS nodes.
void tlas_region_of(tt_ctx* c, uint32_t& capacity, uint32_t& used) {
    if (c->ovl) {
        std::lock_guard<std::recursive_mutex> lk(c->lender->mu);
        capacity = c->lender->ovl_stride;
        used = c->n_tlas_own;
        return;
    }
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    capacity = tt_tlas::region_capacity(c->host.is_blas_node, c->tlas_cap);
    used = tt_tlas::used_nodes(c->host.nodes.data(), capacity);
}

// The mutation itself, after every check passed: the host state, then tt_install_tlas_kernel on the stream, as a
// TLAS-side write section (it waits for plain borrowers only, as tt_tlas_refit does). nodes / idx: host copies
// (the mirror's source); src_nodes / src_idx: what the kernel reads. staged: they are the current pinned slot.
tt_status install_tlas(tt_ctx* c, const tt_tlas::Plan& p, const tt_cwbvh_node* nodes, const int32_t* idx,
                       const tt_tlas::Check& k, const void* src_nodes, const void* src_idx, bool staged) {
    SceneWrite sw(c, false, !c->ovl);  // (an overlay's TLAS is read by nobody else)
    TT_HIP(c, sw.err);
    {
        std::lock_guard<std::recursive_mutex> lk(c->mu);  // node 0 (TT_ROOT_LEAF) is read by launches under it
        SceneHost& h = c->host;
        tt_tlas::apply_mirror(p, nodes, idx, k, c->ovl, h.nodes, h.tlas, h.is_tlas_node, h.tlas_nodes);
        if (c->ovl) c->n_tlas_own = p.n_nodes;
        // (the reach of the scene's own TLAS only grows: what tt_ctx_share_blas may copy, and what a node rewrite
        // treats as the TLAS region; 0 stays "no overlay regions")
        else if (c->tlas_res) c->tlas_res = std::max(c->tlas_res, p.n_nodes);
        c->root_known = true;  // node 0 is the host's again: the root-leaf step and the leaf kernel follow it
        c->refit_gen = ~0ull;  // the TLAS refit plan only (the per-mesh BLAS plans follow scene_gen, untouched)
    }
    uint32_t slot;
    TT_HIP(c, ring_open(c, c->timing, slot));
    hipLaunchKernelGGL(tt_install_tlas_kernel, dim3(p.blocks), dim3(tt_tlas::kInstallBlock), 0, c->stream,
                       static_cast<const uint4*>(src_nodes), static_cast<const int32_t*>(src_idx),
                       reinterpret_cast<uint4*>(c->scene.nodes.p + c->tlas_base),
                       TT_NODE_STRIDE != 80 ? c->scene.nodes_k.p + (size_t)c->tlas_base * TT_NODE_STRIDE : nullptr,
                       c->scene.tlas.p, c->scene.mesh.p, c->scene.leaf.p, p.copy_units, p.units, p.n_idx,
                       (uint32_t)c->host.mesh.size());
    TT_HIP(c, hipGetLastError());
    if (staged) TT_HIP(c, stage_end(c));  // (after the kernel: it reads the staging slot)
    TT_HIP(c, ring_close(c, c->timing, slot));
    TT_HIP(c, sw.end());
    return TT_OK;
}
}  // namespace

extern "C" {

tt_status tt_scene_update_tlas(tt_ctx* c, const tt_cwbvh_node* tlas_nodes, uint32_t n_tlas_nodes,
                               const int32_t* tlas_indices, uint32_t n_tlas_indices, uint32_t flags) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER_TLAS(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    if (flags & ~(uint32_t)TT_TRACE_ASYNC) return fail(c, TT_ERR_INVALID_ARG, "tt_scene_update_tlas: unknown flag");
    uint32_t capacity, used;
    tlas_region_of(c, capacity, used);
    // the counts first; then the arrays are staged and the staged copy is what gets checked, mirrored and
    // installed (the caller may reuse, or be racing on, its own arrays)
    tt_tlas::Check k;
    if (tt_tlas::check_counts(tlas_nodes, n_tlas_nodes, capacity, tlas_indices, n_tlas_indices,
                              (uint32_t)c->host.tlas.size(), k) != TT_OK)
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_update_tlas: %s", k.why.c_str());
    TT_HIP(c, hipSetDevice(c->device));
    const tt_tlas::Plan p = tt_tlas::plan_install(n_tlas_nodes, used, n_tlas_indices);
    void* pinned = nullptr;
    TT_HIP(c, stage_begin(c, nullptr, p.stage_bytes, pinned));
    tt_tlas::fill_stage(p, tlas_nodes, tlas_indices, pinned);
    const tt_cwbvh_node* nodes = static_cast<const tt_cwbvh_node*>(pinned);
    const int32_t* idx = reinterpret_cast<const int32_t*>(static_cast<const uint8_t*>(pinned) + p.idx_offset);
    if (tt_tlas::check_install(nodes, n_tlas_nodes, capacity, idx, n_tlas_indices, (uint32_t)c->host.tlas.size(),
                               (uint32_t)c->host.mesh.size(), k) != TT_OK)
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_update_tlas: %s", k.why.c_str());  // (the slot was not handed on)
    void* src = nullptr;
    TT_HIP(c, hipHostGetDevicePointer(&src, pinned, 0));
    const tt_status st = install_tlas(c, p, nodes, idx, k, src, static_cast<const uint8_t*>(src) + p.idx_offset, true);
    if (st != TT_OK) return st;
    if (!(flags & TT_TRACE_ASYNC)) TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_tlas_rebuild(tt_ctx* c, const float* mesh_aabbs, uint32_t n_mesh, uint32_t flags, uint32_t* n_tlas_nodes) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER_TLAS(c);
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    if (flags & ~(uint32_t)(TT_TRACE_DEVICE_PTRS | TT_TRACE_ASYNC))
        return fail(c, TT_ERR_INVALID_ARG, "tt_tlas_rebuild: unknown flag");
    if (!mesh_aabbs || !n_mesh) return fail(c, TT_ERR_INVALID_ARG, "tt_tlas_rebuild: null or empty boxes");
    if (n_mesh != c->host.mesh.size() || n_mesh != c->host.tlas.size() || n_mesh >= (1u << 29))
        return fail(c, TT_ERR_INVALID_ARG, "tt_tlas_rebuild: n_mesh %u must equal the scene's _MeshData (%zu) and "
                                           "TLASBVH8Indices (%zu) counts", n_mesh, c->host.mesh.size(), c->host.tlas.size());
    uint32_t capacity, used;
    tlas_region_of(c, capacity, used);
    TT_HIP(c, hipSetDevice(c->device));
    const float* d_boxes = mesh_aabbs;
    if (flags & TT_TRACE_DEVICE_PTRS) {
        if (!is_device_ptr(mesh_aabbs)) return fail(c, TT_ERR_INVALID_ARG, "TT_TRACE_DEVICE_PTRS set but boxes are not device memory");
    } else {
        TT_HIP(c, stage_in(c, c->st_boxes, mesh_aabbs, (size_t)6 * n_mesh, 0, d_boxes));
    }
    // ---- build: presort, BVH2 + BVH8 + Aggregate, the forest forms of one tree (they sort <= 16 boxes too)
    const uint32_t start[2] = {0u, n_mesh};
    DevBuf<int32_t> pre;
    TT_HIP(c, pre.alloc(3 * (size_t)n_mesh));
    uint32_t slot;
    tt_status s;
    TT_HIP(c, ring_open(c, c->timing, slot));
    if ((s = tt_build_presort_forest(c->stream, d_boxes, start, 1, nullptr, pre.p, nullptr)) != TT_OK)
        return fail(c, s, "tt_tlas_rebuild: %s", tt_build_error());
    TT_HIP(c, ring_close(c, c->timing, slot));
    tt_forest_dev F;
    TT_HIP(c, ring_open(c, c->timing, slot));
    if ((s = tt_build_blas_forest(c->stream, d_boxes, start, 1, pre.p, F, nullptr)) != TT_OK)
        return fail(c, s, "tt_tlas_rebuild: %s", tt_build_error());
    TT_HIP(c, ring_close(c, c->timing, slot));
    const uint32_t n_nodes = F.node_base[1];
    if (n_nodes == 0 || n_nodes > capacity || n_nodes > 2ull * n_mesh)
        return fail(c, TT_ERR_UNSUPPORTED, "tt_tlas_rebuild: the rebuilt TLAS has %u nodes, its region holds %u", n_nodes,
                    (uint32_t)std::min<uint64_t>(capacity, 2ull * n_mesh));
    // ---- the small arrays come back for the host-side checks, the mirror and the refit plan
    std::vector<tt_cwbvh_node> nodes(n_nodes);
    std::vector<int32_t> idx(n_mesh);
    TT_HIP(c, hipMemcpyAsync(nodes.data(), F.nodes.p, sizeof(tt_cwbvh_node) * n_nodes, hipMemcpyDeviceToHost, c->stream));
    TT_HIP(c, hipMemcpyAsync(idx.data(), F.cwbvh_indices.p, sizeof(int32_t) * n_mesh, hipMemcpyDeviceToHost, c->stream));
    TT_HIP(c, hipStreamSynchronize(c->stream));
    tt_tlas::Check k;
    if ((s = tt_tlas::check_install(nodes.data(), n_nodes, capacity, idx.data(), n_mesh, n_mesh, n_mesh, k)) != TT_OK)
        return fail(c, s, "tt_tlas_rebuild: the built TLAS failed validation: %s", k.why.c_str());
    // ---- install, sourcing the device arrays
    const tt_tlas::Plan p = tt_tlas::plan_install(n_nodes, used, n_mesh);
    if ((s = install_tlas(c, p, nodes.data(), idx.data(), k, F.nodes.p, F.cwbvh_indices.p, false)) != TT_OK) return s;
    TT_HIP(c, hipStreamSynchronize(c->stream));  // (the builder's arrays are freed on return)
    if (n_tlas_nodes) *n_tlas_nodes = n_nodes;
    return TT_OK;
}

tt_status tt_scene_read_tlas_indices(tt_ctx* c, uint32_t first, uint32_t count, int32_t* out) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (!c->has_scene) return fail(c, TT_ERR_NO_SCENE, "no scene uploaded");
    const size_t n = c->lender && !c->ovl ? c->lender->host.tlas.size() : c->host.tlas.size();
    if (!out || (uint64_t)first + count > n)
        return fail(c, TT_ERR_INVALID_ARG, "tt_scene_read_tlas_indices: range out of bounds");
    TT_HIP(c, hipSetDevice(c->device));
    SceneRead sr(c);
    TT_HIP(c, sr.err);
    TT_HIP(c, hipMemcpyAsync(out, c->scene.tlas.p + first, sizeof(int32_t) * count, hipMemcpyDeviceToHost, c->stream));
    sr.end();
    TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

tt_status tt_scene_bytes(const tt_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return TT_ERR_INVALID_ARG;
    *bytes = c->scene.nodes.n * sizeof(tt_cwbvh_node) + c->scene.nodes_k.n + c->scene.tris_raw.n * sizeof(tt_cuda_triangle) + c->scene.tris.n * sizeof(TriPos) +
             c->scene.tlas.n * 4 + c->scene.mesh_raw.n * sizeof(tt_mesh_data) + c->scene.mesh.n * sizeof(MeshGpu) + c->scene.mat_tag.n * 4 +
             c->scene.hmap.n * sizeof(uint16_t) + c->scene.terrains.n * sizeof(tt_terrain);
    return TT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ terrains (tt_terrain.hip)
namespace {

// tt_terrain_validate's check; why receives the first violation
tt_status check_terrains(const tt_terrain* t, uint32_t n, const uint16_t* hm, uint32_t w, uint32_t h, std::string& why) {
    char buf[160];
    if (n == 0) return TT_OK;
    if (!t) {
        why = "null terrain array";
        return TT_ERR_INVALID_ARG;
    }
    if (!hm || w == 0 || h == 0 || (uint64_t)w * h > 0x7fffffffull) {
        why = "empty or oversized heightmap atlas";
        return TT_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0; i < n; i++) {
        const float* f = reinterpret_cast<const float*>(t + i);
        static const char* names[14] = {"PositionOffset.x", "PositionOffset.y", "PositionOffset.z", "HeightScale",
                                        "TerrainDim.x", "TerrainDim.y", "AlphaMap.x", "AlphaMap.y", "AlphaMap.z",
                                        "AlphaMap.w", "HeightMap.x", "HeightMap.y", "HeightMap.z", "HeightMap.w"};
        for (int k = 0; k < 14; k++)
            if (!std::isfinite(f[k])) {
                std::snprintf(buf, sizeof(buf), "terrain %u: %s is not finite", i, names[k]);
                why = buf;
                return TT_ERR_INVALID_ARG;
            }
        for (int k = 0; k < 4; k++)
            if (!(t[i].HeightMap[k] >= 0.0f && t[i].HeightMap[k] <= 1.0f)) {
                std::snprintf(buf, sizeof(buf), "terrain %u: HeightMap rectangle component %d = %g lies outside [0, 1]", i,
                              k, (double)t[i].HeightMap[k]);
                why = buf;
                return TT_ERR_INVALID_ARG;
            }
    }
    return TT_OK;
}
}  // namespace

extern "C" {

tt_status tt_terrain_validate(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap_half, uint32_t width,
                              uint32_t height, char* why, uint32_t why_len) {
    std::string w;
    const tt_status st = check_terrains(terrains, n, heightmap_half, width, height, w);
    copy_why(w, why, why_len);
    return st;
}

tt_status tt_scene_upload_terrains(tt_ctx* c, const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap_half,
                                   uint32_t width, uint32_t height) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_REFUSE_BORROWER(c);
    TT_REFUSE_LENDER(c);
    std::string why;
    const tt_status vs = check_terrains(terrains, n, heightmap_half, width, height, why);
    if (vs != TT_OK) return fail(c, vs, "tt_scene_upload_terrains: %s", why.c_str());
    TT_HIP(c, hipSetDevice(c->device));
    TT_HIP(c, hipStreamSynchronize(c->stream));  // no launch still reads the previous set
    c->scene.terrains_host.clear();
    c->scene.terrains.release();
    c->scene.hmap.release();
    c->scene.hmap_w = c->scene.hmap_h = 0;
    if (n == 0) return TT_OK;
    TT_HIP(c, c->scene.terrains.alloc(n));
    TT_HIP(c, c->scene.hmap.alloc((size_t)width * height));
    TT_HIP(c, hipMemcpy(c->scene.terrains.p, terrains, sizeof(tt_terrain) * n, hipMemcpyHostToDevice));
    TT_HIP(c, hipMemcpy(c->scene.hmap.p, heightmap_half, sizeof(uint16_t) * (size_t)width * height, hipMemcpyHostToDevice));
    c->scene.hmap_w = width;
    c->scene.hmap_h = height;
    c->scene.terrains_host.assign(terrains, terrains + n);
    return TT_OK;
}

}  // extern "C"
