/*
 * truetrace_scene.h — host-side producer of the buffers the trace kernel consumes.
 *
 * TrueTrace builds its acceleration structures on the CPU in C# (AssetManager /
 * ParentObject / BVH2Builder / BVH8Builder / CommonFunctions.Aggregate). No .NET runtime
 * exists in this environment, so this C++ library restates that pipeline (the reference's
 * host is compiled code) to produce byte-layout-identical buffers for tests and benches:
 *
 *   tt_blas_build      ParentObject.BuildTotal + Construct   ParentObject.cs:973-1111, 679-742
 *                        BVH2Builder (BLAS ctor)              BVH2Builder.cs:39-164
 *                        BVH8Builder (collapse)               BVH8Builder.cs:30-365
 *                        CommonFunctions.Aggregate            CommonVars.cs:662-688
 *   tt_scene_assemble  AssetManager.AccumulateData/UpdateTLAS AssetManager.cs:986-1138, 1610-1766
 *                        ConstructNewTLAS                     AssetManager.cs:1317-1421
 *
 * Divergences that cannot be pinned here (documented in DESIGN.md): .NET's Array.Sort tie
 * order is restated from the reference-source introsort; Mono float evaluation is assumed
 * IEEE single without contraction. Traversal parity does not depend on either: the trace
 * library consumes whatever node/triangle bytes it is given.
 */
#ifndef TRUETRACE_SCENE_H
#define TRUETRACE_SCENE_H
#include "truetrace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tt_mesh_input (one ParentObject's merged object-space mesh) is declared in truetrace_hip.h. */

typedef struct tt_blas tt_blas;

typedef struct tt_blas_info {
    uint32_t n_nodes;         /* BVH.cwbvhnode_count                          */
    uint32_t n_tris;          /* AggTriangles.Length                          */
    uint32_t bvh2_depth;      /* deepest BVH2 leaf                            */
    float aabb_min[3];        /* aabb_untransformed (ConstructAABB :1143-1149) */
    float aabb_max[3];
    double build_seconds;
} tt_blas_info;

tt_status tt_blas_build(const tt_mesh_input* mesh, tt_blas** out);
/* The same build in three steps, so the BVH2 stage can run on the GPU (tt_bvh2_build_device in
 * truetrace_hip.h) with byte-identical results:
 *   tt_blas_prepare_aabbs   BuildTotal's triangle AABBs (n_indices / 3 x {BBMax[3], BBMin[3]}),
 *   tt_bvh2_presort         BVH2Builder's three centroid presorts (.NET Array.Sort), 3 x n indices,
 *   tt_blas_build_from_bvh2 Construct's BVH8 stage + Aggregate over a BVH2 as tt_bvh2_build writes it. */
tt_status tt_blas_prepare_aabbs(const tt_mesh_input* mesh, float* aabbs_maxmin);
tt_status tt_bvh2_presort(const float* aabbs_maxmin, uint32_t n, int32_t* presorted);
tt_status tt_blas_build_from_bvh2(const tt_mesh_input* mesh, const int32_t* final_indices, const float* node_aabbs,
                                  const int32_t* node_left, const uint32_t* node_count, uint32_t bvh2_depth,
                                  tt_blas** out);
/* ... or over finished CWBVH8 nodes + cwbvh_indices (tt_blas_build_device in truetrace_hip.h). */
tt_status tt_blas_build_from_cwbvh(const tt_mesh_input* mesh, const tt_cwbvh_node* nodes, uint32_t n_nodes,
                                   const int32_t* cwbvh_indices, uint32_t bvh2_depth, tt_blas** out);
/* The same with the triangle preparation done once: tt_blas_prepare keeps BuildTotal's AggTriangles
 * (and writes the AABBs the device builder consumes); tt_blas_build_from_cwbvh_prepared then only
 * permutes them into leaf order. The handle is consumed (freed) by the build call on success and
 * on failure; tt_blas_prep_free releases one that is not built. */
typedef struct tt_blas_prep tt_blas_prep;
tt_status tt_blas_prepare(const tt_mesh_input* mesh, float* aabbs_maxmin, tt_blas_prep** out);
tt_status tt_blas_build_from_cwbvh_prepared(tt_blas_prep* prep, const tt_cwbvh_node* nodes, uint32_t n_nodes,
                                            const int32_t* cwbvh_indices, uint32_t bvh2_depth, tt_blas** out);
void tt_blas_prep_free(tt_blas_prep* prep);
tt_status tt_blas_get_info(const tt_blas* b, tt_blas_info* info);
/* Copies the packed nodes (80 B) and the leaf-ordered triangles (88 B). */
tt_status tt_blas_copy(const tt_blas* b, tt_cwbvh_node* nodes, tt_cuda_triangle* tris);
/* CWBVHIndicesBufferInverted (ParentObject.cs:691-694): for each source triangle, its position in
 * the leaf-ordered triangle array — the map tt_blas_refit's Construct writes through. */
tt_status tt_blas_copy_leaf_order(const tt_blas* b, int32_t* leaf_of_triangle);
void tt_blas_free(tt_blas* b);

/* AssetManager aggregation. Order of meshes = RenderQue parents, then instances. */
typedef struct tt_parent_desc {
    const tt_blas* blas;
    float local_to_world[16];   /* transform.localToWorldMatrix (column-major)  */
    float world_to_local[16];   /* transform.worldToLocalMatrix (column-major)  */
    uint32_t material_count;    /* ParentObject.MatOffset                      */
} tt_parent_desc;

typedef struct tt_instance_desc {
    uint32_t instance_parent;   /* index into instance_parents[]                */
    float local_to_world[16];
    float world_to_local[16];
} tt_instance_desc;

typedef struct tt_scene_build tt_scene_build;

typedef struct tt_scene_build_info {
    uint32_t n_nodes;           /* AggNodeCount (TLAS region 2*(P+I) included) */
    uint32_t n_tris;
    uint32_t n_tlas_indices;    /* = number of meshes (P + I)                  */
    uint32_t n_mesh;
    uint32_t tlas_nodes;        /* TLASBVH8.cwbvhnode_count                    */
    uint32_t pad;
} tt_scene_build_info;

/* instance_parents are the InstanceData.RenderQue ParentObjects: their BLAS/triangles are
 * aggregated after the RenderQue parents but they get no MeshData of their own
 * (AssetManager.cs:1140-1185, 1704-1750). */
tt_status tt_scene_assemble(const tt_parent_desc* parents, uint32_t n_parents,
                            const tt_parent_desc* instance_parents, uint32_t n_instance_parents,
                            const tt_instance_desc* instances, uint32_t n_instances,
                            tt_scene_build** out);
/* The TLAS side alone, for a host that holds device-built objects (tt_object_build_device in truetrace_hip.h)
 * and no tt_blas: every parent and instance parent is described by what tt_object_build_info reports plus its
 * matrices and material count. The build holds the TLAS-region nodes only (2 * n_mesh of them, no BLAS nodes
 * and no triangles: tt_scene_build_copy copies that much), TLASBVH8Indices, _MeshData and the mesh AABBs, each
 * byte-identical to what tt_scene_assemble yields for the same BLASes; tt_scene_build_get_totals gives the
 * node and triangle counts of the whole layout (what tt_scene_build_info reports after tt_scene_assemble). */
typedef struct tt_object_desc {
    uint32_t n_nodes, n_tris;
    float aabb_min[3], aabb_max[3];   /* aabb_untransformed */
    float local_to_world[16];         /* instance parents: unused (their instances carry the matrices) */
    float world_to_local[16];
    uint32_t material_count;
} tt_object_desc;
tt_status tt_scene_assemble_tlas(const tt_object_desc* parents, uint32_t n_parents,
                                 const tt_object_desc* instance_parents, uint32_t n_instance_parents,
                                 const tt_instance_desc* instances, uint32_t n_instances,
                                 tt_scene_build** out);
tt_status tt_scene_build_get_totals(const tt_scene_build* s, uint32_t* n_nodes_total, uint32_t* n_tris_total);
tt_status tt_scene_build_get_info(const tt_scene_build* s, tt_scene_build_info* info);
tt_status tt_scene_build_copy(const tt_scene_build* s, tt_cwbvh_node* nodes,
                              tt_cuda_triangle* tris, int32_t* tlas_indices,
                              tt_mesh_data* meshdata);
/* The per-mesh world AABBs the TLAS was built over (AssetManager MeshAABBs, CreateAABB
 * :1239-1249), n_mesh x {BBMax[3], BBMin[3]} — the input tt_tlas_refit takes per frame. */
tt_status tt_scene_build_copy_mesh_aabbs(const tt_scene_build* s, float* out6);
void tt_scene_build_free(tt_scene_build* s);

/* The builder half of ConstructNewTLAS / CorrectRefit (AssetManager.cs:1350-1356, :1425-1430, :1412) over
 * caller-supplied world boxes: BVH2Builder's TLAS constructor, BVH8Builder and Aggregate over mesh_aabbs
 * (n_mesh x {BBMax[3], BBMin[3]}, indexed like _MeshData). It is the code tt_scene_assemble and
 * tt_scene_assemble_tlas run, so the same boxes give the same bytes. nodes has room for the TLAS region,
 * 2 * n_mesh nodes, and is written whole: *n_tlas_nodes nodes, then zeros. tlas_indices (n_mesh) receives
 * TLASBVH8Indices. Pure host code with no state: a host may run it on a worker thread, as the reference
 * does, and install the result with tt_scene_update_tlas (truetrace_hip.h). TT_ERR_UNSUPPORTED where the
 * reference's BVH8Builder fails. */
tt_status tt_tlas_build(const float* mesh_aabbs, uint32_t n_mesh, tt_cwbvh_node* nodes, uint32_t* n_tlas_nodes,
                        int32_t* tlas_indices);

/* Standalone pieces, exposed for unit tests. */
/* CommonFunctions.PackOctahedral (CommonVars.cs:816-833) */
uint32_t tt_pack_octahedral(float x, float y, float z);
/* BVH2 (BVH2Builder.cs): AABBs as {max xyz, min xyz} x n (the C# AABB field order).
 * Writes FinalIndices (n) and BVH2 nodes as {aabb(6 floats), left, count} (2n entries). */
tt_status tt_bvh2_build(const float* aabbs_maxmin, uint32_t n, int32_t* final_indices,
                        float* node_aabbs, int32_t* node_left, uint32_t* node_count);
/* .NET Framework IntrospectiveSort with a float-key Comparison (BVH2Builder.cs:137-147). */
void tt_dotnet_sort_by_key(int32_t* items, uint32_t n, const float* keys);

/* Terrains: scalar restatements of kernel_heightmap, kernel_shadow_heightmap's occlusion test and
 * GetHeightmapNormal (IntersectionKernels.compute:508-710, CommonData.cginc:922-938), the host reference of
 * tt_trace_heightmap / tt_trace_shadow_heightmap / tt_resolve_normals (host/tt_terrain.cpp; numerics as
 * pinned in truetrace_hip.h). heightmap: w * h binary16 texels. */
/* In place on rays (the bounce half p selects) and primary_info (nullable), as tt_trace_heightmap with host
 * pointers. stats (nullable): rays, hits, node_visits (samples), reps_exhausted (marches at the step bound). */
tt_status tt_terrain_trace_host(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap, uint32_t w,
                                uint32_t h, const tt_trace_params* p, tt_ray_data* rays, uint32_t* primary_info,
                                tt_stats* stats);
/* The same, plus one word per ray in detail (nullable): bit 0 the record was rewritten, bit 1 a bisection ran,
 * bit 2 a march ended at the step bound, bits 8-15 the terrains (index < 8) whose box test passed, bits
 * 16-23 the terrains (index < 8) that were hit. */
tt_status tt_terrain_trace_detail_host(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap, uint32_t w,
                                       uint32_t h, const tt_trace_params* p, tt_ray_data* rays,
                                       uint32_t* primary_info, tt_stats* stats, uint32_t* detail);
/* occluded_out[i] = 1 when a terrain occludes shadow ray i (rays with t == 0 are not marched: 0). stats
 * (nullable): rays (marched), hits (occluded), node_visits, reps_exhausted. */
tt_status tt_terrain_occluded_host(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap, uint32_t w,
                                   uint32_t h, const tt_shadow_ray* shadow_rays, uint32_t n_rays,
                                   uint8_t* occluded_out, tt_stats* stats);
/* GetHeightmapNormal(position, terrain_id). */
tt_status tt_terrain_normal_host(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap, uint32_t w,
                                 uint32_t h, const float* position3, uint32_t terrain_id, float* normal3);
/* The terrain rows of tt_enqueue_diffuse_bounce with TT_ENQUEUE_TERRAIN_BOUNCE, scalar: random(1, pixel), the
 * cosine sample with the pinned sincos, the octahedral round trip, GetTangentSpace and the terrain branch of
 * kernel_shade's diffuse subset (RayTracingShader.compute:52-84, 99-122). global_rays: the array the enqueue
 * reads (the bounce half p selects); frame_pixels as tt_ctx_set_frame_pixels (0: off). For ray i of the launch's
 * window survives[i] is -1 (not a terrain record: a miss or another mesh_id; out_rays[i] untouched), 0 (a
 * terrain record whose path ends: pdf <= 0, or triangle_id >= n) or 1 (it survives; out_rays[i] is its new
 * ray). out_rays and survives hold p->n_rays entries; nothing is compacted. */
tt_status tt_terrain_bounce_host(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap, uint32_t w,
                                 uint32_t h, const tt_trace_params* p, const tt_ray_data* global_rays,
                                 int32_t frames, int32_t max_bounce, uint32_t frame_pixels, tt_ray_data* out_rays,
                                 int32_t* survives);

/* ------------------------------------------------------------------ lights (host/tt_lights.cpp)
 * The host side of the light BVH: LightBVHBuilder.cs (both constructors), the light-triangle gather
 * (ParentObject.cs:1061-1075, :733-739) and the buffer layout of AssetManager.cs:998-1040, :1100-1204,
 * :1681-1707, restated. The reference sorts with System.Array.Sort (unstable) and ships no serialized light
 * trees, so tree topology is not pinned to it: these builders use a STABLE sort (ties keep index order) and are
 * deterministic. acos / asin / sin / cos run in double and round to float, as the C# does. */
/* LightBounds (CommonVars.cs:267-285): a box, a normal cone (axis w, half-angle acos(cosTheta_o)), the emission
 * falloff cosTheta_e, the power phi and the light count below. */
typedef struct tt_light_bounds {
    float BBMax[3];
    float BBMin[3];
    float w[3];
    float phi;
    float cosTheta_o;
    float cosTheta_e;
    int32_t LightCount;
    float Pad1;
} tt_light_bounds;

/* LightTriData of the triangles `targets` (n_targets indices < n) of a mesh's 88-byte records: pos0 / posedge1 /
 * posedge2 copied, TriTarget = the index. out_normals (n_targets x 3): normals when given, else the normalized
 * mean of the record's three decoded octahedral normals -- this library's stand-in for ParentObject.cs:1068,
 * which averages the source mesh's vertex normals before they are packed. */
tt_status tt_light_tris_from_mesh(const tt_cuda_triangle* tris, uint32_t n, const uint32_t* targets, uint32_t n_targets,
                                  const float* normals, tt_light_tri* out_tris, float* out_normals);
/* LightBVHBuilder(List<LightTriData>, List<Vector3>, phi) (LightBVHBuilder.cs:271-342): per triangle a box
 * (Validate 0.0001), the cone (-normal, cosTheta_o 1), phi 0.1, cosTheta_e = (float)cos(3.14159f / 2); the
 * presort by box centre per axis, partition_sah with EvaluateCost, the UnionCone rules, the packing of
 * :324-338. nodes holds 2 n records (node 1 is never referenced); root (nullable) receives ParentBound.
 * A split whose every cost is NaN (a zero box extent makes Kr infinite) falls back to the middle of axis 0;
 * the reference leaves split.index at -1 there. */
tt_status tt_light_bvh_build_mesh(const tt_light_tri* tris, const float* normals, uint32_t n, tt_light_node* nodes,
                                  tt_light_bounds* root);
/* LightBVHBuilder(LightBounds[]) (:345-409) over per-light-mesh bounds; leaves hold the bound's index. */
tt_status tt_light_bvh_build_tlas(const tt_light_bounds* bounds, uint32_t n, tt_light_node* nodes);
/* A mesh tree's root bound under the instance's localToWorld (column-major), AssetManager.cs:1686-1704: the box
 * about the transformed centre, the axis (Mat * w).normalized. The half extent is transformed with |Mat|, so
 * that the box encloses the transformed box under any rotation or mirroring; the reference applies Mat itself
 * (transform_direction), which is the same for the positive diagonal matrices it is exact for. */
tt_status tt_light_bounds_transform(const tt_light_bounds* root, const float* local_to_world, tt_light_bounds* out);

typedef struct tt_light_parent {  /* one mesh with emissive triangles: one light tree */
    const tt_light_tri* tris;
    const float* normals;         /* n_tris x 3 */
    uint32_t n_tris;
} tt_light_parent;
typedef struct tt_light_instance {  /* one light mesh: a parent's tree under a transform */
    uint32_t parent;
    int32_t mesh_index;             /* its _MeshData record (LockedMeshIndex) */
    float local_to_world[16];       /* column-major */
} tt_light_instance;
/* Lays LightNodes / LightTriangles / _LightMeshes out as the reference does: the TLAS over the instances in
 * nodes [0, 2 n_instances), each parent's tree behind it at an even offset, which becomes LightNodeOffset of
 * the _MeshData record of every instance of that parent (instances share their parent's tree and its rows of
 * LightTriangles); LightTriCount = the parent's triangle count. _LightMeshes row i = instance i:
 * StartIndex / IndexEnd its parent's rows, LockedMeshIndex, MatOffset = the record's MaterialOffset, Center the
 * centre of its world box. nodes_out holds 2 n_instances + 2 sum(n_tris) records, tris_out sum(n_tris),
 * meshes_out n_instances; *n_nodes / *n_tris receive the counts. meshdata is updated in place. */
tt_status tt_lights_assemble(const tt_light_parent* parents, uint32_t n_parents, const tt_light_instance* instances,
                             uint32_t n_instances, tt_mesh_data* meshdata, uint32_t n_mesh, tt_light_node* nodes_out,
                             uint32_t* n_nodes, tt_light_tri* tris_out, uint32_t* n_tris, tt_light_mesh* meshes_out);
/* The scalar host reference of tt_emit_nee (truetrace_hip.h): one ray at a time, float32, the same outputs bit
 * for bit. global_rays is the array the kernel reads (the bounce half p selects); frame_pixels as
 * tt_ctx_set_frame_pixels; terrains != 0: the scene has a terrain set (terrain records emit nothing).
 * p->flags: TT_NEE_NEGATIVE_T. samples / shadow_rays nullable. The lights are checked with the rules of
 * tt_lights_validate first (TT_ERR_INVALID_ARG). */
tt_status tt_emit_nee_host(const tt_light_node* nodes, uint32_t n_nodes, const tt_light_tri* ltris, uint32_t n_ltris,
                           const tt_light_mesh* lmeshes, uint32_t n_lmeshes, const tt_cuda_triangle* tris,
                           uint32_t n_tris, const tt_mesh_data* meshdata, uint32_t n_mesh, const tt_trace_params* p,
                           const tt_ray_data* global_rays, int32_t frames, int32_t max_bounce, uint32_t frame_pixels,
                           uint32_t terrains, tt_light_sample* samples, tt_shadow_ray* shadow_rays,
                           uint32_t* n_shadow);
/* The scalar host reference of tt_lights_refit (truetrace_hip.h): the same arguments over host arrays -- nodes and
 * ltris are rewritten in place, bit for bit what the device leaves. It evaluates the reference's dispatches in the
 * reference's order: per listed mesh the transfer, then its tree one depth level after another from the deepest
 * up; then, with transforms, the TLAS the same way. flags: TT_LIGHT_REFIT_CONSERVATIVE. The lights are checked
 * with the rules of tt_lights_validate first, the call with tt_lights_refit's; why (nullable) names the index. */
tt_status tt_lights_refit_host(tt_light_node* nodes, uint32_t n_nodes, tt_light_tri* ltris, uint32_t n_ltris,
                               const tt_light_mesh* lmeshes, uint32_t n_lmeshes, const tt_cuda_triangle* tris,
                               uint32_t n_tris, const tt_mesh_data* meshdata, uint32_t n_mesh,
                               const uint32_t* mesh_indices, uint32_t n_mesh_indices,
                               const tt_light_transform* transforms, uint32_t n_transforms, uint32_t flags, char* why,
                               uint32_t why_len);
/* The pinned asin / acos / sin / cos of the light refit (csrc/tt_light_refit_core.h) over an array, for tests:
 * fn 0 asin, 1 acos, 2 sin, 3 cos. */
tt_status tt_light_refit_math(uint32_t fn, const float* in, uint32_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif
