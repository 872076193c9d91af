/*
 * truetrace_hip.h — C ABI of the MI355X-native CWBVH8 closest-hit engine.
 *
 * This library replaces ONE dispatch of the TrueTrace path tracer:
 *
 *     cmd.DispatchCompute(IntersectionShader, TraceKernel, CurBounceInfoBuffer, 0)
 *         TrueTrace/Resources/RayTracingMaster.cs:964-970
 *     -> kernel_trace / IntersectBVH
 *         TrueTrace/Resources/MainCompute/IntersectionKernels.compute:60-260
 *
 * It consumes the exact buffers TrueTrace's AssetManager binds for that kernel
 * (AssetManager.SetMeshTraceBuffers, TrueTrace/Resources/AssetManager.cs:75-88):
 *
 *     cwbvh_nodes      80 B  BVHNode8Data            CommonData.cginc:174-181, CommonVars.cs:413-434
 *     AggTris          88 B  CudaTriangle            CommonData.cginc:63-77,   CommonVars.cs:436-456
 *     TLASBVH8Indices   4 B  int                     CommonData.cginc:160
 *     _MeshData        88 B  MyMeshDataCompacted     CommonData.cginc:162-172, CommonVars.cs:245-255
 *     _Materials      252 B  MaterialData            CommonData.cginc:215-258
 *
 * and the per-frame buffers RayTracingMaster binds (RayTracingMaster.cs:645-650):
 *
 *     GlobalRays           48 B RayData (hits written in place)   CommonData.cginc:100-107
 *     _PrimaryTriangleInfo 16 B uint4 per pixel                   IntersectionKernels.compute:11,229-238
 *     GlobalColors         64 B ColData (only Data.w is read)     CommonData.cginc:129-138
 *
 * Conventions: extern "C", cdecl, no exceptions cross the boundary, every call
 * returns tt_status. One host thread drives a context at a time (Unity issues
 * trace dispatches from its single render thread); one context per GPU.
 *
 * Numerics (pinned; the reference leaves them to DXC + the D3D driver):
 *   rcp(x) = IEEE 1.0f/x (correctly rounded); mad(a,b,c) = fmaf(a,b,c);
 *   dot(a,b) = fmaf(a.z,b.z, fmaf(a.y,b.y, a.x*b.x));
 *   cross(a,b).x = fmaf(a.y,b.z, -(a.z*b.y)) (cyclic);
 *   mul(M,v3).r = fmaf(m[r][2],v.z, fmaf(m[r][1],v.y, m[r][0]*v.x));
 *   mul(M,(o,1)).r = fmaf(m[r][2],o.z, fmaf(m[r][1],o.y, m[r][0]*o.x)) + m[r][3];
 *   min/max = IEEE minNum/maxNum (NaN-ignoring); no other contraction;
 *   fp32 denormals are preserved (no flush) on both the GPU and the oracle.
 */
#ifndef TRUETRACE_HIP_H
#define TRUETRACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#define TT_STATIC_ASSERT(c, m) static_assert(c, m)
#else
#define TT_STATIC_ASSERT(c, m) _Static_assert(c, m)
#endif

#define TT_ABI_VERSION 1

/* ---------------------------------------------------------------- status */
typedef int32_t tt_status;
enum {
    TT_OK = 0,
    TT_ERR_INVALID_ARG = 1,
    TT_ERR_OOM = 2,
    TT_ERR_HIP = 3,
    TT_ERR_UNSUPPORTED = 4,     /* e.g. a Cutout material reachable by the trace kernel */
    TT_ERR_STACK_OVERFLOW = 5,  /* a ray needed more than TT_STACK_SIZE stack entries   */
    TT_ERR_NO_DEVICE = 6,
    TT_ERR_NO_SCENE = 7
};

/* Traversal stack depth of the reference: uint2 stack[16]
 * (IntersectionKernels.compute:65). */
#define TT_STACK_SIZE 16
/* Hard loop bound of the reference: while (Reps < 1000)
 * (IntersectionKernels.compute:155). On exhaustion no hit is written. */
#define TT_MAX_REPS 1000

/* ------------------------------------------------------ buffer layouts */
/* BVHNode8Data, 80 B (CommonData.cginc:174-181). */
typedef struct tt_cwbvh_node {
    float p[3];          /* node_0xyz: quantization origin                        */
    uint32_t e_imask;    /* node_0w: e_x | e_y<<8 | e_z<<16 | imask<<24             */
    uint32_t base_child; /* node_1.x                                             */
    uint32_t base_tri;   /* node_1.y                                             */
    uint32_t meta[2];    /* node_1.zw: 8 meta bytes                              */
    uint32_t qlo_x[2], qhi_x[2]; /* node_2 */
    uint32_t qlo_y[2], qhi_y[2]; /* node_3 */
    uint32_t qlo_z[2], qhi_z[2]; /* node_4 */
} tt_cwbvh_node;
TT_STATIC_ASSERT(sizeof(tt_cwbvh_node) == 80, "BVHNode8Data is 80 bytes");

/* CudaTriangle, 88 B (CommonData.cginc:63-77, CommonVars.cs:436-456). */
typedef struct tt_cuda_triangle {
    float pos0[3];
    float posedge1[3];
    float posedge2[3];
    uint32_t norms[3];   /* octahedral 16:16 (CommonVars.cs:816-833)       */
    uint32_t tans[3];
    float tex0[2];
    float texedge1[2];   /* raw vertex UV, not an edge (ParentObject.cs:1039-1041) */
    float texedge2[2];
    uint32_t MatDat;
} tt_cuda_triangle;
TT_STATIC_ASSERT(sizeof(tt_cuda_triangle) == 88, "CudaTriangle is 88 bytes");

/* MyMeshDataCompacted, 88 B (CommonData.cginc:162-172, CommonVars.cs:245-255).
 * W2L is Unity's worldToLocalMatrix, column-major: element (row r, col c) at W2L[c*4+r]. */
typedef struct tt_mesh_data {
    float W2L[16];
    int32_t TriOffset;            /* C#: AggIndexCount */
    int32_t NodeOffset;           /* C#: AggNodeCount  */
    int32_t MaterialOffset;
    int32_t mesh_data_bvh_offsets;/* BLAS root (& 0x7fffffff) */
    int32_t LightTriCount;
    int32_t LightNodeOffset;
} tt_mesh_data;
TT_STATIC_ASSERT(sizeof(tt_mesh_data) == 88, "MyMeshDataCompacted is 88 bytes");

/* MaterialData, 252 B (CommonData.cginc:215-258). Only the fields the trace kernel
 * reads are named; the rest is opaque to this library. */
typedef struct tt_material {
    int32_t AlbedoTex[2];
    int32_t NormalTex[2];
    int32_t EmissiveTex[2];
    int32_t MetallicTex[2];
    int32_t RoughnessTex[2];
    int32_t AlphaTex[2];         /* @40  */
    int32_t MatCapMask[2];
    int32_t MatCapTex[2];
    float surfaceColor[3];       /* @64  */
    float emmissive;
    float EmissionColor[3];
    uint32_t Tag;                /* @92: flag bits, Invisible = bit 7 (GlobalDefines.cginc:46) */
    float roughness;
    int32_t MatType;             /* @100: CutoutIndex = 2 (GlobalDefines.cginc:24) */
    float transmittanceColor[3];
    float ior;
    float metallic, sheen, sheenTint, specularTint, clearcoat, clearcoatGloss;
    float anisotropic, flatness, diffTrans;
    float specTrans;             /* @156 */
    float Specular, scatterDistance;
    float AlbedoTexScale[4];     /* @168 */
    float MetallicRemap[2];
    float RoughnessRemap[2];
    float AlphaCutoff;           /* @200 */
    float NormalStrength, Hue, Saturation, Contrast, Brightness;
    float BlendColor[3];
    float BlendFactor;
    float SecondaryTexScale[2];
    float Rotation;              /* @248 */
} tt_material;
TT_STATIC_ASSERT(sizeof(tt_material) == 252, "MaterialData is 252 bytes");

#define TT_MAT_CUTOUT_INDEX 2   /* GlobalDefines.cginc:24 */
#define TT_FLAG_INVISIBLE   7   /* GlobalDefines.cginc:46 */

/* RayData, 48 B (CommonData.cginc:100-107). hits = (mesh_id, triangle_id, asuint(t),
 * (uint)(u*65535) | (uint)(v*65535)<<16) — set(), CommonData.cginc:430-434. */
typedef struct tt_ray_data {
    float origin[3];
    uint32_t PixelIndex;
    float direction[3];
    float last_pdf;
    uint32_t hits[4];
} tt_ray_data;
TT_STATIC_ASSERT(sizeof(tt_ray_data) == 48, "RayData is 48 bytes");

/* ColData, 64 B (CommonData.cginc:129-138); the trace kernel reads Data.w only. */
typedef struct tt_col_data {
    float throughput[3];
    float Direct[3];
    float Indirect[3];
    uint32_t PrimaryNEERay, Flags, MetRoughIsSpec;
    float Data[4];
} tt_col_data;
TT_STATIC_ASSERT(sizeof(tt_col_data) == 64, "ColData is 64 bytes");

/* ShadowRayData, 48 B (CommonData.cginc:116-123). t > 0 / t < 0 selects the Direct vs
 * PrimaryNEERay/Indirect accumulation in the reference; max distance = |t|; t is set to 0 in
 * place when the ray is occluded (IntersectionKernels.compute:449-454). */
typedef struct tt_shadow_ray {
    float origin[3];
    float LuminanceIncomming;
    float direction[3];
    float t;
    float illumination[3];
    uint32_t PixelIndex;
} tt_shadow_ray;
TT_STATIC_ASSERT(sizeof(tt_shadow_ray) == 48, "ShadowRayData is 48 bytes");

#define TT_FLAG_IS_BACKGROUND 5 /* GlobalDefines.cginc:41 */
#define TT_FLAG_SHADOW_CASTER 6 /* GlobalDefines.cginc:42 */

/* --------------------------------------------------------- context */
typedef struct tt_ctx tt_ctx;

typedef struct tt_config {
    int32_t device;        /* HIP device ordinal                                 */
    uint32_t flags;        /* reserved, 0                                        */
    uint64_t max_rays;     /* capacity of the staging ray buffer for host-pointer
                              traces (2*W*H for a wavefront ray buffer); 0 = none */
    void* stream;          /* hipStream_t to issue on; NULL = a library-owned BLOCKING
                              stream (it orders with the legacy NULL stream in both
                              directions, so a caller that writes device buffers on the
                              NULL stream, e.g. PyTorch's default stream, needs no extra
                              synchronisation before or after a call) */
} tt_config;

/* Create / destroy a per-GPU context. */
tt_status tt_ctx_create(const tt_config* cfg, tt_ctx** out);
tt_status tt_ctx_destroy(tt_ctx* ctx);
/* Last error message of this context (never NULL). */
const char* tt_last_error(const tt_ctx* ctx);
int32_t tt_abi_version(void);
/* Number of visible HIP devices (0 on a machine without a GPU). */
int32_t tt_device_count(void);

/* A non-blocking hipStream_t on a hardware queue of its own, for the concurrent launch streams of
 * one frame (parts / frame slots / the hit-record gather). Plain hipStreamCreate streams share a
 * process's few HW queues round-robin: two persistent trace grids whose streams land on one queue
 * run back to back instead of overlapping each other's drain (measured: a 2-part step then takes
 * the time of both launches, 0.45 vs 0.25 ms at an 8-GPU shard; profiles/r04/streams/). The stream is
 * made with hipExtStreamCreateWithCUMask and every CU enabled, which gives it a dedicated queue.
 * The reference has no equivalent (Unity issues one command buffer); a host that records its
 * dispatches on several queues (RayTracingMaster.cs:954-1007 per camera) would use one per queue.
 * The calling thread's current device is left unchanged. Destroy with tt_stream_destroy (it
 * synchronises the stream first). */
tt_status tt_stream_create(int32_t device, void** stream);
/* Synchronises and destroys a stream tt_stream_create made; TT_ERR_INVALID_ARG for any other handle
 * (or one destroyed already). Streams still alive when the process exits are synchronised and
 * destroyed by the library before the HIP runtime's own teardown (a CU-mask queue alive at that point
 * crashes the exit, SIGSEGV in __cxa_finalize): from the main thread's thread_local destructors (armed by
 * the first launch on such a stream, so they also run ahead of a profiler's per-thread state, e.g. under
 * rocprofv3) and, for launches made only from other threads, from an atexit handler (which runs the teardown on a
 * fresh thread: the exiting thread's per-thread profiler state is gone by then). A host that exits without
 * tt_stream_destroy -- or a Unity domain reload that skips it -- ends cleanly. A context whose stream the teardown
 * (or tt_shutdown) destroyed refuses launches with TT_ERR_INVALID_ARG and tt_ctx_destroy skips its stream sync, so
 * a host's static destructors may still destroy contexts after it. Note the main thread's teardown also runs when
 * the main thread ends with pthread_exit while other threads go on: their launches on library streams are then
 * refused -- such hosts destroy their streams themselves or call tt_shutdown. */
tt_status tt_stream_destroy(void* stream);
/* Streams made by tt_stream_create and not destroyed yet. */
uint32_t tt_stream_live_count(void);

/* ---------------------------------------------------------- scene */
/* Replaces AssetManager.SetMeshTraceBuffers (AssetManager.cs:75-88): copies the
 * aggregated buffers into HBM (the host keeps ownership of its arrays). Any previous
 * scene of the context is released. n_mat may be 0 (no material checks). */
tt_status tt_scene_upload(tt_ctx* ctx,
                          const tt_cwbvh_node* nodes, uint32_t n_nodes,
                          const tt_cuda_triangle* tris, uint32_t n_tris,
                          const int32_t* tlas_indices, uint32_t n_tlas_indices,
                          const tt_mesh_data* meshdata, uint32_t n_mesh,
                          const tt_material* materials, uint32_t n_mat);
/* The structural check tt_scene_upload runs (no GPU needed): every node, triangle, TLAS slot,
 * mesh record and (when any material is Invisible) material index reachable by IntersectBVH's
 * index arithmetic (IntersectionKernels.compute:157-213) is in range. why (nullable) receives
 * the first violation. Returns TT_OK, TT_ERR_INVALID_ARG or TT_ERR_UNSUPPORTED (Cutout). */
tt_status tt_scene_validate(const tt_cwbvh_node* nodes, uint32_t n_nodes,
                            const tt_cuda_triangle* tris, uint32_t n_tris,
                            const int32_t* tlas_indices, uint32_t n_tlas_indices,
                            const tt_mesh_data* meshdata, uint32_t n_mesh,
                            const tt_material* materials, uint32_t n_mat,
                            char* why, uint32_t why_len);
/* ------------------------------------------- GPU-resident objects, on-device scene assembly
 * The scene-change path. tt_scene_upload takes the whole aggregated scene from the host; the reference keeps
 * every ParentObject's node and triangle buffers on the GPU and, whenever the object set changes, lays the
 * aggregated arrays out and fills them there (AssetManager.AccumulateData, AssetManager.cs:986-1227, with
 * CombineNodeBuffers / CombineTriBuffers, GeneralMeshFunctions.compute:26-73). The calls below are that path:
 * an object is created once, and adding, removing or swapping objects costs one assembly -- host work in the
 * number of objects, TLAS nodes and mesh records, and one batched device-to-device gather.
 *
 * tt_object: one BLAS resident on a device -- its 80-byte nodes and 88-byte triangles with BLAS-local indices
 * exactly as tt_blas_copy (truetrace_scene.h) returns them, plus the traversal-layout triangle records derived
 * from them once by a kernel. It belongs to the device, not to the context that created it: any context on
 * that device may assemble it, any number of times and into several scenes, and it may be destroyed as soon
 * as an assembly has returned (the assembly copied it). */
typedef struct tt_object tt_object;

typedef struct tt_object_info {
    uint32_t n_nodes;
    uint32_t n_tris;
    int32_t device;
    uint32_t root;
    uint64_t bytes;     /* HBM the object occupies (nodes, triangles, derived triangle records) */
} tt_object_info;
TT_STATIC_ASSERT(sizeof(tt_object_info) == 24, "tt_object_info is 24 bytes");

/* The check tt_object_create runs (host only, no device needed): the BLAS-level walk of tt_scene_validate
 * from `root` with NodeOffset = TriOffset = 0, bounded by the object's OWN counts -- every reachable child
 * index < n_nodes, every reachable triangle index < n_tris, inner meta with child bits 1, no leaf meta
 * spilling into the internal-child bits. Stricter than the whole-scene check, where a BLAS may reach into its
 * neighbours: an object must stand alone. why (nullable) receives the first violation. */
tt_status tt_object_validate(const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris,
                             uint32_t n_tris, uint32_t root, char* why, uint32_t why_len);
/* Validates (TT_ERR_INVALID_ARG, reason in tt_last_error(ctx)), copies the host arrays to ctx's device and
 * derives the traversal records there. Synchronizes the context stream. */
tt_status tt_object_create(tt_ctx* ctx, const tt_cwbvh_node* nodes, uint32_t n_nodes, const tt_cuda_triangle* tris,
                           uint32_t n_tris, uint32_t root, tt_object** out);
tt_status tt_object_get_info(const tt_object* obj, tt_object_info* info);
tt_status tt_object_destroy(tt_object* obj);

/* One ParentObject's merged object-space mesh (ParentObject.LoadData output). */
typedef struct tt_mesh_input {
    const float* positions;   /* float3 per vertex, object space                          */
    uint32_t n_vertices;
    const float* normals;     /* float3 per vertex, nullable -> (0,1,0)                     */
    const float* tangents;    /* float4 per vertex, nullable -> (1,0,0,1)                   */
    const float* uvs;         /* float2 per vertex, nullable -> (0,0)                       */
    const int32_t* indices;   /* Unity index list, 3 per triangle                           */
    uint32_t n_indices;
    const int32_t* matdat;    /* per triangle MatDat (submesh material), nullable -> 0       */
    float lossy_scale[3];     /* transform.lossyScale: AABB padding 0.001/scale (:462-463)  */
} tt_mesh_input;

/* What a host needs to place a device-built object in a scene (tt_scene_assemble_tlas in truetrace_scene.h). */
typedef struct tt_object_build_info {
    uint32_t n_nodes, n_tris, bvh2_depth, max_matdat;
    float aabb_min[3], aabb_max[3];     /* aabb_untransformed, as tt_blas_info reports it */
    uint32_t presorted_on_host;         /* 1 when the caller's presort was used */
    uint32_t pad;
} tt_object_build_info;
TT_STATIC_ASSERT(sizeof(tt_object_build_info) == 48, "tt_object_build_info is 48 bytes");

/* A mesh built into a tt_object on ctx's device, with no 88-byte record ever in host memory: ParentObject.BuildTotal
 * (ParentObject.cs:973-1111) as two kernels around the device builder (csrc/tt_object_build.hip). Pass 1 derives
 * every triangle's {BBMax, BBMin} box (Create / Extend / Validate with 0.001 / lossy_scale) and checks every index
 * against n_vertices; the three presorts, the BVH2 and the BVH8 stage run as in tt_bvh2_presort_device and
 * tt_blas_build_device but on device-resident arrays; pass 2 writes the leaf-ordered 88-byte records, the traversal
 * records and leaf_of_triangle (CWBVHIndicesBufferInverted) straight from the vertices. Nodes, triangles and the
 * leaf order are byte for byte those of tt_blas_build (truetrace_scene.h) on the same mesh; the object is an
 * ordinary tt_object with root 0.
 *   flags: 0, or TT_TRACE_DEVICE_PTRS: every array the mesh names is in HBM on ctx's device (nullable arrays
 *          stay nullable).
 *   presorted: a HOST array of 3 x n indices (tt_bvh2_presort), or NULL: the presort runs on the device, which
 *          declines n <= 16, non-finite centroids and a depth-exhausted partition above 65536: TT_ERR_UNSUPPORTED,
 *          the reason in tt_last_error, nothing created; the caller retries with tt_blas_prepare_aabbs +
 *          tt_bvh2_presort.
 * A bad index, n_indices % 3 != 0 or null positions / indices: TT_ERR_INVALID_ARG before the builder runs. Any
 * failure frees everything and leaves *out NULL and the context usable. Synchronizes the context stream. With
 * tt_ctx_set_timing on, the call records five tt_timing_read entries: pass 1, presort, BVH2 + BVH8, pass 2, the
 * node mirror's copy. */
tt_status tt_object_build_device(tt_ctx* ctx, const tt_mesh_input* mesh, const int32_t* presorted, uint32_t flags,
                                 tt_object** out, tt_object_build_info* info);
/* n_meshes meshes built into n_meshes objects in one call. out[m] is, byte for byte, the object
 * tt_object_build_device(ctx, &meshes[m], ...) makes -- nodes, triangles, traversal records, leaf_of_triangle, both info
 * structs, the host node mirror -- and as independent: each is destroyed, assembled, read and refitted on its own. The
 * builder runs every level of every stage for all meshes together (csrc/tt_build.hip, the forest forms), so the host
 * waits once per level of the deepest mesh instead of once per level of every mesh; the two mesh passes are one launch
 * each over all triangles; host meshes travel in one copy, the node mirrors come back in one.
 *   presorted: nullable; presorted[m] a HOST list of 3 x n_m indices or NULL (mesh m is sorted on the device). Unlike
 *          the single call, the device sorts meshes of <= 16 triangles too. presorted_on_host is 1 exactly where a list
 *          was supplied. The device presort still declines non-finite centroids and a depth-exhausted partition above
 *          65536, per mesh: TT_ERR_UNSUPPORTED; the caller retries with host lists for those meshes.
 *   flags: 0 or TT_TRACE_DEVICE_PTRS, for all meshes. lossy_scale is per mesh.
 *   infos, mesh_status: nullable, n_meshes each.
 * All or nothing: any failure frees everything, sets every out[m] to NULL and leaves the context usable. Failures are
 * reported by the first stage that finds one, in the order argument checks, pass 1, presort, BVH2, BVH8, pass 2 / walk:
 * tt_last_error names the stage and the lowest failing mesh, mesh_status[m] holds TT_OK or the status that stage found
 * for mesh m (a BVH8 failure names the meshes found at the level the collapse stopped at). Argument checks, made
 * before any launch, TT_ERR_INVALID_ARG: n_meshes == 0, null positions or indices, n_indices not a positive multiple
 * of 3, a supplied presorted entry out of range, 2^29 triangles or more in the call, the single call's 4 GiB limits
 * per object. A bad index: TT_ERR_INVALID_ARG from pass 1. Synchronizes the context stream. With tt_ctx_set_timing on,
 * the call records the single call's five tt_timing_read entries, each once for the whole batch. */
tt_status tt_objects_build_device(tt_ctx* ctx, const tt_mesh_input* meshes, uint32_t n_meshes,
                                  const int32_t* const* presorted, uint32_t flags, tt_object** out,
                                  tt_object_build_info* infos, tt_status* mesh_status);
/* Copies an object's nodes (n_nodes x 80 B), triangles (n_tris x 88 B) and leaf order (n_tris) back to the host;
 * each pointer nullable. The leaf order exists on device-built objects only: TT_ERR_INVALID_ARG for it on an
 * object of tt_object_create (nodes and tris are still copied). Synchronizes the context stream. */
tt_status tt_object_read(tt_ctx* ctx, const tt_object* obj, tt_cwbvh_node* nodes, tt_cuda_triangle* tris,
                         int32_t* leaf_of_triangle);
/* The device array of leaf_of_triangle (n_tris), owned by the object: what tt_blas_refit takes with
 * TT_TRACE_DEVICE_PTRS. TT_ERR_INVALID_ARG for an object of tt_object_create. */
tt_status tt_object_leaf_order_device(const tt_object* obj, const int32_t** leaf_of_triangle_dev);

/* AccumulateData's running sums (AssetManager.cs:995, :1133-1136, :1178-1181), host arithmetic only:
 * node_offsets[0] = tlas_region (the reference's 2 * (parents + instances)), tri_offsets[0] = 0, each later
 * offset adds the previous object's counts; the totals are the scene's n_nodes and n_tris. A host writes
 * these values into its _MeshData records (NodeOffset, TriOffset, and the root = NodeOffset + the object's
 * root), as AssetManager.cs:1660-1679 does. Objects in RenderQue order: parents, then instance parents.
 * Output pointers are nullable. tt_scene_layout_counts is the same on plain counts (no handles). */
tt_status tt_scene_layout_objects(const tt_object* const* objects, uint32_t n, uint32_t tlas_region,
                                  uint32_t* node_offsets, uint32_t* tri_offsets, uint32_t* n_nodes_total,
                                  uint32_t* n_tris_total);
tt_status tt_scene_layout_counts(const uint32_t* n_nodes, const uint32_t* n_tris, uint32_t n, uint32_t tlas_region,
                                 uint32_t* node_offsets, uint32_t* tri_offsets, uint32_t* n_nodes_total,
                                 uint32_t* n_tris_total);

/* The device-side counterpart of tt_scene_upload. The caller supplies what changes per scene and is small --
 * the TLAS-region nodes [0, tlas_region), TLASBVH8Indices, _MeshData and the materials (host arrays) -- and
 * the objects, in layout order, supply everything else. Afterwards the context holds a scene whose device
 * arrays are byte for byte those tt_scene_upload would hold for the host-concatenated arrays, and every later
 * call (traces, tt_tlas_refit, tt_scene_update_*, tt_blas_refit, tt_ctx_share_*) behaves as after that upload.
 * Validation never touches a triangle: the TLAS-level walk over the supplied nodes, bounded by tlas_region;
 * every TLASBVH8Indices entry < n_mesh; every mesh record's (NodeOffset, TriOffset) equal to one object's pair
 * of the layout, and its root a node that object's own walk validated; the 4 GiB limits of tt_scene_upload.
 * Anything else is TT_ERR_INVALID_ARG with the reason in tt_last_error, before anything is launched. Objects
 * of another device: TT_ERR_INVALID_ARG. Refused like tt_scene_upload on a borrower and on a lender with
 * borrowers; a failed call leaves the context without a scene. The atlases and the terrain set survive.
 * The gather is one kernel over all objects on the context stream (csrc/tt_assemble.hip); the environment
 * variable TT_ASSEMBLE_FORM=memcpy (read at each call) selects three device-to-device copies per object
 * instead, kept for measurement, with identical bytes. The gather's GPU time is one tt_timing_read entry.
 * Synchronizes the context stream.
 * A deformed mesh: tt_blas_refit rewrites only the aggregated arrays (as the reference's RefitMesh does), so
 * a re-assembly reverts a deformed mesh to its object's triangles until the next tt_blas_refit. */
tt_status tt_scene_assemble_objects(tt_ctx* ctx, const tt_object* const* objects, uint32_t n_objects,
                                    const tt_cwbvh_node* tlas_nodes, uint32_t tlas_region,
                                    const int32_t* tlas_indices, uint32_t n_tlas_indices,
                                    const tt_mesh_data* meshdata, uint32_t n_mesh,
                                    const tt_material* materials, uint32_t n_mat);

/* Per-frame TLAS refit region rewrite (BVH8AggregatedBuffer.SetData at
 * AssetManager.cs:1760 / GPU refit AssetManager.cs:1821-1822). */
tt_status tt_scene_update_nodes(tt_ctx* ctx, uint32_t first, uint32_t count,
                                const tt_cwbvh_node* nodes);
/* Per-frame transform update (MeshDataBuffer.SetData, AssetManager.cs:1825). */
tt_status tt_scene_update_meshdata(tt_ctx* ctx, uint32_t first, uint32_t count,
                                   const tt_mesh_data* meshdata);
/* _AlphaAtlas (AssetManager.cs:260-262, :309): the R8 alpha atlas Cutout materials sample
 * (IntersectionKernels.compute:35-40 with my_linear_clamp_sampler; CommonData.cginc:616 with
 * my_point_clamp_sampler in the shadow path). texels: width*height bytes, row 0 = v in [0, 1/height)
 * (the sampling orientation, i.e. D3D texture rows). Copied to HBM; replaces any previous atlas.
 * Without an atlas, a scene with Cutout materials traces with TT_ERR_UNSUPPORTED.
 * Filtering is pinned (the reference leaves it to the texture unit): point = texel
 * clamp(floor(uv*size)); linear = taps at floor(uv*size - 0.5) and +1, clamped, weights
 * f = x - floor(x), lerp(a,b,f) = a*(1-f) + b*f in x then y, texel value = byte / 255.0f. */
tt_status tt_scene_upload_alpha_atlas(tt_ctx* ctx, const uint8_t* texels, uint32_t width, uint32_t height);
/* _TextureAtlas (AssetManager.cs:82, :275; declared Texture2D<half4>, CommonData.cginc:272): the
 * albedo atlas, BC6H in the reference, handed over DECODED as RGBA half texels (4 x uint16 IEEE
 * binary16 per texel, row-major, same row orientation as the alpha atlas). The any-hit kernel reads
 * it for the stained-glass shadow tint (triangle_intersect_shadow, CommonData.cginc:613-625 with
 * IgnoreGlassShadow + StainedGlassShadows, GlobalDefines.cginc:3,8): a glass surface (specTrans == 1)
 * never occludes; it multiplies the ray's throughput by surfaceColor * (texel.xyz + 2) / 3, texel =
 * point-clamp sample at AlignUV(BaseUv, AlbedoTexScale, AlbedoTex). Copied to HBM; replaces any
 * previous atlas. Without it, tt_trace_shadow on a scene with glass materials returns
 * TT_ERR_UNSUPPORTED. */
tt_status tt_scene_upload_texture_atlas(tt_ctx* ctx, const uint16_t* rgba_half, uint32_t width, uint32_t height);

/* TerrainDat / TerrainData, 60 B (CommonVars.cs:147-157, CommonData.cginc:280-287): one Unity terrain.
 * The terrain occupies the box PositionOffset + (0 .. TerrainDim.x, 0 .. TerrainDim.x, 0 .. TerrainDim.y);
 * its surface is y = PositionOffset.y + 0.01 + 2 * HeightScale * Heightmap(uv), uv = (x / TerrainDim.x,
 * z / TerrainDim.y) mapped into the atlas rectangle HeightMap: atlas_uv = uv * (HeightMap.xy - HeightMap.zw)
 * + HeightMap.zw (so .zw is the rectangle's corner at uv = 0 and .xy the corner at uv = 1). */
typedef struct tt_terrain {
    float PositionOffset[3];
    float HeightScale;
    float TerrainDim[2];
    float AlphaMap[4];   /* not read by the intersection stage */
    float HeightMap[4];
    int32_t MatOffset;   /* not read by the intersection stage */
} tt_terrain;
TT_STATIC_ASSERT(sizeof(tt_terrain) == 60, "TerrainData is 60 bytes");

/* mesh_id of a terrain hit record (IntersectionKernels.compute:686); its triangle_id is the terrain index. */
#define TT_TERRAIN_MESH_ID 9999999u
/* Hard bound of the heightmap ray march per terrain (IntersectionKernels.compute:535, :653). */
#define TT_TERRAIN_MAX_STEPS 2000

/* Terrains and the Heightmap atlas (AssetManager.cs:90-93; RHalf, :237): n TerrainData records and the atlas
 * as width*height IEEE binary16 texels, same row orientation as the alpha atlas. Copied to HBM; replaces
 * any previous set; n == 0 clears it (heightmap_half may then be NULL). The set belongs to the scene like
 * the atlases: contexts sharing the scene (tt_ctx_share_scene / _blas) see it, the call is refused while
 * borrowers exist, and a later tt_scene_upload keeps it. Every field must be finite and every HeightMap
 * rectangle must lie in [0, 1] (TT_ERR_INVALID_ARG, reason in tt_last_error). Filtering is pinned as the
 * alpha atlas's linear filter, applied to exactly decoded half texels. A group's members take their set
 * through tt_group_scene_upload_terrains (a member's slot contexts borrow its scene context's scene). */
tt_status tt_scene_upload_terrains(tt_ctx* ctx, const tt_terrain* terrains, uint32_t n,
                                   const uint16_t* heightmap_half, uint32_t width, uint32_t height);
/* The check tt_scene_upload_terrains runs (host only, no device needed). why (nullable) receives the first
 * violation. */
tt_status tt_terrain_validate(const tt_terrain* terrains, uint32_t n, const uint16_t* heightmap_half,
                              uint32_t width, uint32_t height, char* why, uint32_t why_len);

/* Per-frame TLAS refit on the GPU: AssetManager.RefitTLAS
 * (AssetManager.cs:1473-1548) with BVHRefitter.compute's RefitBVHLayer / NodeUpdate / NodeCompress
 * (:220-371). Re-quantizes p, e and the child boxes of the uploaded nodes [0, n_tlas_nodes) from
 * per-mesh world AABBs (mesh_aabbs: n_mesh x {BBMax[3], BBMin[3]}, the reference's AABB order,
 * indexed like _MeshData). The TLAS topology (meta, imask, base indices) is the uploaded one; its
 * NodePair / layer plan (ConstructNewTLAS, :1256-1390) is rebuilt on the host only when the scene
 * or its nodes change. Runs on the context stream: a later trace sees the refit TLAS. Numerics
 * pinned: e = 2^ceil(log2(extent * 0.003921569f)) exactly, float -> uint as D3D (NaN -> 0,
 * saturating). flags: TT_TRACE_DEVICE_PTRS (mesh_aabbs in HBM), TT_TRACE_ASYNC. */
tt_status tt_tlas_refit(tt_ctx* ctx, uint32_t n_tlas_nodes, const float* mesh_aabbs, uint32_t n_mesh,
                        uint32_t flags);

/* Per-frame BLAS refit of a deforming or skinned mesh (row f4), replacing ParentObject.RefitMesh
 * (ParentObject.cs:750-917): Construct (BVHRefitter.compute:72-120) re-derives each triangle of the
 * mesh from the current vertex buffer — positions and normals transformed by `transform`, AABB
 * padded by 1e-6 where flat, pos0 / posedge1 / posedge2 / packed normals written to AggTris at
 * TriOffset + leaf_of_triangle[t] — then NodeInitializer, RefitLayer (:177-212, deepest layer
 * first), NodeUpdate and NodeCompress re-quantize the mesh's CWBVH8 nodes in HBM (the plan of
 * ParentObject.Construct, :679-730, is built once per scene and cached per mesh).
 *   vertices: n_vertices x vertex_stride floats, position at +0 and normal at +3 (the raw
 *             GraphicsBuffer of SkinnedMeshRenderer.GetVertexBuffer / Mesh.GetVertexBuffer(0)),
 *   indices: 3 per triangle in Unity order (sharedMesh.triangles; submeshes concatenated, the
 *            triangle is (i0, i2, i1) as everywhere in TrueTrace),
 *   leaf_of_triangle: CWBVHIndicesBufferInverted (source triangle -> leaf-order position),
 *                     from tt_blas_copy_leaf_order.
 * Numerics pinned where the HLSL leaves them to DXC: mul as fmaf(m2, z, fmaf(m1, y, m0 * x)) (+ m3),
 * normalize(v) = v * (1 / sqrt(dot)), octahedral round = round-half-to-even. Out-of-range vertex
 * reads return zeros and out-of-range leaf writes are dropped (D3D semantics); host arrays are
 * also validated up front. The caller refits the TLAS afterwards (the mesh's bounds changed).
 * flags: TT_TRACE_DEVICE_PTRS (all three arrays in HBM), TT_TRACE_ASYNC. */
typedef struct tt_blas_refit_params {
    uint32_t mesh_index;     /* _MeshData record: its TriOffset, NodeOffset and BLAS root          */
    uint32_t n_tris;         /* triangles of the mesh (= its BLAS's triangle count)               */
    uint32_t n_vertices;
    uint32_t vertex_stride;  /* floats per vertex (Unity vertex buffer stride / 4), >= 6           */
    float transform[16];     /* "Transform", column-major (Unity Matrix4x4)                        */
    uint32_t flags;
} tt_blas_refit_params;
tt_status tt_blas_refit(tt_ctx* ctx, const tt_blas_refit_params* p, const float* vertices, const int32_t* indices,
                        const int32_t* leaf_of_triangle);

/* A frame's deforming meshes in one call: ParentObject.RefitMesh (ParentObject.cs:857-877) for any number of
 * meshes, each given as the renderers of its skinned group. The reference runs Construct once per renderer --
 * its own vertex buffer and Stride, its own Transform (worldToLocal * TRS(rootBone), :865), its own VertOffset
 * into CWBVHIndices (BVHRefitter.compute:88) -- and only then one refit pass over the BLAS. Here a renderer is a
 * tt_blas_refit_part, a mesh a tt_blas_refit_item, and the whole list costs two launches: one Construct over
 * every part of every item, one refit over every item's leaf NodePairs.
 *   Every triangle t of a part goes through Construct exactly as in tt_blas_refit (same pinned arithmetic, the
 * (i0, i2, i1) order, the 1e-6 padding) and lands at leaf_of_triangle[first_tri + t] of its item; an
 * out-of-range vertex read gives zeros, a leaf position outside [0, item.n_tris) drops the write. Then every
 * item's BLAS is refitted as tt_blas_refit does it. The device bytes afterwards (nodes, AggTris, traversal
 * records, the kernel-layout node copy) are those of the same refits made one mesh at a time; an item with one
 * part gives tt_blas_refit's bytes.
 *   The ranges [first_tri, first_tri + n_tris) of an item's parts must cover [0, item.n_tris) exactly once, in
 * any order (the reference constructs every renderer; a gap would keep boxes of an earlier frame).
 *   bounds_out (nullable, n_items x {BBMax[3], BBMin[3]}): each item's object-space root box as the refit's root
 * NodePair computed it. mesh_aabbs (nullable, the n_mesh x 6 array tt_tlas_refit takes): for every item with
 * local_to_world, slot mesh_index receives the box over the eight corners of that root box, each corner through
 * fmaf(m2, z, fmaf(m1, y, m0 * x)) + m3, max / min as maxNum / minNum; no other slot is touched (other records
 * instancing the same BLAS are the caller's). The thread that completes an item's root writes both: no further
 * launch, no read-back, so refit -> tt_tlas_refit -> trace chains on the stream with no host wait.
 *   flags: TT_TRACE_DEVICE_PTRS -- every vertices / indices / leaf_of_triangle array, bounds_out and mesh_aabbs
 * are device memory; the item, part and matrix descriptors are always host memory and are copied to pinned
 * staging before the call returns. TT_TRACE_ASYNC is honoured only with device pointers. Without
 * TT_TRACE_DEVICE_PTRS every array is staged, indices and leaf positions are range-checked on the host, and the
 * call synchronizes.
 *   Ordering and sharing are tt_blas_refit's (one BLAS-side mutation for the batch, refused on borrowers, one
 * tt_timing_read entry). The composed plan and its device arrays are cached for (scene, ordered list of
 * (mesh_index, n_tris, the record's NodeOffset)): a frame with the same list as the last allocates nothing and
 * does not synchronize.
 *   Refused with TT_ERR_INVALID_ARG (reason in tt_last_error) before anything is enqueued: n_items == 0, a null
 * array, an empty item or part, vertex_stride < 6, a mesh index out of range or given twice, two items whose
 * records share a NodeOffset (one BLAS: their arrival counters would race), parts that overlap or leave a gap,
 * TriOffset + n_tris beyond the scene, the device flag with a host pointer, more than TT_BLAS_REFIT_MANY_MAX_TRIS
 * triangles in all (leaf ranges are 24 * position + count in an int32); TT_ERR_UNSUPPORTED for a BLAS whose
 * root is not its first node. tt_blas_refit_items_validate is the host-only half of these checks (everything
 * that needs neither node data nor a device): `why` receives the first violation. */
#define TT_BLAS_REFIT_MANY_MAX_TRIS (1u << 26)
typedef struct tt_blas_refit_part {  /* one renderer of the group: one Construct dispatch of the reference */
    const float* vertices;           /* n_vertices x vertex_stride floats, position at +0, normal at +3   */
    uint32_t n_vertices;
    uint32_t vertex_stride;          /* floats per vertex, >= 6                                            */
    const int32_t* indices;          /* 3 per triangle, local to this part's vertex buffer                 */
    uint32_t n_tris;
    uint32_t first_tri;              /* VertOffset: triangle t is source triangle first_tri + t of the mesh */
    float transform[16];             /* column-major, as tt_blas_refit_params.transform                    */
} tt_blas_refit_part;
typedef struct tt_blas_refit_item {
    uint32_t mesh_index;             /* the _MeshData record                                               */
    uint32_t n_tris;                 /* its BLAS's triangle count                                          */
    const int32_t* leaf_of_triangle; /* n_tris, CWBVHIndicesBufferInverted                                 */
    const tt_blas_refit_part* parts;
    uint32_t n_parts;
    const float* local_to_world;     /* nullable, 16 floats column-major: see mesh_aabbs                   */
} tt_blas_refit_item;
tt_status tt_blas_refit_many(tt_ctx* ctx, const tt_blas_refit_item* items, uint32_t n_items, uint32_t flags,
                             float* bounds_out, float* mesh_aabbs);
tt_status tt_blas_refit_items_validate(const tt_blas_refit_item* items, uint32_t n_items, const tt_mesh_data* meshdata,
                                       uint32_t n_mesh, uint32_t n_scene_tris, uint32_t flags, char* why,
                                       uint32_t why_len);

/* BLAS builder, BVH2 stage, on the GPU (row f4's builder half): BVH2Builder (BVH2Builder.cs:9-217)
 * restated level by level -- segmented AABB.Extend scans, the full-sweep SAH with the reference's
 * tie rules, stable partitions -- with outputs identical to the sequential C# recursion and to
 * tt_bvh2_build (include/truetrace_scene.h), which takes the same arguments minus the presort.
 *   aabbs:      n x {BBMax[3], BBMin[3]} primitive boxes (host),
 *   presorted:  3 x n primitive indices, axis x, y, z, each sorted by centroid with .NET's
 *               Array.Sort (tt_bvh2_presort in truetrace_scene.h: the introsort's tie order decides
 *               trees, so the sort stays on the host),
 *   final_indices (n), node_aabbs (2n x 6), node_left (2n), node_count (2n): BVH2Nodes and
 *               FinalIndices as BVH2Builder leaves them; max_depth: BuildRecursive's deepest level.
 * Synchronous on the context stream. TT_ERR_UNSUPPORTED if some node has no finite SAH split. */
tt_status tt_bvh2_build_device(tt_ctx* ctx, const float* aabbs, uint32_t n, const int32_t* presorted,
                               int32_t* final_indices, float* node_aabbs, int32_t* node_left, uint32_t* node_count,
                               uint32_t* max_depth);

/* The whole BLAS build after the host's presort on the GPU (row f4's builder half): the BVH2 stage
 * above, then BVH8Builder (BVH8Builder.cs:30-392) -- the cost pass bottom up over the BVH2's levels,
 * get_children / order_children / collapse top down over the CWBVH8's levels with the sequential
 * depth-first node and triangle numbering recovered from per-subtree counts -- and Aggregate
 * (CommonVars.cs:662-688). Outputs are byte-identical to tt_blas_build's: the 80-B nodes (capacity
 * max_nodes >= n - 1 suffices), their count, cwbvh_indices (n: leaf position -> source triangle)
 * and the BVH2 depth; tt_blas_build_from_cwbvh (truetrace_scene.h) assembles the tt_blas.
 * TT_ERR_UNSUPPORTED where the reference's BVH8Builder.build fails. */
/* BVH2Builder's three centroid presorts (.NET Array.Sort: IntrospectiveSort with the float-key
 * Comparison, BVH2Builder.cs:137-147) on the GPU, with the same output as tt_bvh2_presort -- the
 * unstable sort's exact swap sequence replayed level by level (median of three, the two-pointer
 * partition in closed form, insertion sort <= 16, heapsort at the depth limit). TT_ERR_UNSUPPORTED
 * (use tt_bvh2_presort) for n <= 16, non-finite centroids, or a depth-exhausted partition above
 * 65536 elements. aabbs: n x {BBMax[3], BBMin[3]} (host); presorted: 3 x n (host). */
tt_status tt_bvh2_presort_device(tt_ctx* ctx, const float* aabbs, uint32_t n, int32_t* presorted);

tt_status tt_blas_build_device(tt_ctx* ctx, const float* aabbs, uint32_t n, const int32_t* presorted,
                               tt_cwbvh_node* nodes, uint32_t max_nodes, uint32_t* n_nodes, int32_t* cwbvh_indices,
                               uint32_t* bvh2_depth);

/* Copies AggTris [first, first+count) back from HBM (e.g. after tt_blas_refit). */
tt_status tt_scene_read_tris(tt_ctx* ctx, uint32_t first, uint32_t count, tt_cuda_triangle* out);

/* Copies nodes [first, first+count) of the scene in HBM back to the host (e.g. the TLAS after
 * tt_tlas_refit; the reference reads its refit TLAS back for nothing, but editors and tests do).
 * On a frame-slot context (tt_ctx_share_blas) nodes [0, n_tlas_nodes) are its own TLAS.
 * Synchronizes the context stream. */
tt_status tt_scene_read_nodes(tt_ctx* ctx, uint32_t first, uint32_t count, tt_cwbvh_node* out);
/* Copies TLASBVH8Indices [first, first+count) back from HBM (a frame slot: its own). Synchronizes the
 * context stream. */
tt_status tt_scene_read_tlas_indices(tt_ctx* ctx, uint32_t first, uint32_t count, int32_t* out);

/* TLAS rebuild, the other half of AssetManager.RefitTLAS (AssetManager.cs:1473-1530): its background task
 * CorrectRefit (:1423-1466) rebuilds the TLAS from the current MeshAABBs and every 25th frame the result is
 * swapped in (:1479-1529) -- new nodes (:1525), new TLASBVH8Indices (:1518), a new refit plan. A refit keeps
 * the upload-time topology, so a scene whose instances move far traces ever larger boxes; tt_scene_update_nodes
 * can rewrite the nodes but not TLASBVH8Indices or the leaf records derived from them, so a new topology
 * installed through it names the wrong meshes. These two calls replace, as ONE mutation on the context stream,
 * TLAS nodes [0, n_tlas_nodes), the whole TLASBVH8Indices and every derived leaf record; nodes
 * [n_tlas_nodes, previous count) are zeroed, so the device arrays are byte for byte what tt_scene_upload of the
 * host-composed arrays would hold. _MeshData, every BLAS, the triangles, materials, atlases and terrains are
 * untouched, nothing is reallocated, and the call is NOT refused on a lender with borrowers: like
 * tt_tlas_refit it is a TLAS-side update -- a plain borrower (tt_ctx_share_scene) sees the new TLAS, ordered
 * against its launches by the library; frame slots (tt_ctx_share_blas) neither see it nor wait; on a frame slot
 * it changes that slot's TLAS alone. Refused on a plain borrower. The number of mesh records cannot change:
 * n_tlas_indices must equal the scene's count.
 *   Capacity: the leading nodes of the scene that no validated BLAS walk reaches -- the tlas_region of an
 * assembled scene, 2 * n_mesh in the reference's layout (AssetManager.cs:995). Every frame slot's region behind
 * the lender's nodes has that size too, so a slot's rebuilt TLAS may have more nodes than the uploaded one.
 *   Validation (tt_scene_update_tlas: on the host, before anything is enqueued): the TLAS-level walk over the
 * supplied nodes, no child index leaving [0, n_tlas_nodes); every leaf slot < n_tlas_indices; leaf bits not
 * spilling into the internal-child bits; every index in [0, n_mesh); n_tlas_nodes <= capacity. Any failure is
 * TT_ERR_INVALID_ARG with the reason in tt_last_error, and the scene stays exactly as it was.
 *   Afterwards tt_tlas_refit takes the new n_tlas_nodes (its plan is rebuilt at the next call; the cached
 * per-mesh BLAS refit plans are kept), the host knows node 0 again (the root-leaf step and the leaf-TLAS
 * kernels follow it), and tt_ctx_share_blas accepts up to the largest TLAS installed so far.
 *
 * tt_scene_update_tlas installs a TLAS built on the host (tt_tlas_build in truetrace_scene.h, e.g. on a worker
 * thread as the reference does). The arrays are copied to pinned staging before the call returns -- the caller
 * may reuse them at once -- and one kernel reads them in place. flags: TT_TRACE_ASYNC (no stream sync; host
 * arrays are fine with it). One tt_timing_read entry when timing is on.
 *
 * tt_tlas_rebuild builds on the device from mesh_aabbs (n_mesh x {BBMax[3], BBMin[3]}, the array
 * tt_tlas_refit takes; n_mesh = the scene's count; flags: TT_TRACE_DEVICE_PTRS for boxes in HBM) -- the
 * presort, BVH2 and BVH8 stages of the device BLAS builder over the boxes -- reads the small node and index
 * arrays back for the checks above and the host mirror, and installs them with the same kernel, sourcing the
 * device arrays. The result is byte-identical to tt_tlas_build + tt_scene_update_tlas. Synchronizes the
 * context stream (the builder waits on the host once per tree level). With timing on: three tt_timing_read
 * entries -- presort, BVH2 + BVH8, install. n_tlas_nodes (nullable) receives the new count.
 * TT_ERR_UNSUPPORTED, reason in tt_last_error, scene unchanged -- fall back to tt_tlas_build +
 * tt_scene_update_tlas -- when the presort declines (non-finite centroids, a depth-exhausted partition above
 * 65536), where the reference's BVH8Builder fails, or when the result does not fit the region. */
tt_status tt_scene_update_tlas(tt_ctx* ctx, const tt_cwbvh_node* tlas_nodes, uint32_t n_tlas_nodes,
                               const int32_t* tlas_indices, uint32_t n_tlas_indices, uint32_t flags);
tt_status tt_tlas_rebuild(tt_ctx* ctx, const float* mesh_aabbs, uint32_t n_mesh, uint32_t flags,
                          uint32_t* n_tlas_nodes);

/* Makes `dst` trace `src`'s scene: no copy, the device buffers of src's last tt_scene_upload (and its
 * atlases) are read by dst's launches on dst's own stream. For several contexts tracing one scene
 * concurrently (e.g. a frame's tile-interleaved parts, one context and stream each): one cache
 * footprint instead of one per context. Scene updates (tt_scene_update_*, tt_tlas_refit,
 * tt_blas_refit) go through src and are seen by dst, ordered by the library in call order across
 * the two streams, with no host synchronization: a dst launch (trace, shadow, resolve, enqueue,
 * scene read) waits on the GPU for every src mutation called before it, and a src mutation waits
 * for every dst launch called before it (HIP events; the reference's per-frame "rewrite the TLAS
 * and _MeshData, then dispatch", AssetManager.cs:1821-1825, needs no caller-side ordering). While
 * borrowers exist, src refuses tt_scene_upload / the atlas uploads and
 * tt_ctx_destroy (destroy the borrowers first); dst refuses every scene-mutating call. Same device;
 * src must not itself borrow. Synchronizes both streams. */
tt_status tt_ctx_share_scene(tt_ctx* dst, tt_ctx* src);

/* Makes `dst` a frame slot over `src`'s scene: dst traces src's BLAS nodes, triangles, materials and
 * atlases (no copy, as tt_ctx_share_scene) but has a TLAS of its own -- a copy of the TLAS nodes
 * [0, n_tlas_nodes) (the refit's count, AssetManager.cs:995: the TLAS region at the front of the node
 * array), of TLASBVH8Indices and of _MeshData, taken from src's device buffers as they are now. The
 * reference refits the TLAS and rewrites every _MeshData record each frame before it traces
 * (AssetManager.cs:1767-1826); with one scene shared by frames in flight those writes would have to
 * wait for every in-flight frame's traces. On dst, tt_tlas_refit, tt_scene_update_meshdata and
 * tt_scene_update_nodes (its TLAS nodes only) change dst's TLAS alone and are ordered only on dst's
 * stream: no wait on src or on other slots, and neither src nor other slots see them. src's own
 * TLAS-side updates (tt_tlas_refit, tt_scene_update_meshdata, TLAS-only node rewrites) are not seen by
 * dst and do not wait for it; src's BLAS-side updates (tt_blas_refit) are seen by dst and ordered
 * against its launches as with tt_ctx_share_scene, and a BLAS-side node rewrite through
 * tt_scene_update_nodes is refused while frame slots exist (TT_ERR_UNSUPPORTED). The TLAS copy lives
 * in one of 8 regions src's upload reserved behind its nodes (8 x the TLAS region; TT_ERR_UNSUPPORTED
 * when all are in use). Precondition: every node the TLAS walk reaches lies in [0, n_tlas_nodes)
 * (TT_ERR_INVALID_ARG otherwise). dst refuses tt_blas_refit and uploads. Same device; src must not
 * itself borrow. Synchronizes both streams. */
tt_status tt_ctx_share_blas(tt_ctx* dst, tt_ctx* src, uint32_t n_tlas_nodes);

/* Bytes of HBM the scene occupies (device copies + derived traversal layouts). */
tt_status tt_scene_bytes(const tt_ctx* ctx, uint64_t* bytes);

/* ---------------------------------------------------------- trace */
enum {
    TT_TRACE_DEVICE_PTRS = 1u << 0,  /* ray/info/colors pointers are HIP device memory */
    TT_TRACE_USE_RESTIRGI = 1u << 1, /* uniform UseReSTIRGI (RayTracingMaster.cs:558)   */
    TT_TRACE_USE_ASVGF = 1u << 2,    /* uniform UseASVGF    (RayTracingMaster.cs:562)   */
    TT_TRACE_STATS = 1u << 3,        /* count node visits / tri tests into tt_stats     */
    TT_TRACE_ASYNC = 1u << 4,        /* device pointers only: return without syncing    */
    /* The reference's compile-time trace variants (GlobalDefines.cginc:4,11; both off there by
     * default), tested in IntersectTriangle after the Cutout alpha test:
     *   IgnoreGlassMain  (IntersectionKernels.compute:42-44): a candidate whose material has
     *                    specTrans == 1 is skipped;
     *   IgnoreBackfacing (:45-47): at bounce 0, a candidate whose material has specTrans != 1
     *                    (out-of-range materials read as zeros, so they count) is skipped when
     *                    dot(normalize(cross(normalize(posedge1), normalize(posedge2))), dir) <= 0,
     *                    dir = the ray in the space the triangle is tested in; normalize(v) pinned
     *                    as v * (1 / sqrt(dot(v, v))), cross / dot as in the numerics contract. */
    TT_TRACE_IGNORE_GLASS = 1u << 5,
    TT_TRACE_IGNORE_BACKFACING = 1u << 6,
    /* Adaptive dequeue order (tt_trace_closest only; ignored with TT_TRACE_STATS and by
     * tt_trace_closest_indirect). The launch records, per 64-ray chunk (the 8x8 pixel tile of a
     * full-frame batch, else 64 consecutive records), the largest Reps count of its rays, and the
     * next flagged launch with the same bounce index and screen size on this context dequeues its
     * chunks longest-first within each of the scheduler's segments, so long rays start early instead
     * of forming the launch's tail. Pays on scenes whose long rays are latency-bound chains (the
     * Bistro-shaped C4: -18% primary launch time with the previous, differently jittered frame's
     * costs); neutral to slightly negative on small, L2-resident scenes. Which lane traces which ray
     * changes, what is written does not: results are identical to an unflagged launch. The
     * reference pops rays in InterlockedAdd order (IntersectionKernels.compute:79-81), so no order
     * is part of its contract. */
    TT_TRACE_ADAPTIVE_ORDER = 1u << 7,
    /* tt_enqueue_diffuse_bounce(_indirect) only (every other call ignores it): on a context with terrains a
     * terrain hit bounces off the terrain instead of ending its path. Bit 8 of tt_shadow_params.flags is
     * TT_SHADOW_VISIBILITY_CHECK; the two never meet in one params struct. */
    TT_ENQUEUE_TERRAIN_BOUNCE = 1u << 8
};

typedef struct tt_trace_params {
    uint32_t n_rays;         /* BufferSizes[CurBounce].tracerays                     */
    int32_t bounce;          /* CurBounce; odd bounces read GlobalRays[W*H + i]      */
    float far_plane;         /* FarPlane (miss t)                                    */
    uint32_t screen_width;   /* screen_width  (ping-pong offset, pixel decode)       */
    uint32_t screen_height;  /* screen_height                                        */
    uint32_t flags;          /* TT_TRACE_*                                            */
} tt_trace_params;

typedef struct tt_stats {
    uint64_t rays;           /* rays traced                                           */
    uint64_t node_visits;    /* internal node tests (Reps increments)                  */
    uint64_t tri_tests;      /* IntersectTriangle calls                                */
    uint64_t blas_entries;   /* TLAS -> BLAS switches                                  */
    uint64_t hits;           /* rays whose final t < FarPlane                          */
    uint64_t reps_exhausted; /* rays that hit the Reps >= 1000 bound (no write)        */
    uint64_t stack_overflows;/* rays that would have pushed a 17th stack entry        */
    uint64_t accepts;        /* candidates that passed 0 < t < best.t                  */
    float kernel_ms;         /* trace kernel time (HIP events), sync traces only       */
    uint32_t pad;
} tt_stats;

/* kernel_trace replacement (IntersectionKernels.compute:60-260).
 *   global_rays    : RayData[2*W*H] (or at least bounce-half + n_rays); hits written
 *                    in place into GlobalRays[i].hits.
 *   primary_info   : nullable uint4[W*H] (_PrimaryTriangleInfo).
 *   global_colors  : ColData[W*H]; required when primary_info != NULL and bounce > 0.
 *   stats          : nullable; counters require TT_TRACE_STATS. */
tt_status tt_trace_closest(tt_ctx* ctx, const tt_trace_params* p, tt_ray_data* global_rays,
                           uint32_t* primary_info, const tt_col_data* global_colors,
                           tt_stats* stats);
/* tt_trace_closest that also writes each ray's 16-byte hit record contiguously: ray i of the launch
 * (GlobalRays[offset + i]) -> hits_out[4 i .. 4 i + 3], the same bytes as its RayData.hits. The hit
 * records of a tile-sharded frame are what the multi-GPU path gathers; written by
 * the trace itself they need no strided copy out of GlobalRays before the collective. Requires
 * TT_TRACE_DEVICE_PTRS; hits_out is 16-byte-aligned device memory of n_rays records. Everything
 * else (flags, stats, synchronization) is tt_trace_closest's. */
tt_status tt_trace_closest_hits(tt_ctx* ctx, const tt_trace_params* p, tt_ray_data* global_rays,
                                uint32_t* primary_info, const tt_col_data* global_colors, uint32_t* hits_out);
/* kernel_trace dispatched indirectly (the reference keeps BufferSizes[CurBounce].tracerays on the
 * GPU; TransferKernel turns it into DispatchIndirect arguments, RayTracingShader.compute:736-747,
 * RayTracingMaster.cs:964-970): the launch traces min(*n_rays_dev, p->n_rays) rays, the count read
 * on the device when the kernel starts, so a bounce chain (trace -> enqueue -> trace ...) runs on the
 * context stream with no host round trip. p->n_rays is the capacity (e.g. W*H); n_rays_dev is a
 * device uint32 written by an earlier operation on the stream (tt_enqueue_diffuse_bounce_indirect,
 * or the caller's own kernel / copy). Requires TT_TRACE_DEVICE_PTRS, implies TT_TRACE_ASYNC, and
 * rejects TT_TRACE_STATS. Results are identical to tt_trace_closest with the same count. */
tt_status tt_trace_closest_indirect(tt_ctx* ctx, const tt_trace_params* p, const uint32_t* n_rays_dev,
                                    tt_ray_data* global_rays, uint32_t* primary_info,
                                    const tt_col_data* global_colors);

/* The per-chunk costs the last TT_TRACE_ADAPTIVE_ORDER launch of bounce index `bounce` recorded on this
 * context (one uint32 per 64-ray chunk: the chunk's largest Reps count, 0 when every ray of the chunk
 * stayed below 32 node steps). A full-frame launch (n_rays == W*H, W and H multiples of 8) indexes
 * chunks by 8x8 pixel tile, (y / 8) * (W / 8) + x / 8; otherwise chunk i holds rays [64 i, 64 i + 64)
 * of the launch. Copies min(max, chunks) values and sets *n to that count (0 before any flagged
 * launch). Synchronizes the context stream. Hosts use it to balance screen tiles over GPUs by the
 * previous frame's cost (bench.py's strong-scaling deal). */
tt_status tt_trace_chunk_costs(tt_ctx* ctx, int32_t bounce, uint32_t* costs, uint32_t max, uint32_t* n);
/* Per-call GPU durations (HIP events on the context stream, in issue order) since the last
 * tt_timing_reset (ring of 256 entries). One entry per call of tt_trace_closest and
 * tt_trace_shadow (the trace kernel alone), tt_generate_primary (the generate kernel),
 * tt_enqueue_diffuse_bounce (counter reset + enqueue kernel), tt_tlas_refit, tt_blas_refit and
 * tt_blas_refit_many (the whole device-side refit; one entry for the whole list).
 * Host<->device staging copies are never inside an entry. Synchronizes. */
tt_status tt_timing_reset(tt_ctx* ctx);
tt_status tt_timing_read(tt_ctx* ctx, float* ms, uint32_t max, uint32_t* n);
/* Per-call timing on (default) or off. Off: asynchronous calls (TT_TRACE_ASYNC, device-resident counts)
 * record no HIP events and add no entry; synchronous trace calls still time their kernel (stats->kernel_ms).
 * Each timed call puts two stream-ordered event markers around its kernel, which costs little beside a
 * whole-frame launch but ~15-20% of a strong-scaled rank's small launches (profiles/r05/events/): a host
 * with several frames in flight keeps timing on for the one context it measures, if any. */
tt_status tt_ctx_set_timing(tt_ctx* ctx, int32_t enabled);
/* Several frames traced as one batch on a screen B times as tall (frame j's rays carry PixelIndex + j *
 * frame_pixels, so each frame keeps its own _PrimaryTriangleInfo / GlobalColors texels): with frame_pixels
 * = W * H of one frame, tt_enqueue_diffuse_bounce(_indirect) draws the bounce direction of a ray with
 * PixelIndex p from pixel p mod frame_pixels at frames + p / frame_pixels -- frame j's bounce rays are those
 * of the same pixels traced alone with frames_accumulated = frames + j (RayTracingShader.compute:52-84's
 * random(1, pixel) per frame). 0 (the default): PixelIndex as-is, the reference's form. */
tt_status tt_ctx_set_frame_pixels(tt_ctx* ctx, uint32_t frame_pixels);

/* SIMD-efficiency diagnostics of the last synchronous TT_TRACE_STATS launch: wave loop
 * iterations, iterations with node-phase work, node-phase lanes, iterations with triangle-phase
 * work, triangle-phase lanes, active lanes (sums over waves), node-phase lanes visiting the
 * same node as the wave's first node-phase lane, wave-uniform node phases. */
tt_status tt_trace_diagnostics(const tt_ctx* ctx, uint64_t* out8);

/* Which form of the closest-hit kernel the context's last trace launch (tt_trace_closest, _hits, _indirect)
 * took. The leaf-TLAS form serves scenes whose TLAS root is one leaf holding one instance (one imported
 * mesh): launches without TT_TRACE_STATS, the material check or TT_TRACE_ADAPTIVE_ORDER, while the host knows
 * node 0 (not after a device tt_tlas_refit until the next node update). Results are bit-identical in both
 * forms; the environment variable TT_LEAF_KERNEL=0 (read once per process) forces the generic form. */
enum {
    TT_TRACE_FORM_NONE = 0,    /* no trace launch yet */
    TT_TRACE_FORM_GENERIC = 1, /* the two-level kernel */
    TT_TRACE_FORM_LEAF = 2     /* the leaf-TLAS kernel */
};
tt_status tt_trace_last_form(const tt_ctx* ctx, uint32_t* form);
/* The selection predicate on its own (host only, no device needed): what node 0 of a TLAS is. */
enum {
    TT_ROOT_GENERIC = 0,     /* an internal child, or more than one child */
    TT_ROOT_ONE_LEAF = 1,    /* one child, a leaf of 2-3 instances: the generic kernel with its root shortcut */
    TT_ROOT_ONE_INSTANCE = 2 /* one child, a leaf of one instance: qualifies for the leaf-TLAS kernel */
};
tt_status tt_tlas_root_form(const tt_cwbvh_node* node0, uint32_t* form);

/* Self-test of the fast reciprocal the kernels use for rcp() (numerics contract: correctly
 * rounded 1.0f/x): evaluates it and the full IEEE division for all 2^32 fp32 bit patterns on the
 * context's device and returns the number of inputs whose results differ (bitwise, NaN == NaN) in
 * *mismatches; 0 is required. Synchronous, a few milliseconds. */
tt_status tt_selftest_rcp(tt_ctx* ctx, uint64_t* mismatches);

/* Wait for all work issued on the context's stream. */
tt_status tt_sync(tt_ctx* ctx);
/* Stack overflows (rays that would have pushed a 17th entry and were dropped) of every trace and
 * any-hit launch since the previous call, TT_TRACE_ASYNC launches included: synchronizes, writes
 * the count (nullable) and resets it. Returns TT_ERR_STACK_OVERFLOW when it is non-zero. */
tt_status tt_async_overflows(tt_ctx* ctx, uint64_t* count);
/* The hipStream_t the context issues on. */
void* tt_ctx_stream(tt_ctx* ctx);

/* --------------------------------------- any-hit visibility */
/* PropogatedCacheData, 48 B (CommonData.cginc:1621-1627, PropDepth 4 at :1493): the radiance-cache
 * record per pixel; the any-hit kernel updates CurrentIlluminance only. */
typedef struct tt_cache_data {
    uint32_t samples[4][2];
    uint32_t throughput;
    uint32_t pathLength;
    uint32_t CurrentIlluminance; /* @40: EncodeRGB log-luminance colour */
    uint32_t Norm;
} tt_cache_data;
TT_STATIC_ASSERT(sizeof(tt_cache_data) == 48, "PropogatedCacheData is 48 bytes");

/* tt_shadow_params.flags beyond TT_TRACE_DEVICE_PTRS / _STATS / _ASYNC / _USE_RESTIRGI: */
enum {
    /* the reference's RadianceCache define (GlobalDefines.cginc:15, on in its shipped define set):
     * selects the #ifdef RadianceCache accumulations of IntersectionKernels.compute:463-482 */
    TT_SHADOW_RADIANCE_CACHE = 1u << 7,
    /* VisabilityCheckCompute semantics (CommonData.cginc:710-819): the same any-hit traversal with
     * max distance = t as given (not |t|); visibility = (1,1,1,1) when no occluder is found -- the
     * Reps bound included -- else (0,0,0,0); nothing else is written */
    TT_SHADOW_VISIBILITY_CHECK = 1u << 8
};

typedef struct tt_shadow_params {
    uint32_t n_rays;         /* BufferSizes[CurBounce].shadow_rays                      */
    int32_t bounce;          /* CurBounce                                               */
    uint32_t screen_width;   /* NEEPosA pixel decode                                    */
    uint32_t screen_height;
    uint32_t flags;          /* TT_TRACE_DEVICE_PTRS | TT_TRACE_STATS | TT_TRACE_ASYNC  */
} tt_shadow_params;

/* Replaces one kernel_shadow dispatch (IntersectionKernels.compute:264-505, HardwareRT off,
 * AdvancedAlphaMapped / IgnoreGlassShadow / StainedGlassShadows on): any-hit CWBVH8 traversal of
 * shadow_rays[0, n_rays) against max distance |t|, skipping IsBackground / ShadowCaster
 * materials (triangle_intersect_shadow, CommonData.cginc:593-634). Outputs:
 *   shadow_rays    : t = 0 in place for occluded rays (as the reference);
 *   visibility     : nullable float4[n_rays] = (throughput.xyz, 1) for rays that reached |t|,
 *                    (0,0,0,0) occluded, (0,0,0,-1) Reps bound hit (the reference writes nothing);
 *   global_colors  : nullable ColData[W*H]; at bounce 0, for unoccluded rays with t >= 0,
 *                    Direct += illumination * throughput (:466-470);
 *   nee_pos        : nullable float4[W*H]; at bounce 0, unoccluded rays write
 *                    (origin + direction * |t|, 0) to NEEPosA[pixel] (:461).
 * tt_trace_shadow_ex (below) adds the radiance-cache, PrimaryNEERay and bounce > 0 Indirect
 * accumulations (RGBE / log-luminance encodings). Scenes with Cutout materials need the
 * alpha atlas and scenes with glass (specTrans == 1, stained-glass tint) the texture atlas;
 * without them the call returns TT_ERR_UNSUPPORTED. throughput = product of the glass tints of the
 * surfaces crossed, in traversal order (IEEE: t *= (c * (x + 2)) / 3 per component). */
tt_status tt_trace_shadow(tt_ctx* ctx, const tt_shadow_params* p, tt_shadow_ray* shadow_rays, float* visibility,
                          tt_col_data* global_colors, float* nee_pos, tt_stats* stats);
/* The full kernel_shadow output contract of a ray that reaches |t| (IntersectionKernels.compute:
 * 457-485, TerrainExists false), beyond tt_trace_shadow's Direct / NEEPosA, pixel = PixelIndex
 * (writes to pixels >= W*H are dropped):
 *   TT_SHADOW_RADIANCE_CACHE set (the reference's define set):
 *     cache_buffer[pixel].CurrentIlluminance = EncodeRGB(DecodeRGB(it) + illumination * throughput
 *         * ((!UseReSTIRGI || t >= 0) ? 1 : unpackRGBE(asuint(LuminanceIncomming))))  (cache nullable);
 *     t >= 0: bounce 0: Direct += illumination * throughput;
 *     t <  0: bounce != 0 && (UseReSTIRGI || Data.w == bounce):
 *                 Indirect += illumination * throughput * (UseReSTIRGI ? unpackRGBE(Lum..) : 1)
 *             else PrimaryNEERay = packRGBE(pow(unpackRGBE(PrimaryNEERay), 2.2f)
 *                                           + pow(illumination, rcp(2.2f)) * throughput);
 *   flag clear (#ifndef RadianceCache):
 *     t >= 0: bounce 0: Direct += illumination * throughput, else Indirect += the same;
 *     t <  0: bounce != 0 && !UseReSTIRGI && Data.w == -1: Indirect += illumination * throughput,
 *             else the PrimaryNEERay update above.
 * UseReSTIRGI = TT_TRACE_USE_RESTIRGI. The encoders and HLSL pow are pinned (driver-defined in the
 * reference): log2 / exp2 evaluated in double with a fixed series and rounded once to float, exact
 * floor(log2) / pow(2, n), round-half-to-even, D3D float -> uint; see csrc/tt_encode.h. One shadow
 * ray per pixel per launch (the reference's updates are not atomic either). */
tt_status tt_trace_shadow_ex(tt_ctx* ctx, const tt_shadow_params* p, tt_shadow_ray* shadow_rays, float* visibility,
                             tt_col_data* global_colors, float* nee_pos, tt_cache_data* cache_buffer,
                             tt_stats* stats);
/* tt_trace_shadow_ex dispatched indirectly (BufferSizes[CurBounce].shadow_rays on the GPU,
 * TransferKernel Type 1): traces min(*n_rays_dev, p->n_rays) shadow rays; as
 * tt_trace_closest_indirect (device pointers, asynchronous, no stats). */
tt_status tt_trace_shadow_ex_indirect(tt_ctx* ctx, const tt_shadow_params* p, const uint32_t* n_rays_dev,
                                      tt_shadow_ray* shadow_rays, float* visibility, tt_col_data* global_colors,
                                      float* nee_pos, tt_cache_data* cache_buffer);

/* ------------------------------------------------- terrains (heightmap ray march) */
/* Replaces one kernel_heightmap dispatch (IntersectionKernels.compute:602-710; RayTracingMaster.cs:973-977):
 * per-ray sphere tracing against the uploaded terrains, over the rays tt_trace_closest just traced (same
 * bounce half of GlobalRays, same flags: TT_TRACE_DEVICE_PTRS / _ASYNC / _USE_RESTIRGI / _STATS, same
 * host-staging rules). For each terrain in order: rayBoxIntersection (:513-521) against the box shrunk by
 * 0.001 with tMax = the record's t (floor 0.025); from max(t0 + 0.0001, 0) a march of at most
 * TT_TERRAIN_MAX_STEPS samples while CurDist < t and the position is strictly inside (0, dim.x) x (0, 1000) x
 * (0, dim.y); on dist < 0.0001 -- after the reference's two-stage bisection (:658-677) when the sample lies
 * below the surface -- the record becomes (TT_TERRAIN_MESH_ID, terrain index, CurDist + t0, uv packed as set()),
 * u, v = the last sample's unmapped uv, and the _PrimaryTriangleInfo texel (primary_info nullable) is written
 * at bounce 0 as (mesh_id, terrain, asuint(u), asuint(v)) and at bounce 1 as (UseReSTIRGI ? origin +
 * direction * t : direction, 1) (:687-691: no Data.w test, global_colors is not read); the next terrain then
 * sees the shortened t. Rays that miss keep their record and texel. Numerics: the header's contract, plus
 * g = sin(atan(1/2)) pinned as the fp32 nearest 1/sqrt(5), length(q) = sqrt(dot(q, q)) correctly rounded,
 * abs / max(0, q) / all(a < b) as plain IEEE comparisons (NaN compares false), SampleLevel = the pinned
 * linear filter on exactly decoded half texels. Results are bit-identical to tt_terrain_trace_host
 * (truetrace_scene.h). With TT_TRACE_STATS: rays, hits (rays whose record was rewritten), node_visits
 * (heightmap samples taken) and reps_exhausted (marches that ended at the step bound).
 * TT_ERR_NO_SCENE when no terrain set is uploaded. One launch per terrain, one thread per ray; the
 * environment variable TT_TERRAIN_FORM=persistent (read once per process) selects the persistent refill form
 * of the march kernels instead, which measured slower and gives identical results. */
tt_status tt_trace_heightmap(tt_ctx* ctx, const tt_trace_params* p, tt_ray_data* global_rays,
                             uint32_t* primary_info, tt_stats* stats);
/* tt_trace_heightmap that also writes every record it rewrites to the contiguous hit stream: whenever the march
 * rewrites ray i of the launch, the same 16 bytes go to hits_out[4 i .. 4 i + 3]; records of rays it does not
 * rewrite are not touched. hits_out is the buffer tt_trace_closest_hits just filled for the same rays, so after
 * both calls it equals RayData.hits of every ray (what a tile-sharded frame gathers). Requires
 * TT_TRACE_DEVICE_PTRS and 16-byte-aligned device memory of n_rays records; TT_TRACE_STATS is
 * TT_ERR_INVALID_ARG. Everything else is tt_trace_heightmap's. */
tt_status tt_trace_heightmap_hits(tt_ctx* ctx, const tt_trace_params* p, tt_ray_data* global_rays,
                                  uint32_t* primary_info, uint32_t* hits_out);
/* The same with a device-resident ray count: the contract of tt_trace_closest_indirect. */
tt_status tt_trace_heightmap_indirect(tt_ctx* ctx, const tt_trace_params* p, const uint32_t* n_rays_dev,
                                      tt_ray_data* global_rays, uint32_t* primary_info);
/* Replaces one kernel_shadow_heightmap dispatch (IntersectionKernels.compute:508-600; RayTracingMaster.cs:
 * 1000-1004). Only rays with t != 0 are marched (max distance |t|, the unshrunken box, from t0 + 0.001; the
 * loop tests the previous sample's position > 0, as the reference). An occluded ray writes nothing and keeps
 * its t. A ray no terrain occludes gets the outputs of :573-591, which use illumination without a throughput:
 *   bounce 0: NEEPosA[pixel] = (origin + direction * |t|, 0);
 *   TT_SHADOW_RADIANCE_CACHE: CurrentIlluminance = EncodeRGB(DecodeRGB(it) + illumination *
 *       ((!UseReSTIRGI || t >= 0) ? 1 : unpackRGBE(asuint(LuminanceIncomming))));
 *   t >= 0: bounce 0: Direct += illumination; else, without TT_SHADOW_RADIANCE_CACHE: Indirect += illumination;
 *   t <  0: bounce != 0 && UseReSTIRGI: Indirect += illumination;
 *           else PrimaryNEERay = packRGBE(pow(unpackRGBE(PrimaryNEERay), 2.2f) + pow(illumination, rcp(2.2f))).
 * visibility (nullable): (1,1,1,1) not occluded, (0,0,0,0) occluded; rays with t == 0 are left unwritten.
 * Flags as tt_trace_shadow_ex (TT_TRACE_STATS is accepted and reports nothing); TT_SHADOW_VISIBILITY_CHECK is
 * TT_ERR_INVALID_ARG. Every output pointer may be NULL. TT_ERR_NO_SCENE without a terrain set.
 * The reference's kernel_shadow with TerrainExists == true (:328, :459) only zeroes the t of occluded rays
 * and accumulates nothing; a host gets that form by calling tt_trace_shadow_ex with NULL global_colors,
 * nee_pos and cache_buffer and then this function on the same rays (tt_trace_shadow_ex itself is
 * unchanged). */
tt_status tt_trace_shadow_heightmap(tt_ctx* ctx, const tt_shadow_params* p, tt_shadow_ray* shadow_rays,
                                    float* visibility, tt_col_data* global_colors, float* nee_pos,
                                    tt_cache_data* cache_buffer);
tt_status tt_trace_shadow_heightmap_indirect(tt_ctx* ctx, const tt_shadow_params* p, const uint32_t* n_rays_dev,
                                             tt_shadow_ray* shadow_rays, float* visibility,
                                             tt_col_data* global_colors, float* nee_pos,
                                             tt_cache_data* cache_buffer);

/* ------------------------------------------------- attribute resolve */
/* Parity aid for "normals within 1e-5": per hit, the interpolated shading normal
 * (GetTriangleNormal, CommonData.cginc:904-911) with Inverse = transpose of W2L's
 * 3x3 (RayTracingShader.compute:99-118) and the geometric normal. Out: float[6] per
 * ray (shading xyz, geometric xyz); misses write zeros. On a context with terrains a hit with
 * mesh_id == TT_TERRAIN_MESH_ID and triangle_id < the terrain count writes GetHeightmapNormal
 * (CommonData.cginc:922-938) at origin + direction * t to both slots (RayTracingShader.compute:109-111);
 * without a terrain set such a record writes zeros, as ever. */
tt_status tt_resolve_normals(tt_ctx* ctx, const tt_trace_params* p,
                             const tt_ray_data* global_rays, float* normals6);

/* ------------------------------------------- ray producers */
/* Camera for Generate (RayGenKernels.compute:40-57) + CreateCameraRay (CommonData.cginc:511-567),
 * UseDoF off. Matrices are Unity's cameraToWorldMatrix and projectionMatrix.inverse,
 * column-major (m[c*4+r]). */
typedef struct tt_camera {
    float cam_to_world[16];
    float cam_inv_proj[16];
    float near_plane;
    float far_plane;
    uint32_t width;
    uint32_t height;
    int32_t jitter;             /* 1: random(0,pixel)-0.5 sub-pixel jitter (the !UseReCur path) */
    int32_t frames_accumulated; /* random() seed inputs (non-ASVGF branch)                      */
    int32_t max_bounce;
    uint32_t flags;             /* TT_TRACE_DEVICE_PTRS [| TT_TRACE_ASYNC]                      */
} tt_camera;

/* Writes W*H RayData (hits = (0,0,asuint(FarPlane),0)) into GlobalRays[pixel]. With device rays and
 * TT_TRACE_ASYNC the call returns without waiting (the camera is staged through pinned memory), so a
 * whole frame -- Generate, trace, enqueue, indirect trace -- is issued with no host synchronization. */
tt_status tt_generate_primary(tt_ctx* ctx, const tt_camera* cam, tt_ray_data* global_rays);

/* Diffuse-lobe next-bounce enqueue for the rays traced at p->bounce (the subset of kernel_shade
 * in RayTracingShader.compute:52-84, 99-122, 293, 498-506 that produces the next ray): hits
 * spawn a cosine-weighted ray about the shading normal, offset 1e-4 along the geometric normal;
 * misses terminate. Survivors are compacted into the other half of the ping-pong buffer in
 * source order (a stable single-pass scan: 4096-ray tiles, block ballot / LDS prefix, decoupled
 * look-back over the preceding tiles' counts; the reference's InterlockedAdd order,
 * RayTracingShader.compute:500, is whatever its atomics serialise to); *n_next receives their
 * count. On a context with terrains a hit with mesh_id == TT_TERRAIN_MESH_ID terminates its path, unless
 * p->flags has TT_ENQUEUE_TERRAIN_BOUNCE: then a terrain record with triangle_id < the terrain count survives
 * under the triangle rule (t < far_plane, pdf > 0 from the same random(1, pixel) draw) and its new ray is the
 * diffuse subset's terrain branch (RayTracingShader.compute:109-111): Geomnorm = USGNorm =
 * GetHeightmapNormal(origin + direction * t, triangle_id) (numerics as tt_resolve_normals), both negated when
 * dot(direction, USGNorm) > 0, then the triangle path's tail (octahedral round trip, tangent space, origin
 * USGNorm * 1e-4 + pos, last_pdf, hits copied); _MeshData and AggTris are not read for it. A terrain record
 * with triangle_id >= the terrain count is malformed input and ends its path (the guard of
 * tt_resolve_normals). Without a terrain set, or without the flag, nothing changes. */
tt_status tt_enqueue_diffuse_bounce(tt_ctx* ctx, const tt_trace_params* p, tt_ray_data* global_rays,
                                    int32_t frames_accumulated, int32_t max_bounce, uint32_t* n_next);
/* The same enqueue with device-resident counts: reads the traced count from n_rays_dev (nullable:
 * p->n_rays; otherwise p->n_rays is the capacity) and writes the survivor count to the device uint32
 * n_next_dev (BufferSizes[CurBounce + 1].tracerays) instead of returning it: no synchronization, so
 * it chains with tt_trace_closest_indirect. Requires TT_TRACE_DEVICE_PTRS. */
tt_status tt_enqueue_diffuse_bounce_indirect(tt_ctx* ctx, const tt_trace_params* p, const uint32_t* n_rays_dev,
                                             tt_ray_data* global_rays, int32_t frames_accumulated,
                                             int32_t max_bounce, uint32_t* n_next_dev);

/* --------------------------------- lights: the light BVH and next event estimation */
/* LightBVHData, 40 B (CommonData.cginc:987-994, CommonVars.cs:294-302). w: the cone axis, octahedral 16:16;
 * cosTheta_oe: floor(32767 (cosTheta_o + 1) / 2) in the low half, the same of cosTheta_e in the high half;
 * left >= 0: the even index of the first of two adjacent children (relative to the tree's first node);
 * left < 0: a leaf holding -(left + 1) (a _LightMeshes row in the TLAS part, else a light triangle relative
 * to the mesh's StartIndex). */
typedef struct tt_light_node {
    float BBMax[3];
    float BBMin[3];
    uint32_t w;
    float phi;
    uint32_t cosTheta_oe;
    int32_t left;
} tt_light_node;
TT_STATIC_ASSERT(sizeof(tt_light_node) == 40, "LightBVHData is 40 bytes");

/* LightTriData, 40 B (CommonData.cginc:297-302): the triangle in its mesh's space; TriTarget is its index
 * among the mesh's triangles (_MeshData.TriOffset is added on the device). */
typedef struct tt_light_tri {
    float pos0[3];
    float posedge1[3];
    float posedge2[3];
    uint32_t TriTarget;
} tt_light_tri;
TT_STATIC_ASSERT(sizeof(tt_light_tri) == 40, "LightTriData is 40 bytes");

/* LightMeshData, 28 B (CommonData.cginc:308-314): [StartIndex, IndexEnd) are the mesh's rows of
 * LightTriangles, LockedMeshIndex its _MeshData record. */
typedef struct tt_light_mesh {
    float Center[3];
    int32_t StartIndex;
    int32_t IndexEnd;
    int32_t MatOffset;
    int32_t LockedMeshIndex;
} tt_light_mesh;
TT_STATIC_ASSERT(sizeof(tt_light_mesh) == 28, "LightMeshData is 28 bytes");

/* Hard loop bound of SampleLightBVH: while (Reps < 322) (CommonData.cginc:1132). */
#define TT_LIGHT_MAX_REPS 322

/* What tt_emit_nee reports per traced ray, 48 B. A ray that missed, a terrain record and a ray beyond
 * far_plane get the "-1 record": light_tri = mesh_index = agg_tri = -1 and zeros. A hit whose descent ends
 * without a light (both importances zero) has light_tri = agg_tri = -1, the mesh_index reached so far
 * (-1 in the TLAS part), steps and weight as they stood, and zeros. */
typedef struct tt_light_sample {
    int32_t light_tri;   /* index into LightTriangles, or -1                                   */
    int32_t mesh_index;  /* the _MeshData index of the light's instance (LockedMeshIndex)      */
    int32_t agg_tri;     /* TriTarget + TriOffset                                              */
    int32_t steps;       /* Reps when SampleLightBVH returned                                  */
    float weight;        /* lightWeight after SampleLightBVH (from selectionoptions = 1)       */
    float area;          /* world area (RayTracingShader.compute:405-407)                      */
    float position[3];   /* world LightPosition (:408)                                         */
    float normal[3];     /* world LightNorm (:409)                                             */
} tt_light_sample;
TT_STATIC_ASSERT(sizeof(tt_light_sample) == 48, "tt_light_sample is 48 bytes");

/* tt_trace_params.flags of tt_emit_nee(_indirect), beyond TT_TRACE_DEVICE_PTRS / TT_TRACE_ASYNC: every
 * written t is negated (the PrimaryNEERay / Indirect form of kernel_shadow's accumulation). The reference
 * derives the sign from the radiance-cache path state (:465-474), which is the shading side. */
enum { TT_NEE_NEGATIVE_T = 1u << 9 };

/* The structural check tt_scene_upload_lights runs (host only, no device): everything SampleLightBVH's index
 * arithmetic (CommonData.cginc:1126-1166) and the caller (:1913-1920) can reach is in range, and the descent
 * ends. meshdata / n_mesh are the scene's _MeshData, n_scene_tris its triangle count. Refused, with the
 * offending index in why (nullable): an interior left that is odd, out of range or not greater than its
 * node's own index (children behind their parent: no cycle, so the descent is finite); a TLAS leaf whose
 * light mesh is >= n_meshes; a LockedMeshIndex outside _MeshData; a LightNodeOffset that is odd, below
 * 2 * n_meshes or past the nodes; a mesh-tree leaf outside [StartIndex, IndexEnd); a TriTarget outside its
 * mesh's triangles; a descent longer than TT_LIGHT_MAX_REPS steps. The TLAS part is nodes [0, 2 * n_meshes). */
tt_status tt_lights_validate(const tt_light_node* nodes, uint32_t n_nodes, const tt_light_tri* tris, uint32_t n_tris,
                             const tt_light_mesh* meshes, uint32_t n_meshes, const tt_mesh_data* meshdata,
                             uint32_t n_mesh, uint32_t n_scene_tris, char* why, uint32_t why_len);
/* LightNodes, LightTriangles and _LightMeshes of the context's scene (AssetManager.cs:1100-1204, :1705),
 * validated with tt_lights_validate against the scene's _MeshData. They belong to the scene: a
 * tt_ctx_share_scene borrower sees them, and tt_scene_upload / tt_scene_assemble_objects drop them.
 * TT_ERR_NO_SCENE without a scene; a borrower and a lender with borrowers refuse, as for tt_scene_upload. */
tt_status tt_scene_upload_lights(tt_ctx* ctx, const tt_light_node* nodes, uint32_t n_nodes, const tt_light_tri* tris,
                                 uint32_t n_tris, const tt_light_mesh* meshes, uint32_t n_meshes);
/* Rewrites LightNodes[first, first + count) (a host that moved a light mesh rebuilds the TLAS part,
 * AssetManager.cs:1681-1707); the whole set is validated again before anything is copied. Ordered against the
 * borrowers' launches like tt_scene_update_nodes. */
tt_status tt_scene_update_light_nodes(tt_ctx* ctx, uint32_t first, uint32_t count, const tt_light_node* nodes);

/* LightBVHTransform, 68 B (AssetManager.cs:1311-1314): a light mesh's current localToWorldMatrix and the root of
 * its mesh tree (its _MeshData record's LightNodeOffset). Transform is column-major like every other matrix
 * here: HLSL mat[r][c] is element (r, c) = Transform[c * 4 + r]. */
typedef struct tt_light_transform {
    float Transform[16];
    int32_t SolidOffset;
} tt_light_transform;
TT_STATIC_ASSERT(sizeof(tt_light_transform) == 68, "LightBVHTransform is 68 bytes");

/* tt_lights_refit flag, beyond TT_TRACE_DEVICE_PTRS / TT_TRACE_ASYNC: every cone contains the cones below it.
 * The default is the reference's drop-in arithmetic with its two kept exceptions: Rotate
 * returns m * transpose(m), so a union cone keeps its first child's axis and need not contain the second; a
 * TLAS leaf's axis goes through the matrix of absolute values. With the flag Rotate applies m itself and the
 * leaf axis is the matrix times the root's axis, normalized. */
enum { TT_LIGHT_REFIT_CONSERVATIVE = 1u << 10 };
/* The most light nodes tt_lights_refit addresses (40-byte nodes behind 32-bit byte offsets of a 2 GiB buffer
 * resource); tt_scene_upload_lights takes more, a refit of them is TT_ERR_UNSUPPORTED. */
#define TT_LIGHT_REFIT_MAX_NODES 53687091u

/* The per-frame refit of the light BVH on the device: LightBVHRefitter.compute's LightRefitKernel (:183-209, with
 * BVHRefitter.compute's TransferKernel :135-147 in front of it) for every listed mesh, then RefitKernel (:136-157)
 * over the light TLAS -- what the reference runs every frame from ParentObject.RefitMesh and
 * AssetManager.RefitTLAS. Two launches on the context stream, each a thread per leaf that climbs (no dispatch
 * per depth level), under one tt_timing_read entry.
 *   mesh_indices  host memory, may be empty: the _MeshData records whose light trees follow their triangles.
 *                 Call after tt_blas_refit(_many) of those meshes. Per light-triangle leaf: pos0 / posedge1 /
 *                 posedge2 of its LightTriangles row are copied from the 88-byte triangle at TriTarget +
 *                 TriOffset (TriTarget stays); the leaf's BBMax, BBMin, w and phi (the triangle's area) are
 *                 rewritten (cosTheta_oe and left stay); every interior node above is the Union of its children.
 *   transforms    nullable: NULL means no TLAS pass. Otherwise n_transforms must equal the light-mesh count;
 *                 TLAS leaf -(left + 1) = i takes transforms[i] and the node at its SolidOffset (after the mesh
 *                 pass, so it sees a refit root; instances that share a tree read the same root). With
 *                 TT_TRACE_DEVICE_PTRS the array is in HBM and an out-of-range SolidOffset reads zeros (D3D); a
 *                 SolidOffset there that names a TLAS node reads a node the same launch rewrites (order-dependent
 *                 bytes: the caller's error). A host array is checked instead: every SolidOffset must be the root
 *                 of a mesh tree, that is the LightNodeOffset of some light mesh's record.
 *   flags         TT_TRACE_DEVICE_PTRS, TT_TRACE_ASYNC (return without waiting; host arrays are copied to pinned
 *                 staging before the call returns, so either form may be asynchronous),
 *                 TT_LIGHT_REFIT_CONSERVATIVE.
 * Nodes no descent reaches (slot 1 of every tree, unused tail slots) keep their bytes. A moved light instance
 * also needs its _MeshData record rewritten (tt_scene_update_meshdata): the emit reads its W2L.
 * The host mirrors keep structure only after a refit: tt_scene_update_light_nodes still validates against them
 * (a refit never changes a `left`), but boxes, cones and powers are read back with tt_scene_read_light_nodes.
 * Results are bit-identical to tt_lights_refit_host (truetrace_scene.h) whatever the arrival order.
 * TT_ERR_INVALID_ARG, with the offending index in tt_last_error: a listed record with LightTriCount == 0 or
 * without a light tree, two listed records with one LightNodeOffset, n_transforms != the light-mesh count, a
 * host-side SolidOffset that is not a mesh tree's root; lights that tt_lights_validate accepts but no refit can
 * climb -- a node reached from two trees with distinct LightNodeOffset, or two light meshes naming one tree with
 * different StartIndex (the validator looks at each light mesh alone); a tt_ctx_share_scene borrower is refused (refit the lender: its
 * borrowers see it, ordered like tt_scene_update_light_nodes). TT_ERR_NO_SCENE without lights.
 * TT_ERR_UNSUPPORTED on a frame slot (tt_ctx_share_blas) or a group member, and
 * with more than TT_LIGHT_REFIT_MAX_NODES light nodes. */
tt_status tt_lights_refit(tt_ctx* ctx, const uint32_t* mesh_indices, uint32_t n_mesh_indices,
                          const tt_light_transform* transforms, uint32_t n_transforms, uint32_t flags);
/* LightNodes[first, first + count) / LightTriangles[first, first + count) as the device holds them, after
 * everything enqueued on the context stream (synchronizes). A borrower reads its lender's. */
tt_status tt_scene_read_light_nodes(tt_ctx* ctx, uint32_t first, uint32_t count, tt_light_node* out);
tt_status tt_scene_read_light_tris(tt_ctx* ctx, uint32_t first, uint32_t count, tt_light_tri* out);

/* Next event estimation toward the scene's emissive triangles for the rays traced at p->bounce: the geometric
 * subset of kernel_shade's NEE block (RayTracingShader.compute:328-344, :391-409, :418-479) for triangle
 * lights, as the enqueue is the subset that produces the next ray. Per hit (t < far_plane, a triangle record):
 *   pos, the shading normal norm (octahedral round trip), its flip and ray.origin = USGNorm * 1e-4 + pos are
 *     exactly tt_enqueue_diffuse_bounce's;
 *   SelectedLightGroup = 0 (LightMeshCount != 0, no unity lights, no sky), so RunningWeight starts at 1;
 *   the light is SampleLightBVH(pos, norm) (CommonData.cginc:1126-1166, Importance :1007-1043): a stochastic
 *     descent of the two-level light BVH with random(264 + Reps, pixel).x, bounded by TT_LIGHT_MAX_REPS;
 *   FinalUV = sample_triangle(random(79, pixel)) (:824-833), LightPosition, area and LightNorm in world space
 *     through inverse(W2L) of the light's instance (:401-409; AreaOfTriangle is Heron's formula);
 *   to_light, distance_to_light and SurfaceCos = dot(to_light, norm) (:419-426): a ray needs SurfaceCos > 0.
 * The BSDF is a diffuse stand-in, NOT the reference's Disney BSDF: bsdf_value = bsdf_pdf = SurfaceCos / pi, a ray
 * needs bsdf_pdf > 0.0001f; no Russian roulette (UseRussianRoulette off); NEE_pdf per :445; illumination =
 * (bsdf_value / NEE_pdf) * power_heuristic(NEE_pdf, bsdf_pdf) in all three channels (throughput 1, radiance 1).
 * Material emission and the emission atlas (CommonData.cginc:1921-1960) are not restated. The record written is
 * {ray.origin, asfloat(packRGBE(bsdf_value.xxx)), to_light, distance_to_light - 0.01f (negated with
 * TT_NEE_NEGATIVE_T), illumination, PixelIndex}. Survivors are compacted in source order with a stable scan
 * (tile ballot / LDS prefix / decoupled look-back, as the enqueue), so the output is deterministic byte for byte.
 * PixelIndex and tt_ctx_set_frame_pixels behave as in the enqueue. On a context with terrains a terrain record
 * emits nothing.
 *   samples      nullable: one tt_light_sample per traced ray (p->n_rays rows);
 *   shadow_rays  nullable: room for p->n_rays rows; rows past the survivor count are not touched;
 *   n_shadow     the survivor count. With TT_TRACE_ASYNC (device pointers) the call returns without waiting
 *                and n_shadow is not written (it may be NULL).
 * Numerics: the header's contract; pow(x, 2) and packRGBE are the pinned forms of the shadow kernel; inverse()
 * is the cofactor expansion by 3x3 minors, each a * (e i - f h) - b * (d i - f g) + c * (d h - e g), times
 * 1 / det. Results are bit-identical to tt_emit_nee_host (truetrace_scene.h).
 * TT_ERR_NO_SCENE without a scene or without lights; TT_ERR_UNSUPPORTED on a frame slot (tt_ctx_share_blas):
 * frame slots and groups do not carry lights. */
tt_status tt_emit_nee(tt_ctx* ctx, const tt_trace_params* p, const tt_ray_data* global_rays,
                      int32_t frames_accumulated, int32_t max_bounce, tt_light_sample* samples,
                      tt_shadow_ray* shadow_rays, uint32_t* n_shadow);
/* The same with device-resident counts: traces min(*n_rays_dev, p->n_rays) rays (n_rays_dev nullable:
 * p->n_rays) and writes the survivor count to the device uint32 n_shadow_dev (BufferSizes[CurBounce].shadow_rays),
 * without synchronizing, so it chains into tt_trace_shadow_ex_indirect. Requires TT_TRACE_DEVICE_PTRS. */
tt_status tt_emit_nee_indirect(tt_ctx* ctx, const tt_trace_params* p, const uint32_t* n_rays_dev,
                               const tt_ray_data* global_rays, int32_t frames_accumulated, int32_t max_bounce,
                               tt_light_sample* samples, tt_shadow_ray* shadow_rays, uint32_t* n_shadow_dev);

/* ------------------------------- multi-GPU tile-sharded frames */
/* The reference traces a frame with one dispatch per bounce on one GPU
 * (RayTracingMaster.cs:954-1007: Generate, then kernel_trace / kernel_shade per bounce). A group
 * traces a frame over several MI355X: the scene is replicated per device, the screen is cut into
 * tile x tile pixel tiles dealt round-robin (tile t to rank t % world), every member generates and
 * traces the primary rays of its tiles on its own device and streams, and the 16-B primary hit
 * records go to rank 0 with ONE RCCL gather (ncclSend / ncclRecv in a single group), where they are
 * scattered back to screen order: hits_out[pixel] holds exactly the RayData.hits tt_generate_primary
 * + tt_trace_closest write at GlobalRays[pixel]. Optionally each member then continues its own rays
 * (bounce 1: tt_enqueue_diffuse_bounce_indirect + tt_trace_closest_indirect on its stream) -- the
 * bounce chain never leaves the device. Members with a terrain set (tt_group_scene_upload_terrains) march it
 * after each triangle trace (tt_trace_heightmap_hits at bounce 0, before the info texels are packed and the
 * records gathered; tt_trace_heightmap_indirect at bounce 1) and bounce off terrain hits
 * (TT_ENQUEUE_TERRAIN_BOUNCE); without one a frame issues exactly the launches it issued before terrains.
 *
 * Two ways to form a group, one code path after that:
 *   tt_group_create       one process drives n devices (ncclCommInitAll): the C# / Unity host shape;
 *   tt_group_create_rank  one process per device (ncclCommInitRank over a tt_group_unique_id that
 *                         the host distributes), the shape of bench.py under torch.distributed.run.
 * RCCL is loaded at run time (dlopen "librccl.so.1": the copy a process already has, e.g. PyTorch's,
 * or the system ROCm one); TT_GROUP_COPY_GATHER gathers with device-to-device copies instead (one
 * process only; lets several members share one device, for tests on a one-GPU machine).
 * Frames are asynchronous when TT_TRACE_ASYNC is set: frame k uses slot k % slots (its own rays,
 * contexts and dedicated streams per member), so a member's next frame overlaps the previous one's
 * drain and gather; tt_group_sync waits for everything. */
typedef struct tt_group tt_group;

enum {
    TT_GROUP_COPY_GATHER = 1u << 0, /* gather with hipMemcpyAsync instead of RCCL (tt_group_create only)   */
    TT_GROUP_BOUNCE = 1u << 1,      /* each member traces bounce 1 of its primary hits (diffuse enqueue)  */
    TT_GROUP_INFO = 1u << 2         /* gather the bounce-0 _PrimaryTriangleInfo texels too (info_out)      */
};

typedef struct tt_group_config {
    uint32_t width, height; /* the screen (hits_out holds width * height records)                      */
    uint32_t tile;          /* tile edge in pixels, a multiple of 8 (0: 64)                               */
    uint32_t slots;         /* frames in flight per member (0: 2; at most 8)                              */
    uint32_t flags;         /* TT_GROUP_*                                                                 */
    uint32_t batch;         /* frames per call, B (0: 1; at most 16): a call traces frames_accumulated + b,
                               b < B, of one camera as ONE screen B frames tall (frame b's PixelIndex + b W H,
                               tt_ctx_set_frame_pixels): a launch's ramp-up and drain and every per-frame call
                               are paid once per B frames -- for progressive accumulation of a still view (the
                               next B samples' pose is known); B = 1 for a moving camera                  */
} tt_group_config;

/* One process, n devices (devices[i] is member i's HIP ordinal; member 0 is rank 0 and receives the
 * gather). Without TT_GROUP_COPY_GATHER the devices must be distinct. */
tt_status tt_group_create(const int32_t* devices, uint32_t n, const tt_group_config* cfg, tt_group** out);
/* The 128-byte RCCL unique id for tt_group_create_rank (rank 0 makes it; the host broadcasts it). */
tt_status tt_group_unique_id(uint8_t id[128]);
/* One member per process: this process is rank `rank` of `world` and drives HIP device `device`.
 * Every rank calls it concurrently (RCCL's init is collective). */
tt_status tt_group_create_rank(const uint8_t id[128], uint32_t world, uint32_t rank, int32_t device,
                               const tt_group_config* cfg, tt_group** out);
/* Synchronizes, tears the communicators, contexts and streams down. */
tt_status tt_group_destroy(tt_group* g);
const char* tt_group_last_error(const tt_group* g);
/* Members this process drives (n for tt_group_create, 1 for tt_group_create_rank). */
uint32_t tt_group_local_members(const tt_group* g);
/* Member m's scene context (slot 0's; the other slots share its scene, tt_ctx_share_scene): scene
 * updates (tt_scene_update_*, tt_tlas_refit, tt_blas_refit) go through it, and every slot sees them
 * in call order. NULL for m out of range. */
tt_ctx* tt_group_member_ctx(tt_group* g, uint32_t m);
/* tt_scene_upload on every local member (the scene replicated per device). */
tt_status tt_group_scene_upload(tt_group* g, const tt_cwbvh_node* nodes, uint32_t n_nodes,
                                const tt_cuda_triangle* tris, uint32_t n_tris,
                                const int32_t* tlas_indices, uint32_t n_tlas_indices,
                                const tt_mesh_data* meshdata, uint32_t n_mesh,
                                const tt_material* materials, uint32_t n_mat);
/* tt_scene_upload_alpha_atlas / tt_scene_upload_texture_atlas on every local member (after the scene upload:
 * a scene with Cutout materials needs the alpha atlas before it is traced). */
tt_status tt_group_scene_upload_alpha_atlas(tt_group* g, const uint8_t* texels, uint32_t width, uint32_t height);
tt_status tt_group_scene_upload_texture_atlas(tt_group* g, const uint16_t* rgba_half, uint32_t width, uint32_t height);
/* tt_scene_upload_terrains on every local member; n == 0 clears the set. With more than one slot a member's
 * scene context lends its scene and refuses the upload itself: this call lets the borrowers go and share again. */
tt_status tt_group_scene_upload_terrains(tt_group* g, const tt_terrain* terrains, uint32_t n,
                                         const uint16_t* heightmap_half, uint32_t width, uint32_t height);
/* Per-frame scene updates on every local member, between frames (AssetManager.cs:1760-1825 on each device):
 * tt_scene_update_meshdata / tt_scene_update_nodes / tt_tlas_refit of each member's scene context. The frame slots
 * borrow that scene, and the library orders each update after the traces already issued and before later ones, so
 * no synchronisation is needed. tt_group_tlas_refit takes host AABBs (flags: TT_TRACE_ASYNC). */
tt_status tt_group_scene_update_meshdata(tt_group* g, uint32_t first, uint32_t count, const tt_mesh_data* meshdata);
tt_status tt_group_scene_update_nodes(tt_group* g, uint32_t first, uint32_t count, const tt_cwbvh_node* nodes);
tt_status tt_group_tlas_refit(tt_group* g, uint32_t n_tlas_nodes, const float* mesh_aabbs, uint32_t n_mesh,
                              uint32_t flags);
/* tt_tlas_rebuild / tt_scene_update_tlas of each local member's scene context, between frames like the calls
 * above. Host arrays only (one device array cannot serve every member's device). The members build the same
 * boxes with the same code, so they end with the same TLAS; n_tlas_nodes (nullable) receives its node count.
 * tt_group_scene_update_tlas flags: TT_TRACE_ASYNC. */
tt_status tt_group_tlas_rebuild(tt_group* g, const float* mesh_aabbs, uint32_t n_mesh, uint32_t flags,
                                uint32_t* n_tlas_nodes);
tt_status tt_group_scene_update_tlas(tt_group* g, const tt_cwbvh_node* tlas_nodes, uint32_t n_tlas_nodes,
                                     const int32_t* tlas_indices, uint32_t n_tlas_indices, uint32_t flags);
/* One frame: Generate (cam: width / height must be the group's; TT_TRACE_DEVICE_PTRS implied) on every
 * member for its tiles, the primary trace, the gather to rank 0 and, with TT_GROUP_BOUNCE, bounce 1 on
 * every member. hits_out: on the process holding rank 0, a 16-byte-aligned buffer of batch * width * height uint4
 * records (frame b's screen-order records at [b W H, (b + 1) W H)) -- device memory of rank 0's device, or host
 * memory (then the frame must be
 * synchronous: the records are staged on rank 0's device and copied back); ignored (may be NULL) elsewhere.
 * info_out (TT_GROUP_INFO; else ignored): batch * width * height uint4 _PrimaryTriangleInfo texels, as hits_out, the
 * bounce-0 form tt_trace_closest writes (IntersectionKernels.compute:229-238), same kind of memory as hits_out;
 * each member packs its texels behind its hit records, so they travel in the same RCCL group.
 * flags: TT_TRACE_ASYNC (return without waiting; device hits_out only). */
tt_status tt_group_trace_frame(tt_group* g, const tt_camera* cam, uint32_t* hits_out, uint32_t* info_out,
                               uint32_t flags);
/* Waits for every frame issued so far (all members, all slots, the gathers). */
tt_status tt_group_sync(tt_group* g);
/* Of the latest call, member m: its primary ray count (batch x its pixels), its bounce-1 ray count (0 without
 * TT_GROUP_BOUNCE) and the device pointer of its ray buffer (RayData[batch * width * height + primary]: primary
 * rays at [0, primary) -- frame b's at [b n, (b + 1) n) --, bounce-1 rays at [batch * width * height, + bounce),
 * each frame's survivors after the previous frame's). Synchronizes. Any output may be NULL. */
tt_status tt_group_frame_rays(tt_group* g, uint32_t m, uint32_t* n_primary, uint32_t* n_bounce,
                              tt_ray_data** rays_dev);
/* The shard arithmetic (host only, no GPU): the pixels rank `rank` of `world` traces, in trace order --
 * its tiles t = rank, rank + world, ... (row-major tile ids over ceil(W / tile) x ceil(H / tile)), inside a
 * tile 8 x 8 pixel blocks in row-major block order, pixels row-major inside a block (so the 64 rays a
 * wave dequeues together are one 8 x 8 screen patch). world == 1 is the identity (pixel i = ray i, the
 * full-frame order the trace kernel swizzles itself). Writes min(count, max) indices, sets *n to count. */
tt_status tt_group_tile_pixels(uint32_t width, uint32_t height, uint32_t tile, uint32_t world, uint32_t rank,
                               uint32_t* pixels, uint32_t max, uint32_t* n);

/* ------------------------------------------------------------- shutdown */
/* Synchronizes and destroys every stream tt_stream_create made that is still alive. For hosts that
 * trace from a thread other than the main one (Unity's render thread): call it before the process or
 * the domain goes down (OnApplicationQuit / AppDomain.DomainUnload), after the last launch. Contexts
 * still alive keep their own streams; a context on a destroyed library stream refuses further launches
 * (TT_ERR_INVALID_ARG). Idempotent. */
tt_status tt_shutdown(void);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* TRUETRACE_HIP_H */
