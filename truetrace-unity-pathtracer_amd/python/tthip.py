"""tthip — Python (ctypes) view of the C ABI in include/truetrace_hip.h and
include/truetrace_scene.h.

The product is the C-ABI library ``lib/libtruetrace_hip.so`` (gfx950 kernels); this module is
thin plumbing so tests and bench.py can drive it. It never falls back to a CPU path: if the
HIP library is missing or no GPU is visible, the trace entry points raise.

Names mirror the reference dispatch surface:
  * ``AssetManager`` — owns the aggregated buffers (AssetManager.cs:75-88 SetMeshTraceBuffers,
    :986-1227 AccumulateData, :1610-1766 UpdateTLAS) and uploads them (tt_scene_upload);
  * ``Engine.trace`` — one ``kernel_trace`` dispatch (RayTracingMaster.cs:964-970).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(PKG_DIR, "lib")

# ---------------------------------------------------------------- status codes
TT_OK = 0
TT_ERR_INVALID_ARG = 1
TT_ERR_OOM = 2
TT_ERR_HIP = 3
TT_ERR_UNSUPPORTED = 4
TT_ERR_STACK_OVERFLOW = 5
TT_ERR_NO_DEVICE = 6
TT_ERR_NO_SCENE = 7
STATUS_NAMES = {0: "TT_OK", 1: "TT_ERR_INVALID_ARG", 2: "TT_ERR_OOM", 3: "TT_ERR_HIP", 4: "TT_ERR_UNSUPPORTED",
                5: "TT_ERR_STACK_OVERFLOW", 6: "TT_ERR_NO_DEVICE", 7: "TT_ERR_NO_SCENE"}

TT_TRACE_DEVICE_PTRS = 1 << 0
TT_TRACE_USE_RESTIRGI = 1 << 1
TT_TRACE_USE_ASVGF = 1 << 2
TT_TRACE_STATS = 1 << 3
TT_TRACE_ASYNC = 1 << 4
TT_TRACE_IGNORE_GLASS = 1 << 5       # IgnoreGlassMain (IntersectionKernels.compute:42-44)
TT_TRACE_IGNORE_BACKFACING = 1 << 6  # IgnoreBackfacing (IntersectionKernels.compute:45-47)
TT_TRACE_ADAPTIVE_ORDER = 1 << 7  # dequeue the previous launch's costliest tiles first (tt_order.hip)
TT_ENQUEUE_TERRAIN_BOUNCE = 1 << 8  # tt_enqueue_diffuse_bounce(_indirect): terrain hits bounce off the terrain
# tt_trace_last_form: which closest-hit kernel form a context's last trace launch took
TT_TRACE_FORM_NONE, TT_TRACE_FORM_GENERIC, TT_TRACE_FORM_LEAF = 0, 1, 2
# tt_tlas_root_form: what a TLAS's node 0 is (2: one leaf of one instance, the leaf-TLAS kernels' condition)
TT_ROOT_GENERIC, TT_ROOT_ONE_LEAF, TT_ROOT_ONE_INSTANCE = 0, 1, 2
TT_NEE_NEGATIVE_T = 1 << 9  # tt_emit_nee(_indirect): every written t negated (the PrimaryNEERay / Indirect form)
TT_LIGHT_MAX_REPS = 322     # SampleLightBVH's loop bound (CommonData.cginc:1132)
TT_LIGHT_REFIT_CONSERVATIVE = 1 << 10  # tt_lights_refit: every cone contains the cones below it
TT_SHADOW_RADIANCE_CACHE = 1 << 7    # RadianceCache define (GlobalDefines.cginc:15) for tt_trace_shadow_ex
TT_SHADOW_VISIBILITY_CHECK = 1 << 8  # VisabilityCheckCompute semantics (CommonData.cginc:710-819)
TT_TERRAIN_MESH_ID = 9999999   # mesh_id of a terrain hit record (IntersectionKernels.compute:686)
TT_TERRAIN_MAX_STEPS = 2000    # step bound of the heightmap march per terrain (:535, :653)
TT_STACK_SIZE = 16
TT_MAX_REPS = 1000

# ---------------------------------------------------------------- numpy layouts
NODE_DTYPE = np.dtype([("p", "<f4", 3), ("e_imask", "<u4"), ("base_child", "<u4"), ("base_tri", "<u4"),
                       ("meta", "<u4", 2), ("qlo_x", "<u4", 2), ("qhi_x", "<u4", 2), ("qlo_y", "<u4", 2),
                       ("qhi_y", "<u4", 2), ("qlo_z", "<u4", 2), ("qhi_z", "<u4", 2)])
TRI_DTYPE = np.dtype([("pos0", "<f4", 3), ("posedge1", "<f4", 3), ("posedge2", "<f4", 3), ("norms", "<u4", 3),
                      ("tans", "<u4", 3), ("tex0", "<f4", 2), ("texedge1", "<f4", 2), ("texedge2", "<f4", 2),
                      ("MatDat", "<u4")])
MESH_DTYPE = np.dtype([("W2L", "<f4", 16), ("TriOffset", "<i4"), ("NodeOffset", "<i4"), ("MaterialOffset", "<i4"),
                       ("mesh_data_bvh_offsets", "<i4"), ("LightTriCount", "<i4"), ("LightNodeOffset", "<i4")])
MAT_DTYPE = np.dtype([("AlbedoTex", "<i4", 2), ("NormalTex", "<i4", 2), ("EmissiveTex", "<i4", 2),
                      ("MetallicTex", "<i4", 2), ("RoughnessTex", "<i4", 2), ("AlphaTex", "<i4", 2),
                      ("MatCapMask", "<i4", 2), ("MatCapTex", "<i4", 2), ("surfaceColor", "<f4", 3),
                      ("emmissive", "<f4"), ("EmissionColor", "<f4", 3), ("Tag", "<u4"), ("roughness", "<f4"),
                      ("MatType", "<i4"), ("transmittanceColor", "<f4", 3), ("ior", "<f4"), ("metallic", "<f4"),
                      ("sheen", "<f4"), ("sheenTint", "<f4"), ("specularTint", "<f4"), ("clearcoat", "<f4"),
                      ("clearcoatGloss", "<f4"), ("anisotropic", "<f4"), ("flatness", "<f4"), ("diffTrans", "<f4"),
                      ("specTrans", "<f4"), ("Specular", "<f4"), ("scatterDistance", "<f4"),
                      ("AlbedoTexScale", "<f4", 4), ("MetallicRemap", "<f4", 2), ("RoughnessRemap", "<f4", 2),
                      ("AlphaCutoff", "<f4"), ("NormalStrength", "<f4"), ("Hue", "<f4"), ("Saturation", "<f4"),
                      ("Contrast", "<f4"), ("Brightness", "<f4"), ("BlendColor", "<f4", 3), ("BlendFactor", "<f4"),
                      ("SecondaryTexScale", "<f4", 2), ("Rotation", "<f4")])
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("PixelIndex", "<u4"), ("direction", "<f4", 3), ("last_pdf", "<f4"),
                      ("hits", "<u4", 4)])
COL_DTYPE = np.dtype([("throughput", "<f4", 3), ("Direct", "<f4", 3), ("Indirect", "<f4", 3),
                      ("PrimaryNEERay", "<u4"), ("Flags", "<u4"), ("MetRoughIsSpec", "<u4"), ("Data", "<f4", 4)])
for _dt, _sz in ((NODE_DTYPE, 80), (TRI_DTYPE, 88), (MESH_DTYPE, 88), (MAT_DTYPE, 252), (RAY_DTYPE, 48),
                 (COL_DTYPE, 64)):
    assert _dt.itemsize == _sz, (_dt, _sz)
assert MAT_DTYPE.fields["Tag"][1] == 92 and MAT_DTYPE.fields["MatType"][1] == 100
assert MAT_DTYPE.fields["AlbedoTexScale"][1] == 168 and MAT_DTYPE.fields["AlphaCutoff"][1] == 200

MAT_CUTOUT_INDEX = 2
FLAG_INVISIBLE = 7


# ---------------------------------------------------------------- ctypes structs
# ShadowRayData (CommonData.cginc:116-123)
SHADOW_DTYPE = np.dtype([("origin", "<f4", 3), ("LuminanceIncomming", "<f4"), ("direction", "<f4", 3), ("t", "<f4"),
                         ("illumination", "<f4", 3), ("PixelIndex", "<u4")])
assert SHADOW_DTYPE.itemsize == 48
# PropogatedCacheData (CommonData.cginc:1621-1627, PropDepth 4): the RadianceCache record per pixel
# TerrainData, 60 B (CommonVars.cs:147-157, CommonData.cginc:280-287)
TERRAIN_DTYPE = np.dtype([("PositionOffset", "<f4", 3), ("HeightScale", "<f4"), ("TerrainDim", "<f4", 2),
                          ("AlphaMap", "<f4", 4), ("HeightMap", "<f4", 4), ("MatOffset", "<i4")])
assert TERRAIN_DTYPE.itemsize == 60
CACHE_DTYPE = np.dtype([("samples", "<u4", (4, 2)), ("throughput", "<u4"), ("pathLength", "<u4"),
                        ("CurrentIlluminance", "<u4"), ("Norm", "<u4")])
assert CACHE_DTYPE.itemsize == 48 and CACHE_DTYPE.fields["CurrentIlluminance"][1] == 40
TT_FLAG_IS_BACKGROUND, TT_FLAG_SHADOW_CASTER = 5, 6


# LightBVHData / LightTriData / LightMeshData (CommonData.cginc:987-994, :297-314), tt_light_sample, tt_light_bounds
LIGHT_NODE_DTYPE = np.dtype([("BBMax", "<f4", 3), ("BBMin", "<f4", 3), ("w", "<u4"), ("phi", "<f4"),
                             ("cosTheta_oe", "<u4"), ("left", "<i4")])
LIGHT_TRI_DTYPE = np.dtype([("pos0", "<f4", 3), ("posedge1", "<f4", 3), ("posedge2", "<f4", 3), ("TriTarget", "<u4")])
LIGHT_MESH_DTYPE = np.dtype([("Center", "<f4", 3), ("StartIndex", "<i4"), ("IndexEnd", "<i4"), ("MatOffset", "<i4"),
                             ("LockedMeshIndex", "<i4")])
LIGHT_SAMPLE_DTYPE = np.dtype([("light_tri", "<i4"), ("mesh_index", "<i4"), ("agg_tri", "<i4"), ("steps", "<i4"),
                               ("weight", "<f4"), ("area", "<f4"), ("position", "<f4", 3), ("normal", "<f4", 3)])
LIGHT_BOUNDS_DTYPE = np.dtype([("BBMax", "<f4", 3), ("BBMin", "<f4", 3), ("w", "<f4", 3), ("phi", "<f4"),
                               ("cosTheta_o", "<f4"), ("cosTheta_e", "<f4"), ("LightCount", "<i4"), ("Pad1", "<f4")])
# LightBVHTransform (AssetManager.cs:1311-1314): Transform column-major, element (r, c) at [c * 4 + r]
LIGHT_TRANSFORM_DTYPE = np.dtype([("Transform", "<f4", 16), ("SolidOffset", "<i4")])
assert (LIGHT_NODE_DTYPE.itemsize, LIGHT_TRI_DTYPE.itemsize, LIGHT_MESH_DTYPE.itemsize, LIGHT_SAMPLE_DTYPE.itemsize) == (40, 40, 28, 48)
assert LIGHT_TRANSFORM_DTYPE.itemsize == 68


class LightParent(C.Structure):
    _fields_ = [("tris", C.c_void_p), ("normals", C.c_void_p), ("n_tris", C.c_uint32)]


class LightInstance(C.Structure):
    _fields_ = [("parent", C.c_uint32), ("mesh_index", C.c_int32), ("local_to_world", C.c_float * 16)]


class ShadowParams(C.Structure):
    _fields_ = [("n_rays", C.c_uint32), ("bounce", C.c_int32), ("screen_width", C.c_uint32),
                ("screen_height", C.c_uint32), ("flags", C.c_uint32)]


class BlasRefitParams(C.Structure):
    _fields_ = [("mesh_index", C.c_uint32), ("n_tris", C.c_uint32), ("n_vertices", C.c_uint32),
                ("vertex_stride", C.c_uint32), ("transform", C.c_float * 16), ("flags", C.c_uint32)]


class BlasRefitPart(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("n_vertices", C.c_uint32), ("vertex_stride", C.c_uint32),
                ("indices", C.c_void_p), ("n_tris", C.c_uint32), ("first_tri", C.c_uint32),
                ("transform", C.c_float * 16)]


class BlasRefitItem(C.Structure):
    _fields_ = [("mesh_index", C.c_uint32), ("n_tris", C.c_uint32), ("leaf_of_triangle", C.c_void_p),
                ("parts", C.POINTER(BlasRefitPart)), ("n_parts", C.c_uint32), ("local_to_world", C.c_void_p)]


class TraceParams(C.Structure):
    _fields_ = [("n_rays", C.c_uint32), ("bounce", C.c_int32), ("far_plane", C.c_float),
                ("screen_width", C.c_uint32), ("screen_height", C.c_uint32), ("flags", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64),
                ("blas_entries", C.c_uint64), ("hits", C.c_uint64), ("reps_exhausted", C.c_uint64),
                ("stack_overflows", C.c_uint64), ("accepts", C.c_uint64), ("kernel_ms", C.c_float),
                ("pad", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32), ("max_rays", C.c_uint64), ("stream", C.c_void_p)]


class Camera(C.Structure):
    _fields_ = [("cam_to_world", C.c_float * 16), ("cam_inv_proj", C.c_float * 16), ("near_plane", C.c_float),
                ("far_plane", C.c_float), ("width", C.c_uint32), ("height", C.c_uint32), ("jitter", C.c_int32),
                ("frames_accumulated", C.c_int32), ("max_bounce", C.c_int32), ("flags", C.c_uint32)]


class MeshInput(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("n_vertices", C.c_uint32), ("normals", C.c_void_p),
                ("tangents", C.c_void_p), ("uvs", C.c_void_p), ("indices", C.c_void_p), ("n_indices", C.c_uint32),
                ("matdat", C.c_void_p), ("lossy_scale", C.c_float * 3)]


class BlasInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_tris", C.c_uint32), ("bvh2_depth", C.c_uint32),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3), ("build_seconds", C.c_double)]


class ParentDesc(C.Structure):
    _fields_ = [("blas", C.c_void_p), ("local_to_world", C.c_float * 16), ("world_to_local", C.c_float * 16),
                ("material_count", C.c_uint32)]


class InstanceDesc(C.Structure):
    _fields_ = [("instance_parent", C.c_uint32), ("local_to_world", C.c_float * 16),
                ("world_to_local", C.c_float * 16)]


class SceneBuildInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_tris", C.c_uint32), ("n_tlas_indices", C.c_uint32),
                ("n_mesh", C.c_uint32), ("tlas_nodes", C.c_uint32), ("pad", C.c_uint32)]


class ObjectInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_tris", C.c_uint32), ("device", C.c_int32), ("root", C.c_uint32),
                ("bytes", C.c_uint64)]


class ObjectBuildInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_tris", C.c_uint32), ("bvh2_depth", C.c_uint32), ("max_matdat", C.c_uint32),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3), ("presorted_on_host", C.c_uint32),
                ("pad", C.c_uint32)]


class ObjectDesc(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_tris", C.c_uint32), ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
                ("local_to_world", C.c_float * 16), ("world_to_local", C.c_float * 16), ("material_count", C.c_uint32)]


class TTError(RuntimeError):
    def __init__(self, status: int, msg: str = ""):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


def _check(st: int, what: str):
    if st != TT_OK:
        raise TTError(st, what)


def _ptr(a) -> Optional[int]:
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"], "arrays passed to the C ABI must be contiguous"
        return a.ctypes.data
    if hasattr(a, "data_ptr"):  # torch tensor
        return a.data_ptr()
    return int(a)


# ---------------------------------------------------------------- library loading
_SCENE = None
_HIP = None

HIP_SYMBOLS = ["tt_abi_version", "tt_device_count", "tt_ctx_create", "tt_ctx_destroy", "tt_last_error",
               "tt_scene_upload", "tt_scene_update_nodes", "tt_scene_update_meshdata", "tt_scene_bytes",
               "tt_trace_closest", "tt_sync", "tt_ctx_stream", "tt_resolve_normals", "tt_generate_primary",
               "tt_enqueue_diffuse_bounce", "tt_trace_closest_indirect", "tt_enqueue_diffuse_bounce_indirect",
               "tt_trace_shadow_ex_indirect", "tt_timing_reset", "tt_timing_read", "tt_scene_validate", "tt_trace_diagnostics",
               "tt_selftest_rcp", "tt_trace_closest_hits", "tt_ctx_share_scene", "tt_scene_upload_terrains",
               "tt_terrain_validate", "tt_trace_heightmap", "tt_trace_heightmap_indirect", "tt_trace_shadow_heightmap",
               "tt_trace_shadow_heightmap_indirect", "tt_object_validate", "tt_object_create", "tt_object_get_info",
               "tt_object_destroy", "tt_scene_layout_objects", "tt_scene_layout_counts", "tt_scene_assemble_objects",
               "tt_object_build_device", "tt_object_read", "tt_object_leaf_order_device", "tt_objects_build_device",
               "tt_scene_update_tlas", "tt_tlas_rebuild", "tt_scene_read_tlas_indices", "tt_group_tlas_rebuild",
               "tt_group_scene_update_tlas", "tt_blas_refit_many", "tt_blas_refit_items_validate", "tt_lights_validate",
               "tt_scene_upload_lights", "tt_scene_update_light_nodes", "tt_emit_nee", "tt_emit_nee_indirect",
               "tt_lights_refit", "tt_scene_read_light_nodes", "tt_scene_read_light_tris"]
SCENE_SYMBOLS = ["tt_blas_build", "tt_blas_get_info", "tt_blas_copy", "tt_blas_free", "tt_scene_assemble",
                 "tt_scene_build_get_info", "tt_scene_build_copy", "tt_scene_build_free", "tt_pack_octahedral",
                 "tt_bvh2_build", "tt_dotnet_sort_by_key", "tt_synth_cornell", "tt_synth_soup", "tt_synth_sponza",
                 "tt_synth_prop", "tt_synth_ground", "tt_synth_san_miguel", "tt_synth_mesh_view", "tt_synth_mesh_free",
                 "tt_synth_mesh_from_arrays", "tt_blas_copy_leaf_order", "tt_blas_prepare_aabbs", "tt_bvh2_presort",
                 "tt_blas_build_from_bvh2", "tt_blas_build_from_cwbvh", "tt_blas_prepare",
                 "tt_blas_build_from_cwbvh_prepared", "tt_blas_prep_free", "tt_terrain_trace_host",
                 "tt_terrain_trace_detail_host", "tt_terrain_occluded_host", "tt_terrain_normal_host",
                 "tt_scene_assemble_tlas", "tt_scene_build_get_totals", "tt_tlas_build", "tt_light_tris_from_mesh",
                 "tt_light_bvh_build_mesh", "tt_light_bvh_build_tlas", "tt_light_bounds_transform", "tt_lights_assemble",
                 "tt_emit_nee_host", "tt_lights_refit_host", "tt_light_refit_math"]


def scene_lib():
    global _SCENE
    if _SCENE is None:
        path = os.path.join(LIB_DIR, "libtruetrace_scene.so")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} missing: run `make -C truetrace-unity-pathtracer_amd` or __graft_entry__.build()")
        L = C.CDLL(path)
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
        L.tt_blas_build.argtypes = [C.POINTER(MeshInput), C.POINTER(vp)]
        L.tt_blas_get_info.argtypes = [vp, C.POINTER(BlasInfo)]
        L.tt_blas_copy.argtypes = [vp, vp, vp]
        L.tt_blas_free.argtypes = [vp]
        L.tt_blas_free.restype = None
        L.tt_blas_copy_leaf_order.argtypes = [vp, vp]
        L.tt_blas_copy_leaf_order.restype = i32
        L.tt_scene_assemble.argtypes = [vp, u32, vp, u32, vp, u32, C.POINTER(vp)]
        L.tt_scene_assemble_tlas.argtypes = [vp, u32, vp, u32, vp, u32, C.POINTER(vp)]
        L.tt_scene_assemble_tlas.restype = i32
        L.tt_scene_build_get_totals.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
        L.tt_scene_build_get_totals.restype = i32
        L.tt_scene_build_get_info.argtypes = [vp, C.POINTER(SceneBuildInfo)]
        L.tt_scene_build_copy.argtypes = [vp, vp, vp, vp, vp]
        L.tt_scene_build_free.argtypes = [vp]
        L.tt_scene_build_copy_mesh_aabbs.argtypes = [vp, vp]
        L.tt_tlas_build.argtypes = [vp, u32, vp, C.POINTER(u32), vp]
        L.tt_tlas_build.restype = i32
        L.tt_scene_build_free.restype = None
        L.tt_pack_octahedral.argtypes = [C.c_float, C.c_float, C.c_float]
        L.tt_pack_octahedral.restype = u32
        L.tt_bvh2_build.argtypes = [vp, u32, vp, vp, vp, vp]
        L.tt_blas_prepare_aabbs.argtypes = [C.POINTER(MeshInput), vp]
        L.tt_bvh2_presort.argtypes = [vp, u32, vp]
        L.tt_blas_build_from_bvh2.argtypes = [C.POINTER(MeshInput), vp, vp, vp, vp, u32, C.POINTER(vp)]
        L.tt_blas_build_from_cwbvh.argtypes = [C.POINTER(MeshInput), vp, u32, vp, u32, C.POINTER(vp)]
        L.tt_blas_prepare.argtypes = [C.POINTER(MeshInput), vp, C.POINTER(vp)]
        L.tt_blas_build_from_cwbvh_prepared.argtypes = [vp, vp, u32, vp, u32, C.POINTER(vp)]
        L.tt_blas_prep_free.argtypes = [vp]
        L.tt_blas_prep_free.restype = None
        L.tt_dotnet_sort_by_key.argtypes = [vp, u32, vp]
        L.tt_dotnet_sort_by_key.restype = None
        L.tt_synth_cornell.argtypes = [C.POINTER(vp)]
        L.tt_synth_soup.argtypes = [C.c_uint64, u32, C.c_float, C.c_float, C.POINTER(vp)]
        L.tt_synth_sponza.argtypes = [C.c_uint64, u32, C.POINTER(vp)]
        L.tt_synth_prop.argtypes = [C.c_uint64, u32, C.POINTER(vp)]
        L.tt_synth_ground.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, u32, u32, C.POINTER(vp)]
        L.tt_synth_san_miguel.argtypes = [C.c_uint64, u32, C.POINTER(vp)]
        L.tt_synth_mesh_view.argtypes = [vp, C.POINTER(MeshInput)]
        L.tt_synth_mesh_free.argtypes = [vp]
        L.tt_synth_mesh_free.restype = None
        L.tt_synth_mesh_from_arrays.argtypes = [vp, u32, vp, u32, vp]
        L.tt_synth_mesh_from_arrays.restype = vp
        L.tt_terrain_trace_host.argtypes = [vp, u32, vp, u32, u32, C.POINTER(TraceParams), vp, vp, C.POINTER(Stats)]
        L.tt_terrain_trace_detail_host.argtypes = [vp, u32, vp, u32, u32, C.POINTER(TraceParams), vp, vp,
                                                   C.POINTER(Stats), vp]
        L.tt_terrain_occluded_host.argtypes = [vp, u32, vp, u32, u32, vp, u32, vp, C.POINTER(Stats)]
        L.tt_terrain_normal_host.argtypes = [vp, u32, vp, u32, u32, vp, u32, vp]
        L.tt_terrain_bounce_host.argtypes = [vp, u32, vp, u32, u32, C.POINTER(TraceParams), vp, i32, i32, u32, vp, vp]
        for s in ["tt_terrain_trace_host", "tt_terrain_trace_detail_host", "tt_terrain_occluded_host",
                  "tt_terrain_normal_host", "tt_terrain_bounce_host"]:
            getattr(L, s).restype = i32
        L.tt_light_tris_from_mesh.argtypes = [vp, u32, vp, u32, vp, vp, vp]
        L.tt_light_bvh_build_mesh.argtypes = [vp, vp, u32, vp, vp]
        L.tt_light_bvh_build_tlas.argtypes = [vp, u32, vp]
        L.tt_light_bounds_transform.argtypes = [vp, vp, vp]
        L.tt_lights_assemble.argtypes = [C.POINTER(LightParent), u32, C.POINTER(LightInstance), u32, vp, u32, vp,
                                         C.POINTER(u32), vp, C.POINTER(u32), vp]
        L.tt_emit_nee_host.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, C.POINTER(TraceParams), vp, i32, i32,
                                       u32, u32, vp, vp, C.POINTER(u32)]
        L.tt_lights_refit_host.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, u32,
                                           C.c_char_p, u32]
        L.tt_light_refit_math.argtypes = [u32, vp, u32, vp]
        for s in ["tt_light_tris_from_mesh", "tt_light_bvh_build_mesh", "tt_light_bvh_build_tlas",
                  "tt_light_bounds_transform", "tt_lights_assemble", "tt_emit_nee_host", "tt_lights_refit_host",
                  "tt_light_refit_math"]:
            getattr(L, s).restype = i32
        for s in ["tt_blas_build", "tt_blas_get_info", "tt_blas_copy", "tt_scene_assemble", "tt_scene_build_get_info",
                  "tt_scene_build_copy", "tt_bvh2_build", "tt_synth_cornell", "tt_synth_soup", "tt_synth_sponza",
                  "tt_synth_prop", "tt_synth_ground", "tt_synth_san_miguel", "tt_synth_mesh_view"]:
            getattr(L, s).restype = i32
        _SCENE = L
    return _SCENE


def hip_lib():
    """The gfx950 engine. Raises if the library was not built — there is no CPU fallback."""
    global _HIP
    if _HIP is None:
        # torch ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7). Load it
        # first so our NEEDED libamdhip64.so.7 binds to that same runtime: two HIP/HSA runtimes in one
        # process break torch.cuda / RCCL. Without torch the system ROCm runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        path = os.environ.get("TT_HIP_LIB") or os.path.join(LIB_DIR, "libtruetrace_hip.so")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} missing: the HIP engine was not built (no fallback exists)")
        L = C.CDLL(path)
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
        L.tt_abi_version.restype = i32
        L.tt_device_count.restype = i32
        L.tt_ctx_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
        L.tt_ctx_destroy.argtypes = [vp]
        L.tt_last_error.argtypes = [vp]
        L.tt_last_error.restype = C.c_char_p
        L.tt_scene_upload.argtypes = [vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32]
        L.tt_scene_update_nodes.argtypes = [vp, u32, u32, vp]
        L.tt_scene_update_meshdata.argtypes = [vp, u32, u32, vp]
        L.tt_scene_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.tt_trace_closest.argtypes = [vp, C.POINTER(TraceParams), vp, vp, vp, C.POINTER(Stats)]
        L.tt_trace_shadow.argtypes = [vp, C.POINTER(ShadowParams), vp, vp, vp, vp, C.POINTER(Stats)]
        L.tt_trace_shadow_ex.argtypes = [vp, C.POINTER(ShadowParams), vp, vp, vp, vp, vp, C.POINTER(Stats)]
        if hasattr(L, "tt_trace_closest_indirect"):  # (absent from round-2 variant libraries, tools/run_variants.py)
            L.tt_trace_closest_indirect.argtypes = [vp, C.POINTER(TraceParams), vp, vp, vp, vp]
            L.tt_trace_shadow_ex_indirect.argtypes = [vp, C.POINTER(ShadowParams), vp, vp, vp, vp, vp, vp]
            L.tt_enqueue_diffuse_bounce_indirect.argtypes = [vp, C.POINTER(TraceParams), vp, vp, i32, i32, vp]
        if hasattr(L, "tt_ctx_share_scene"):
            L.tt_ctx_share_scene.argtypes = [vp, vp]
        if hasattr(L, "tt_ctx_share_blas"):
            L.tt_ctx_share_blas.argtypes = [vp, vp, u32]
        if hasattr(L, "tt_trace_chunk_costs"):
            L.tt_trace_chunk_costs.argtypes = [vp, i32, vp, u32, C.POINTER(u32)]
            L.tt_trace_chunk_costs.restype = i32
        if hasattr(L, "tt_trace_closest_hits"):
            L.tt_trace_closest_hits.argtypes = [vp, C.POINTER(TraceParams), vp, vp, vp, vp]
        L.tt_scene_upload_alpha_atlas.argtypes = [vp, vp, u32, u32]
        L.tt_scene_upload_texture_atlas.argtypes = [vp, vp, u32, u32]
        L.tt_tlas_refit.argtypes = [vp, u32, vp, u32, u32]
        if hasattr(L, "tt_scene_upload_terrains"):  # (absent from older variant libraries)
            L.tt_scene_upload_terrains.argtypes = [vp, vp, u32, vp, u32, u32]
            L.tt_terrain_validate.argtypes = [vp, u32, vp, u32, u32, C.c_char_p, u32]
            L.tt_trace_heightmap.argtypes = [vp, C.POINTER(TraceParams), vp, vp, C.POINTER(Stats)]
            L.tt_trace_heightmap_indirect.argtypes = [vp, C.POINTER(TraceParams), vp, vp, vp]
            if hasattr(L, "tt_trace_heightmap_hits"):
                L.tt_trace_heightmap_hits.argtypes = [vp, C.POINTER(TraceParams), vp, vp, vp]
                L.tt_trace_heightmap_hits.restype = i32
            L.tt_trace_shadow_heightmap.argtypes = [vp, C.POINTER(ShadowParams), vp, vp, vp, vp, vp]
            L.tt_trace_shadow_heightmap_indirect.argtypes = [vp, C.POINTER(ShadowParams), vp, vp, vp, vp, vp, vp]
            for s in ["tt_scene_upload_terrains", "tt_terrain_validate", "tt_trace_heightmap",
                      "tt_trace_heightmap_indirect", "tt_trace_shadow_heightmap", "tt_trace_shadow_heightmap_indirect"]:
                getattr(L, s).restype = i32
        if hasattr(L, "tt_object_create"):  # (absent from older variant libraries)
            L.tt_object_validate.argtypes = [vp, u32, vp, u32, u32, C.c_char_p, u32]
            L.tt_object_create.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(vp)]
            L.tt_object_get_info.argtypes = [vp, C.POINTER(ObjectInfo)]
            L.tt_object_destroy.argtypes = [vp]
            L.tt_scene_layout_objects.argtypes = [vp, u32, u32, vp, vp, C.POINTER(u32), C.POINTER(u32)]
            L.tt_scene_layout_counts.argtypes = [vp, vp, u32, u32, vp, vp, C.POINTER(u32), C.POINTER(u32)]
            L.tt_scene_assemble_objects.argtypes = [vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32]
            for s in ["tt_object_validate", "tt_object_create", "tt_object_get_info", "tt_object_destroy",
                      "tt_scene_layout_objects", "tt_scene_layout_counts", "tt_scene_assemble_objects"]:
                getattr(L, s).restype = i32
        if hasattr(L, "tt_object_build_device"):  # (absent from older variant libraries)
            L.tt_object_build_device.argtypes = [vp, C.POINTER(MeshInput), vp, u32, C.POINTER(vp),
                                                 C.POINTER(ObjectBuildInfo)]
            L.tt_object_read.argtypes = [vp, vp, vp, vp, vp]
            L.tt_object_leaf_order_device.argtypes = [vp, C.POINTER(vp)]
            for s in ["tt_object_build_device", "tt_object_read", "tt_object_leaf_order_device"]:
                getattr(L, s).restype = i32
        if hasattr(L, "tt_objects_build_device"):  # (absent from older libraries)
            L.tt_objects_build_device.argtypes = [vp, C.POINTER(MeshInput), u32, C.POINTER(vp), u32, C.POINTER(vp),
                                                  C.POINTER(ObjectBuildInfo), C.POINTER(i32)]
            L.tt_objects_build_device.restype = i32
        if hasattr(L, "tt_tlas_rebuild"):  # (absent from older libraries)
            L.tt_scene_update_tlas.argtypes = [vp, vp, u32, vp, u32, u32]
            L.tt_tlas_rebuild.argtypes = [vp, vp, u32, u32, C.POINTER(u32)]
            L.tt_scene_read_tlas_indices.argtypes = [vp, u32, u32, vp]
            for s in ["tt_scene_update_tlas", "tt_tlas_rebuild", "tt_scene_read_tlas_indices"]:
                getattr(L, s).restype = i32
        L.tt_scene_read_nodes.argtypes = [vp, u32, u32, vp]
        L.tt_scene_read_tris.argtypes = [vp, u32, u32, vp]
        L.tt_blas_refit.argtypes = [vp, C.POINTER(BlasRefitParams), vp, vp, vp]
        if hasattr(L, "tt_blas_refit_many"):  # (absent from older libraries)
            L.tt_blas_refit_many.argtypes = [vp, C.POINTER(BlasRefitItem), u32, u32, vp, vp]
            L.tt_blas_refit_items_validate.argtypes = [C.POINTER(BlasRefitItem), u32, vp, u32, u32, u32, C.c_char_p, u32]
            for s in ["tt_blas_refit_many", "tt_blas_refit_items_validate"]:
                getattr(L, s).restype = i32
        if hasattr(L, "tt_emit_nee"):  # (absent from older libraries)
            L.tt_lights_validate.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, u32, C.c_char_p, u32]
            L.tt_scene_upload_lights.argtypes = [vp, vp, u32, vp, u32, vp, u32]
            L.tt_scene_update_light_nodes.argtypes = [vp, u32, u32, vp]
            L.tt_emit_nee.argtypes = [vp, C.POINTER(TraceParams), vp, i32, i32, vp, vp, C.POINTER(u32)]
            L.tt_emit_nee_indirect.argtypes = [vp, C.POINTER(TraceParams), vp, vp, i32, i32, vp, vp, vp]
            for s in ["tt_lights_validate", "tt_scene_upload_lights", "tt_scene_update_light_nodes", "tt_emit_nee",
                      "tt_emit_nee_indirect"]:
                getattr(L, s).restype = i32
        if hasattr(L, "tt_lights_refit"):  # (absent from older libraries)
            L.tt_lights_refit.argtypes = [vp, vp, u32, vp, u32, u32]
            L.tt_scene_read_light_nodes.argtypes = [vp, u32, u32, vp]
            L.tt_scene_read_light_tris.argtypes = [vp, u32, u32, vp]
            for s in ["tt_lights_refit", "tt_scene_read_light_nodes", "tt_scene_read_light_tris"]:
                getattr(L, s).restype = i32
        L.tt_bvh2_build_device.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, C.POINTER(u32)]
        L.tt_blas_build_device.argtypes = [vp, vp, u32, vp, vp, u32, C.POINTER(u32), vp, C.POINTER(u32)]
        L.tt_bvh2_presort_device.argtypes = [vp, vp, u32, vp]
        L.tt_sync.argtypes = [vp]
        if hasattr(L, "tt_stream_create"):
            L.tt_stream_create.argtypes = [i32, C.POINTER(vp)]
            L.tt_stream_create.restype = i32
            L.tt_stream_destroy.argtypes = [vp]
            L.tt_stream_destroy.restype = i32
        if hasattr(L, "tt_stream_live_count"):
            L.tt_stream_live_count.restype = u32
        L.tt_async_overflows.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.tt_ctx_stream.argtypes = [vp]
        L.tt_ctx_stream.restype = vp
        L.tt_resolve_normals.argtypes = [vp, C.POINTER(TraceParams), vp, vp]
        L.tt_generate_primary.argtypes = [vp, C.POINTER(Camera), vp]
        L.tt_enqueue_diffuse_bounce.argtypes = [vp, C.POINTER(TraceParams), vp, i32, i32, C.POINTER(u32)]
        L.tt_scene_validate.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, C.c_char_p, u32]
        L.tt_scene_validate.restype = i32
        L.tt_trace_diagnostics.argtypes = [vp, vp]
        L.tt_trace_diagnostics.restype = i32
        L.tt_trace_last_form.argtypes = [vp, C.POINTER(u32)]
        L.tt_trace_last_form.restype = i32
        L.tt_tlas_root_form.argtypes = [vp, C.POINTER(u32)]
        L.tt_tlas_root_form.restype = i32
        L.tt_selftest_rcp.argtypes = [vp, vp]
        L.tt_selftest_rcp.restype = i32
        L.tt_timing_reset.argtypes = [vp]
        L.tt_timing_read.argtypes = [vp, vp, u32, C.POINTER(u32)]
        L.tt_ctx_set_timing.argtypes = [vp, i32]
        L.tt_ctx_set_timing.restype = i32
        L.tt_ctx_set_frame_pixels.argtypes = [vp, C.c_uint32]
        L.tt_ctx_set_frame_pixels.restype = i32
        for s in ["tt_ctx_create", "tt_ctx_destroy", "tt_scene_upload", "tt_scene_update_nodes",
                  "tt_scene_update_meshdata", "tt_scene_bytes", "tt_trace_closest", "tt_sync", "tt_resolve_normals",
                  "tt_generate_primary", "tt_enqueue_diffuse_bounce", "tt_timing_reset", "tt_timing_read"]:
            getattr(L, s).restype = i32
        if hasattr(L, "tt_group_create"):  # (absent from older variant libraries)
            _bind_group(L)
        _HIP = L
    return _HIP


# ---------------------------------------------------------------- terrains
def _half_bits(heightmap) -> np.ndarray:
    hm = np.ascontiguousarray(heightmap)
    return hm.view(np.uint16) if hm.dtype == np.float16 else np.ascontiguousarray(hm, np.uint16)


def terrain_validate(terrains, heightmap):
    """tt_terrain_validate (host only): (status, reason) of what tt_scene_upload_terrains would answer."""
    t = np.ascontiguousarray(terrains, TERRAIN_DTYPE)
    hm = None if heightmap is None else _half_bits(heightmap)
    h, w = (0, 0) if hm is None else hm.shape
    why = C.create_string_buffer(256)
    st = hip_lib().tt_terrain_validate(_ptr(t) if len(t) else None, len(t), _ptr(hm), w, h, why, 256)
    return st, why.value.decode()


def synthetic_heightmap(seed: int, w: int, h: int) -> np.ndarray:
    """A seeded heightmap as binary16 bits (uint16 [h, w], values in [0, 1]): a few smooth sine hills plus one
    vertical step (a cliff along a line x = const), the two shapes a heightmap march meets."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64) / max(h - 1, 1), np.arange(w, dtype=np.float64) / max(w - 1, 1),
                       indexing="ij")
    z = np.zeros((h, w))
    for _ in range(4):
        fx, fy = rng.uniform(0.5, 3.0, 2)
        px, py = rng.uniform(0.0, 2.0 * np.pi, 2)
        z += rng.uniform(0.3, 1.0) * np.sin(2.0 * np.pi * fx * x + px) * np.sin(2.0 * np.pi * fy * y + py)
    z = (z - z.min()) / max(z.max() - z.min(), 1e-12) * 0.6
    z[:, x[0] > rng.uniform(0.55, 0.75)] += 0.4  # the step
    return np.clip(z, 0.0, 1.0).astype(np.float16).view(np.uint16)


def terrain_trace_host(terrains, heightmap, rays, n_rays, bounce, far_plane, width, height, info=None, flags=0,
                       detail=None) -> Stats:
    """tt_terrain_trace_(detail_)host: the scalar host reference of tt_trace_heightmap, in place on rays / info."""
    t = np.ascontiguousarray(terrains, TERRAIN_DTYPE)
    hm = _half_bits(heightmap)
    p = TraceParams(n_rays=n_rays, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                    flags=flags)
    s = Stats()
    _check(scene_lib().tt_terrain_trace_detail_host(_ptr(t), len(t), _ptr(hm), hm.shape[1], hm.shape[0], C.byref(p),
                                                    _ptr(rays), _ptr(info), C.byref(s), _ptr(detail)),
           "tt_terrain_trace_detail_host")
    return s


def terrain_occluded_host(terrains, heightmap, shadow_rays, n_rays):
    """tt_terrain_occluded_host: (occluded uint8 per ray, Stats) of the host reference's shadow march."""
    t = np.ascontiguousarray(terrains, TERRAIN_DTYPE)
    hm = _half_bits(heightmap)
    occ = np.zeros(n_rays, np.uint8)
    s = Stats()
    _check(scene_lib().tt_terrain_occluded_host(_ptr(t), len(t), _ptr(hm), hm.shape[1], hm.shape[0], _ptr(shadow_rays),
                                                n_rays, _ptr(occ), C.byref(s)), "tt_terrain_occluded_host")
    return occ, s


def terrain_normal_host(terrains, heightmap, position, terrain_id: int) -> np.ndarray:
    """tt_terrain_normal_host: GetHeightmapNormal(position, terrain_id)."""
    t = np.ascontiguousarray(terrains, TERRAIN_DTYPE)
    hm = _half_bits(heightmap)
    pos = np.ascontiguousarray(position, np.float32)
    out = np.zeros(3, np.float32)
    _check(scene_lib().tt_terrain_normal_host(_ptr(t), len(t), _ptr(hm), hm.shape[1], hm.shape[0], _ptr(pos),
                                              int(terrain_id), _ptr(out)), "tt_terrain_normal_host")
    return out


def terrain_bounce_host(terrains, heightmap, rays, n_rays, bounce, far_plane, width, height, frames=0, max_bounce=3,
                        frame_pixels=0):
    """tt_terrain_bounce_host: the scalar reference of the enqueue's terrain rows (TT_ENQUEUE_TERRAIN_BOUNCE).
    Returns (out_rays, survives), n_rays entries each: survives -1 not a terrain record, 0 its path ends, 1 it
    survives and out_rays[i] is its new ray (nothing is compacted)."""
    t = np.ascontiguousarray(terrains, TERRAIN_DTYPE)
    hm = _half_bits(heightmap)
    p = TraceParams(n_rays=n_rays, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height, flags=0)
    out = np.zeros(max(1, n_rays), RAY_DTYPE)
    sv = np.zeros(max(1, n_rays), np.int32)
    _check(scene_lib().tt_terrain_bounce_host(_ptr(t) if len(t) else None, len(t), _ptr(hm), hm.shape[1], hm.shape[0],
                                              C.byref(p), _ptr(rays), frames, max_bounce, frame_pixels, _ptr(out),
                                              _ptr(sv)), "tt_terrain_bounce_host")
    return out[:n_rays], sv[:n_rays]


# ---------------------------------------------------------------- lights
@dataclass
class Lights:
    """LightNodes / LightTriangles / _LightMeshes as tt_scene_upload_lights takes them."""
    nodes: np.ndarray
    tris: np.ndarray
    meshes: np.ndarray


def lights_validate(lights: "Lights", meshdata, n_scene_tris: int):
    """tt_lights_validate (host only): (status, reason) of what tt_scene_upload_lights would answer."""
    md = np.ascontiguousarray(meshdata, MESH_DTYPE)
    why = C.create_string_buffer(512)
    st = hip_lib().tt_lights_validate(_ptr(lights.nodes), len(lights.nodes), _ptr(lights.tris), len(lights.tris),
                                      _ptr(lights.meshes), len(lights.meshes), _ptr(md), len(md), int(n_scene_tris), why, 512)
    return st, why.value.decode()


def light_tris_from_mesh(tris, targets, normals=None):
    """tt_light_tris_from_mesh: (LightTriData, normals [n, 3]) of the triangles `targets` of a mesh's records."""
    t = np.ascontiguousarray(tris, TRI_DTYPE)
    tg = np.ascontiguousarray(targets, np.uint32)
    nr = None if normals is None else np.ascontiguousarray(normals, np.float32)
    out = np.zeros(len(tg), LIGHT_TRI_DTYPE)
    on = np.zeros((len(tg), 3), np.float32)
    _check(scene_lib().tt_light_tris_from_mesh(_ptr(t), len(t), _ptr(tg), len(tg), _ptr(nr), _ptr(out), _ptr(on)),
           "tt_light_tris_from_mesh")
    return out, on


def light_bvh_build_mesh(ltris, normals):
    """tt_light_bvh_build_mesh: (2 n nodes, the root's LightBounds)."""
    lt = np.ascontiguousarray(ltris, LIGHT_TRI_DTYPE)
    nr = np.ascontiguousarray(normals, np.float32)
    nodes = np.zeros(2 * len(lt), LIGHT_NODE_DTYPE)
    root = np.zeros(1, LIGHT_BOUNDS_DTYPE)
    _check(scene_lib().tt_light_bvh_build_mesh(_ptr(lt), _ptr(nr), len(lt), _ptr(nodes), _ptr(root)), "tt_light_bvh_build_mesh")
    return nodes, root


def light_bvh_build_tlas(bounds):
    b = np.ascontiguousarray(bounds, LIGHT_BOUNDS_DTYPE)
    nodes = np.zeros(2 * len(b), LIGHT_NODE_DTYPE)
    _check(scene_lib().tt_light_bvh_build_tlas(_ptr(b), len(b), _ptr(nodes)), "tt_light_bvh_build_tlas")
    return nodes


def light_bounds_transform(root, local_to_world):
    """tt_light_bounds_transform: local_to_world is a row-major (math convention) 4x4, as trs_matrix returns."""
    r = np.ascontiguousarray(root, LIGHT_BOUNDS_DTYPE)
    m = unity_colmajor(np.asarray(local_to_world))
    out = np.zeros(1, LIGHT_BOUNDS_DTYPE)
    _check(scene_lib().tt_light_bounds_transform(_ptr(r), _ptr(m), _ptr(out)), "tt_light_bounds_transform")
    return out


def lights_assemble(parents, instances, meshdata) -> "Lights":
    """tt_lights_assemble. parents: [(LightTriData, normals)], instances: [(parent, mesh_index, local_to_world
    row-major 4x4)]; meshdata (MESH_DTYPE) gets LightNodeOffset / LightTriCount in place."""
    assert meshdata.dtype == MESH_DTYPE and meshdata.flags["C_CONTIGUOUS"]
    keep = [(np.ascontiguousarray(t, LIGHT_TRI_DTYPE), np.ascontiguousarray(n, np.float32)) for t, n in parents]
    P = (LightParent * len(keep))()
    for k, (t, n) in enumerate(keep):
        P[k].tris, P[k].normals, P[k].n_tris = _ptr(t), _ptr(n), len(t)
    I = (LightInstance * len(instances))()
    for k, (par, mesh_index, l2w) in enumerate(instances):
        I[k].parent, I[k].mesh_index = par, mesh_index
        I[k].local_to_world[:] = unity_colmajor(np.asarray(l2w))
    total = sum(len(t) for t, _ in keep)
    nodes = np.zeros(2 * len(instances) + 2 * total, LIGHT_NODE_DTYPE)
    tris = np.zeros(total, LIGHT_TRI_DTYPE)
    meshes = np.zeros(len(instances), LIGHT_MESH_DTYPE)
    nn, nt = C.c_uint32(), C.c_uint32()
    _check(scene_lib().tt_lights_assemble(P, len(keep), I, len(instances), _ptr(meshdata), len(meshdata), _ptr(nodes),
                                          C.byref(nn), _ptr(tris), C.byref(nt), _ptr(meshes)), "tt_lights_assemble")
    return Lights(nodes[:nn.value].copy(), tris[:nt.value].copy(), meshes)


def emit_nee_host(lights: "Lights", scene, rays, n_rays, bounce, far_plane, width, height, frames=0, max_bounce=3,
                  frame_pixels=0, terrains=False, flags=0, check: bool = True):
    """tt_emit_nee_host: (samples [n_rays], shadow rays [n_shadow]) of the scalar reference of tt_emit_nee."""
    p = TraceParams(n_rays=n_rays, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height, flags=flags)
    smp = np.zeros(max(1, n_rays), LIGHT_SAMPLE_DTYPE)
    out = np.zeros(max(1, n_rays), SHADOW_DTYPE)
    n = C.c_uint32()
    st = scene_lib().tt_emit_nee_host(_ptr(lights.nodes), len(lights.nodes), _ptr(lights.tris), len(lights.tris),
                                      _ptr(lights.meshes), len(lights.meshes), _ptr(scene.tris), len(scene.tris),
                                      _ptr(scene.meshdata), len(scene.meshdata), C.byref(p), _ptr(rays), frames,
                                      max_bounce, frame_pixels, 1 if terrains else 0, _ptr(smp), _ptr(out), C.byref(n))
    if check:
        _check(st, "tt_emit_nee_host")
    return smp[:n_rays], out[:n.value].copy()


def light_transforms(local_to_world, solid_offsets) -> np.ndarray:
    """LIGHT_TRANSFORM_DTYPE rows of tt_lights_refit from row-major (math convention) 4x4 matrices, one per light
    mesh, and the LightNodeOffset of each light mesh's _MeshData record."""
    out = np.zeros(len(local_to_world), LIGHT_TRANSFORM_DTYPE)
    for k, m in enumerate(local_to_world):
        out["Transform"][k] = unity_colmajor(np.asarray(m))
    out["SolidOffset"] = np.asarray(solid_offsets, np.int32)
    return out


def lights_refit_host(lights: "Lights", scene, mesh_indices=(), transforms=None, flags=0, check: bool = True):
    """tt_lights_refit_host: the refitted copy of `lights` (nodes and tris new arrays; the input is not touched).
    check=False returns (status, reason, lights)."""
    out = Lights(lights.nodes.copy(), lights.tris.copy(), lights.meshes)
    mi = np.ascontiguousarray(mesh_indices, np.uint32)
    x = None if transforms is None else np.ascontiguousarray(transforms, LIGHT_TRANSFORM_DTYPE)
    why = C.create_string_buffer(512)
    st = scene_lib().tt_lights_refit_host(_ptr(out.nodes), len(out.nodes), _ptr(out.tris), len(out.tris), _ptr(out.meshes),
                                          len(out.meshes), _ptr(scene.tris), len(scene.tris), _ptr(scene.meshdata),
                                          len(scene.meshdata), _ptr(mi) if len(mi) else None, len(mi), _ptr(x),
                                          0 if x is None else len(x), flags, why, 512)
    if not check:
        return st, why.value.decode(), out
    _check(st, "tt_lights_refit_host: " + why.value.decode())
    return out


def light_refit_math(fn: str, x) -> np.ndarray:
    """tt_light_refit_math: the refit's pinned "asin" / "acos" / "sin" / "cos" over a float32 array."""
    xs = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(xs)
    _check(scene_lib().tt_light_refit_math(("asin", "acos", "sin", "cos").index(fn), _ptr(xs), xs.size, _ptr(out)),
           "tt_light_refit_math")
    return out


# ---------------------------------------------------------------- matrices
def trs_matrix(translation=(0, 0, 0), rotation_y_deg=0.0, scale=1.0) -> np.ndarray:
    """4x4 localToWorld (row-major numpy, math convention) of a rigid + uniform scale transform."""
    a = np.deg2rad(rotation_y_deg)
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4)
    m[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) * scale
    m[:3, 3] = translation
    return m


def unity_colmajor(m: np.ndarray) -> np.ndarray:
    """Unity stores Matrix4x4 column-major: element (r, c) at [c*4 + r]."""
    return np.asarray(m, dtype=np.float64).T.reshape(16).astype(np.float32)


def unity_camera(position, forward, up, vfov_deg, width, height, near=0.3, far=1000.0):
    """(cameraToWorldMatrix, projectionMatrix.inverse) as Unity computes them (OpenGL conventions:
    camera looks down -z in camera space)."""
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(np.asarray(up, np.float64), f)  # Unity is left-handed: right = up x forward
    r = r / np.linalg.norm(r)
    u = np.cross(f, r)
    l2w = np.eye(4)
    l2w[:3, 0], l2w[:3, 1], l2w[:3, 2], l2w[:3, 3] = r, u, f, position
    c2w = l2w @ np.diag([1.0, 1.0, -1.0, 1.0])
    aspect = width / height
    ft = 1.0 / np.tan(np.deg2rad(vfov_deg) / 2.0)
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = ft / aspect, ft
    P[2, 2], P[2, 3] = (far + near) / (near - far), 2 * far * near / (near - far)
    P[3, 2] = -1.0
    return c2w, np.linalg.inv(P)


# ---------------------------------------------------------------- scene building
class Mesh:
    """A ParentObject's merged object-space mesh (owned by the scene library)."""

    def __init__(self, handle: int):
        self.h = handle

    @staticmethod
    def _check(st, what):
        if st != TT_OK:
            raise TTError(st, what)

    @classmethod
    def cornell(cls) -> "Mesh":
        h = C.c_void_p()
        cls._check(scene_lib().tt_synth_cornell(C.byref(h)), "tt_synth_cornell")
        return cls(h.value)

    @classmethod
    def soup(cls, seed: int, n_tris: int, extent: float = 1.0, tri_size: float = 0.1) -> "Mesh":
        h = C.c_void_p()
        cls._check(scene_lib().tt_synth_soup(seed, n_tris, extent, tri_size, C.byref(h)), "tt_synth_soup")
        return cls(h.value)

    @classmethod
    def sponza(cls, seed: int = 0x53504F4E, n_tris: int = 262267) -> "Mesh":
        h = C.c_void_p()
        cls._check(scene_lib().tt_synth_sponza(seed, n_tris, C.byref(h)), "tt_synth_sponza")
        return cls(h.value)

    @classmethod
    def prop(cls, seed: int, n_tris: int) -> "Mesh":
        h = C.c_void_p()
        cls._check(scene_lib().tt_synth_prop(seed, n_tris, C.byref(h)), "tt_synth_prop")
        return cls(h.value)

    @classmethod
    def ground(cls, x0: float, x1: float, z0: float, z1: float, nu: int, nv: int) -> "Mesh":
        h = C.c_void_p()
        cls._check(scene_lib().tt_synth_ground(x0, x1, z0, z1, nu, nv, C.byref(h)), "tt_synth_ground")
        return cls(h.value)

    @classmethod
    def san_miguel(cls, seed: int = 0x5A4E4D, n_tris: int = 10_000_000) -> "Mesh":
        h = C.c_void_p()
        cls._check(scene_lib().tt_synth_san_miguel(seed, n_tris, C.byref(h)), "tt_synth_san_miguel")
        return cls(h.value)

    @classmethod
    def from_arrays(cls, positions: np.ndarray, indices: np.ndarray, matdat: Optional[np.ndarray] = None) -> "Mesh":
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1)
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
        md = None if matdat is None else np.ascontiguousarray(matdat, np.int32)
        h = scene_lib().tt_synth_mesh_from_arrays(pos.ctypes.data, pos.size // 3, idx.ctypes.data, idx.size,
                                                  None if md is None else md.ctypes.data)
        if not h:
            raise TTError(TT_ERR_OOM, "tt_synth_mesh_from_arrays")
        return cls(h)

    def arrays(self):
        """(positions (n,3), normals (n,3), indices (3*tris,)) copies of the mesh."""
        v = self.view()
        n, k = v.n_vertices, v.n_indices
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        pos = np.ctypeslib.as_array(C.cast(v.positions, fp), (3 * n,)).reshape(n, 3).copy()
        nrm = (np.ctypeslib.as_array(C.cast(v.normals, fp), (3 * n,)).reshape(n, 3).copy() if v.normals
               else np.tile(np.float32([0, 1, 0]), (n, 1)))
        idx = np.ctypeslib.as_array(C.cast(v.indices, ip), (k,)).copy()
        return pos, nrm, idx

    def view(self) -> MeshInput:
        v = MeshInput()
        self._check(scene_lib().tt_synth_mesh_view(self.h, C.byref(v)), "tt_synth_mesh_view")
        v._owner = self  # the view points into this mesh's native arrays: it keeps the mesh alive
        return v

    def __del__(self):
        if getattr(self, "h", None) and _SCENE is not None:
            _SCENE.tt_synth_mesh_free(self.h)
            self.h = None


class ArrayMesh:
    """A mesh over the caller's numpy arrays, every attribute tt_mesh_input names (normals, tangents, uvs and
    matdat are nullable). Usable wherever a Mesh is built from: Blas(mesh), Engine.build_object(mesh)."""

    def __init__(self, positions, indices, normals=None, tangents=None, uvs=None, matdat=None):
        def arr(a, dt, width):
            return None if a is None else np.ascontiguousarray(a, dt).reshape(-1, width)

        self.positions = arr(positions, np.float32, 3)
        self.indices = np.ascontiguousarray(indices, np.int32).reshape(-1)
        self.normals, self.tangents, self.uvs = arr(normals, np.float32, 3), arr(tangents, np.float32, 4), arr(uvs, np.float32, 2)
        self.matdat = None if matdat is None else np.ascontiguousarray(matdat, np.int32).reshape(-1)

    def view(self) -> MeshInput:
        v = MeshInput(positions=_ptr(self.positions), n_vertices=len(self.positions), normals=_ptr(self.normals),
                      tangents=_ptr(self.tangents), uvs=_ptr(self.uvs), indices=_ptr(self.indices),
                      n_indices=self.indices.size, matdat=_ptr(self.matdat))
        v.lossy_scale[:] = (1.0, 1.0, 1.0)
        v._owner = self  # the view points into this object's arrays
        return v


_BUILD_ENGINE = None
_BUILD_MIN_TRIS = 0


def set_build_engine(engine: "Engine" = None, min_tris: int = 100_000):
    """Route every later Blas(mesh) of at least ``min_tris`` triangles through ``engine``'s GPU
    (tt_blas_build_device; byte-identical to the host build). None: host builds again."""
    global _BUILD_ENGINE, _BUILD_MIN_TRIS
    _BUILD_ENGINE, _BUILD_MIN_TRIS = engine, int(min_tris)


class Blas:
    """A built ParentObject: CWBVH8 nodes + leaf-ordered CudaTriangles (ParentObject.BuildTotal)."""

    def __init__(self, mesh: Mesh, lossy_scale=(1.0, 1.0, 1.0), engine: "Engine" = None, timings: dict = None,
                 device_stages: str = "bvh2+bvh8"):
        """engine: build on that engine's GPU after the host's presort -- device_stages "bvh2+bvh8"
        (tt_blas_build_device) or "bvh2" (tt_bvh2_build_device, BVH8 on the host); either way the
        result is byte-identical to the host build. timings (dict): the stage times in seconds."""
        v = mesh.view()
        v.lossy_scale[:] = lossy_scale
        h = C.c_void_p()
        L = scene_lib()
        if engine is None and _BUILD_ENGINE is not None and v.n_indices // 3 >= _BUILD_MIN_TRIS:
            engine = _BUILD_ENGINE
        if engine is None:
            st = L.tt_blas_build(C.byref(v), C.byref(h))
            if st != TT_OK:
                raise TTError(st, "tt_blas_build")
        else:
            import time
            t0 = time.perf_counter()
            n = v.n_indices // 3
            aabbs = np.zeros((n, 6), np.float32)
            prep = C.c_void_p()  # the prepared triangles, kept for the final assembly (bvh2+bvh8)
            if device_stages == "bvh2+bvh8":
                _check(L.tt_blas_prepare(C.byref(v), aabbs.ctypes.data, C.byref(prep)), "tt_blas_prepare")
            else:
                _check(L.tt_blas_prepare_aabbs(C.byref(v), aabbs.ctypes.data), "tt_blas_prepare_aabbs")
            t1 = time.perf_counter()
            pre = np.zeros((3, n), np.int32)
            if engine.L.tt_bvh2_presort_device(engine.h, aabbs.ctypes.data, n, pre.ctypes.data) != TT_OK:
                st = L.tt_bvh2_presort(aabbs.ctypes.data, n, pre.ctypes.data)
                if st != TT_OK:
                    if prep:
                        L.tt_blas_prep_free(prep)
                    raise TTError(st, "tt_bvh2_presort")
            t2 = time.perf_counter()
            if device_stages == "bvh2+bvh8":
                cap = max(1, n - 1)
                nodes = np.zeros(cap, NODE_DTYPE)
                cw = np.zeros(n, np.int32)
                nn, depth = C.c_uint32(0), C.c_uint32(0)
                st = engine.L.tt_blas_build_device(engine.h, aabbs.ctypes.data, n, pre.ctypes.data, nodes.ctypes.data,
                                                   cap, C.byref(nn), cw.ctypes.data, C.byref(depth))
                if st != TT_OK:
                    L.tt_blas_prep_free(prep)
                    raise TTError(st, "tt_blas_build_device")
                t3 = time.perf_counter()
                _check(L.tt_blas_build_from_cwbvh_prepared(prep, nodes.ctypes.data, nn.value, cw.ctypes.data,
                                                           depth.value, C.byref(h)),
                       "tt_blas_build_from_cwbvh_prepared")  # consumes prep
                if timings is not None:
                    timings.update(prepare_s=t1 - t0, presort_s=t2 - t1, device_s=t3 - t2,
                                   assemble_s=time.perf_counter() - t3)
                self.h = h.value
                info = BlasInfo()
                L.tt_blas_get_info(self.h, C.byref(info))
                self.info = info
                return
            fi = np.zeros(n, np.int32)
            boxes = np.zeros((2 * n, 6), np.float32)
            left = np.zeros(2 * n, np.int32)
            count = np.zeros(2 * n, np.uint32)
            depth = C.c_uint32(0)
            st = engine.L.tt_bvh2_build_device(engine.h, aabbs.ctypes.data, n, pre.ctypes.data, fi.ctypes.data,
                                               boxes.ctypes.data, left.ctypes.data, count.ctypes.data, C.byref(depth))
            if st != TT_OK:
                raise TTError(st, "tt_bvh2_build_device")
            t3 = time.perf_counter()
            _check(L.tt_blas_build_from_bvh2(C.byref(v), fi.ctypes.data, boxes.ctypes.data, left.ctypes.data,
                                             count.ctypes.data, depth.value, C.byref(h)), "tt_blas_build_from_bvh2")
            if timings is not None:
                timings.update(prepare_s=t1 - t0, presort_s=t2 - t1, bvh2_device_s=t3 - t2,
                               bvh8_s=time.perf_counter() - t3)
        self.h = h.value
        info = BlasInfo()
        L.tt_blas_get_info(self.h, C.byref(info))
        self.info = info

    @property
    def n_nodes(self):
        return self.info.n_nodes

    @property
    def n_tris(self):
        return self.info.n_tris

    def leaf_order(self) -> np.ndarray:
        """CWBVHIndicesBufferInverted: source triangle -> position in the leaf-ordered triangles."""
        out = np.zeros(self.info.n_tris, np.int32)
        scene_lib().tt_blas_copy_leaf_order(self.h, out.ctypes.data)
        return out

    def arrays(self):
        nodes = np.zeros(self.info.n_nodes, NODE_DTYPE)
        tris = np.zeros(self.info.n_tris, TRI_DTYPE)
        scene_lib().tt_blas_copy(self.h, nodes.ctypes.data, tris.ctypes.data)
        return nodes, tris

    def __del__(self):
        if getattr(self, "h", None) and _SCENE is not None:
            _SCENE.tt_blas_free(self.h)
            self.h = None


@dataclass
class Scene:
    """Aggregated trace buffers exactly as AssetManager.SetMeshTraceBuffers binds them."""
    nodes: np.ndarray
    tris: np.ndarray
    tlas: np.ndarray
    meshdata: np.ndarray
    materials: np.ndarray
    tlas_nodes: int = 0
    meta: dict = field(default_factory=dict)
    alpha_atlas: Optional[np.ndarray] = None  # _AlphaAtlas, uint8 [height, width] (Cutout materials)
    texture_atlas: Optional[np.ndarray] = None  # _TextureAtlas decoded, float16 [height, width, 4] (glass)

    def save(self, path: str):
        np.savez_compressed(path, nodes=self.nodes.view(np.uint8), tris=self.tris.view(np.uint8),
                            tlas=self.tlas, meshdata=self.meshdata.view(np.uint8),
                            materials=self.materials.view(np.uint8), tlas_nodes=np.int64(self.tlas_nodes))

    @classmethod
    def load(cls, path: str) -> "Scene":
        z = np.load(path, allow_pickle=False)
        return cls(nodes=z["nodes"].view(NODE_DTYPE).copy(), tris=z["tris"].view(TRI_DTYPE).copy(),
                   tlas=z["tlas"].astype(np.int32), meshdata=z["meshdata"].view(MESH_DTYPE).copy(),
                   materials=z["materials"].view(MAT_DTYPE).copy(), tlas_nodes=int(z["tlas_nodes"]))


class AssetManager:
    """Host mirror of the reference AssetManager's aggregation (AccumulateData + UpdateTLAS +
    ConstructNewTLAS): RenderQue parents, InstanceData parents and InstancedObjects."""

    def __init__(self):
        self.parents: List = []          # (Blas, l2w 4x4, material_count)
        self.instance_parents: List = []  # (Blas, material_count)
        self.instances: List = []        # (instance_parent index, l2w 4x4)
        self.materials: List[np.ndarray] = []

    def add_parent(self, blas: Blas, local_to_world=None, materials: Optional[np.ndarray] = None):
        mats = materials if materials is not None else np.zeros(1, MAT_DTYPE)
        self.parents.append((blas, np.eye(4) if local_to_world is None else np.asarray(local_to_world), len(mats)))
        self.materials.append(mats)

    def add_instance_parent(self, blas: Blas, materials: Optional[np.ndarray] = None) -> int:
        mats = materials if materials is not None else np.zeros(1, MAT_DTYPE)
        self.instance_parents.append((blas, len(mats)))
        self._ip_mats = getattr(self, "_ip_mats", [])
        self._ip_mats.append(mats)
        return len(self.instance_parents) - 1

    def add_instance(self, parent_index: int, local_to_world):
        self.instances.append((parent_index, np.asarray(local_to_world)))

    def add_parent_object(self, obj: "SceneObject", local_to_world=None, materials: Optional[np.ndarray] = None):
        """add_parent for a device-built object (Engine.build_object): assemble_objects places it by its summary."""
        assert obj.build_info is not None, "add_parent_object takes an object of Engine.build_object"
        self.add_parent(obj, local_to_world, materials)

    def add_instance_parent_object(self, obj: "SceneObject", materials: Optional[np.ndarray] = None) -> int:
        assert obj.build_info is not None, "add_instance_parent_object takes an object of Engine.build_object"
        return self.add_instance_parent(obj, materials)

    def _instance_descs(self):
        I = (InstanceDesc * max(1, len(self.instances)))()
        for i, (pi, l2w) in enumerate(self.instances):
            I[i].instance_parent = pi
            I[i].local_to_world[:] = unity_colmajor(l2w)
            I[i].world_to_local[:] = unity_colmajor(np.linalg.inv(l2w))
        return I

    def assemble_objects(self, engine: "Engine"):
        """The scene-change path with no host BLAS anywhere: every parent is a device-built object
        (add_parent_object / add_instance_parent_object), the TLAS side comes from their summaries
        (tt_scene_assemble_tlas) and the BLAS side is gathered on the device (Engine.assemble). Returns
        (Scene, objects); the Scene holds the TLAS-region nodes and no triangles, its meta the layout's totals."""
        def desc(obj, l2w, nm, d):
            bi = obj.build_info
            d.n_nodes, d.n_tris = bi.n_nodes, bi.n_tris
            d.aabb_min[:], d.aabb_max[:] = bi.aabb_min[:], bi.aabb_max[:]
            d.local_to_world[:] = unity_colmajor(l2w)
            d.world_to_local[:] = unity_colmajor(np.linalg.inv(l2w))
            d.material_count = nm

        P = (ObjectDesc * max(1, len(self.parents)))()
        for i, (o, l2w, nm) in enumerate(self.parents):
            desc(o, l2w, nm, P[i])
        IP = (ObjectDesc * max(1, len(self.instance_parents)))()
        for i, (o, nm) in enumerate(self.instance_parents):
            desc(o, np.eye(4), nm, IP[i])
        I = self._instance_descs()
        h = C.c_void_p()
        L = scene_lib()
        _check(L.tt_scene_assemble_tlas(C.addressof(P), len(self.parents), C.addressof(IP), len(self.instance_parents),
                                        C.addressof(I), len(self.instances), C.byref(h)), "tt_scene_assemble_tlas")
        try:
            info = SceneBuildInfo()
            L.tt_scene_build_get_info(h, C.byref(info))
            nodes = np.zeros(info.n_nodes, NODE_DTYPE)
            tlas = np.zeros(info.n_tlas_indices, np.int32)
            md = np.zeros(info.n_mesh, MESH_DTYPE)
            L.tt_scene_build_copy(h, nodes.ctypes.data, None, tlas.ctypes.data, md.ctypes.data)
            aabbs = np.zeros((info.n_mesh, 6), np.float32)
            L.tt_scene_build_copy_mesh_aabbs(h, aabbs.ctypes.data)
            tn, tt = C.c_uint32(), C.c_uint32()
            L.tt_scene_build_get_totals(h, C.byref(tn), C.byref(tt))
        finally:
            L.tt_scene_build_free(h)
        mats = self.materials + getattr(self, "_ip_mats", [])
        materials = np.concatenate(mats) if mats else np.zeros(1, MAT_DTYPE)
        objects = self.blases()
        engine.assemble(objects, nodes, tlas, md, materials)
        s = Scene(nodes, np.zeros(0, TRI_DTYPE), tlas, md, materials, tlas_nodes=info.tlas_nodes,
                  meta={"mesh_aabbs": aabbs, "n_nodes_total": int(tn.value), "n_tris_total": int(tt.value)})
        return s, objects

    def build(self) -> Scene:
        if not all(isinstance(p[0], Blas) for p in self.parents + self.instance_parents):
            raise TypeError("AssetManager.build needs host BLASes; device-built objects go through assemble_objects")
        P = (ParentDesc * max(1, len(self.parents)))()
        for i, (b, l2w, nm) in enumerate(self.parents):
            P[i].blas = b.h
            P[i].local_to_world[:] = unity_colmajor(l2w)
            P[i].world_to_local[:] = unity_colmajor(np.linalg.inv(l2w))
            P[i].material_count = nm
        IP = (ParentDesc * max(1, len(self.instance_parents)))()
        for i, (b, nm) in enumerate(self.instance_parents):
            IP[i].blas = b.h
            IP[i].local_to_world[:] = unity_colmajor(np.eye(4))
            IP[i].world_to_local[:] = unity_colmajor(np.eye(4))
            IP[i].material_count = nm
        I = self._instance_descs()
        h = C.c_void_p()
        L = scene_lib()
        st = L.tt_scene_assemble(C.addressof(P), len(self.parents), C.addressof(IP), len(self.instance_parents),
                                 C.addressof(I), len(self.instances), C.byref(h))
        if st != TT_OK:
            raise TTError(st, "tt_scene_assemble")
        try:
            info = SceneBuildInfo()
            L.tt_scene_build_get_info(h, C.byref(info))
            nodes = np.zeros(info.n_nodes, NODE_DTYPE)
            tris = np.zeros(info.n_tris, TRI_DTYPE)
            tlas = np.zeros(info.n_tlas_indices, np.int32)
            md = np.zeros(info.n_mesh, MESH_DTYPE)
            L.tt_scene_build_copy(h, nodes.ctypes.data, tris.ctypes.data, tlas.ctypes.data, md.ctypes.data)
            aabbs = np.zeros((info.n_mesh, 6), np.float32)
            L.tt_scene_build_copy_mesh_aabbs(h, aabbs.ctypes.data)
        finally:
            L.tt_scene_build_free(h)
        mats = self.materials + getattr(self, "_ip_mats", [])
        materials = np.concatenate(mats) if mats else np.zeros(1, MAT_DTYPE)
        return Scene(nodes, tris, tlas, md, materials, tlas_nodes=info.tlas_nodes, meta={"mesh_aabbs": aabbs})

    def blases(self) -> List:
        """The BLASes in layout order (AccumulateData): RenderQue parents, then InstanceData parents."""
        return [p[0] for p in self.parents] + [p[0] for p in self.instance_parents]

    def assemble(self, engine: "Engine", objects=None):
        """The scene-change path: the TLAS side is built on the host as build() does, the BLAS side is gathered on
        the device from one GPU-resident object per BLAS (`objects` in blases() order; created here when None).
        Returns (Scene, objects): the host Scene is what tt_scene_upload would have taken."""
        s = self.build()
        if objects is None:
            objects = [engine.create_object(b) for b in self.blases()]
        region = 2 * len(s.meshdata)  # AssetManager.cs:995: the TLAS region in front of the first object
        engine.assemble(objects, s.nodes[:region], s.tlas, s.meshdata, s.materials)
        return s, objects


def tlas_build(mesh_aabbs) -> Tuple[np.ndarray, np.ndarray]:
    """tt_tlas_build (host): the TLAS over per-mesh world AABBs (n_mesh x {BBMax, BBMin}) as ConstructNewTLAS /
    CorrectRefit build it. Returns (nodes[:n_tlas_nodes], TLASBVH8Indices); raises TTError(TT_ERR_UNSUPPORTED)
    where the reference's BVH8Builder fails."""
    a = np.ascontiguousarray(mesh_aabbs, np.float32).reshape(-1, 6)
    n = a.shape[0]
    nodes = np.zeros(2 * n, NODE_DTYPE)
    idx = np.zeros(n, np.int32)
    cnt = C.c_uint32()
    _check(scene_lib().tt_tlas_build(a.ctypes.data, n, nodes.ctypes.data, C.byref(cnt), idx.ctypes.data), "tt_tlas_build")
    return nodes[: cnt.value].copy(), idx


def single_object_scene(mesh: Mesh, local_to_world=None, n_materials: int = 8) -> Scene:
    am = AssetManager()
    am.add_parent(Blas(mesh), local_to_world, np.zeros(n_materials, MAT_DTYPE))
    return am.build()


# ---------------------------------------------------------------- ray buffers
def camera_rays_host(cam_to_world: np.ndarray, cam_inv_proj: np.ndarray, width: int, height: int,
                     near: float, far: float) -> np.ndarray:
    """Vectorised float32 restatement of Generate for tests without a GPU (pinned like the
    kernel up to normalize's rounding; parity tests use rays from one source on both sides)."""
    c2w = unity_colmajor(cam_to_world).reshape(4, 4).T.astype(np.float32)
    ip = unity_colmajor(cam_inv_proj).reshape(4, 4).T.astype(np.float32)
    ys, xs = np.meshgrid(np.arange(height, dtype=np.float32), np.arange(width, dtype=np.float32), indexing="ij")
    uvx = xs / np.float32(width) * np.float32(2) - np.float32(1)
    uvy = ys / np.float32(height) * np.float32(2) - np.float32(1)
    d = np.stack([ip[r, 0] * uvx + ip[r, 1] * uvy + ip[r, 3] for r in range(3)], -1).astype(np.float32)
    d = np.stack([c2w[r, 0] * d[..., 0] + c2w[r, 1] * d[..., 1] + c2w[r, 2] * d[..., 2] for r in range(3)], -1)
    d = (d / np.sqrt((d * d).sum(-1, keepdims=True))).astype(np.float32)
    o = c2w[:3, 3].astype(np.float32)
    rays = np.zeros(2 * width * height, RAY_DTYPE)
    prim = rays[: width * height]
    prim["origin"] = (o + np.float32(near) * d).reshape(-1, 3)
    prim["direction"] = d.reshape(-1, 3)
    prim["PixelIndex"] = np.arange(width * height, dtype=np.uint32)
    prim["hits"][:, 2] = np.array([far], np.float32).view(np.uint32)[0]
    return rays


# ---------------------------------------------------------------- engine
def tlas_root_form(node0) -> int:
    """tt_tlas_root_form of one 80-byte node (any contiguous array holding node 0 first); needs no device."""
    f = C.c_uint32()
    st = hip_lib().tt_tlas_root_form(_ptr(node0), C.byref(f))
    if st != TT_OK:
        raise TTError(st, "tt_tlas_root_form")
    return int(f.value)


def plan_build_batches(n_tris, budget: int):
    """How Engine.build_objects splits a mesh list into tt_objects_build_device calls: consecutive runs [lo, hi) of
    the list, in order, each holding as many meshes as fit `budget` triangles; a mesh above the budget goes alone.
    A pure function of the triangle counts."""
    if budget < 1:
        raise ValueError("the triangle budget must be positive")
    runs, lo, held = [], 0, 0
    for k, n in enumerate(n_tris):
        if k > lo and held + n > budget:
            runs.append((lo, k))
            lo, held = k, 0
        held += n
    if lo < len(n_tris):
        runs.append((lo, len(n_tris)))
    return runs


class SceneObject:
    """tt_object: one BLAS resident on a device (Engine.create_object). An assembly copies it, so it may be
    destroyed as soon as Engine.assemble has returned."""

    def __init__(self, L, handle: int, build_info: "ObjectBuildInfo" = None, engine: "Engine" = None):
        self.L, self.h = L, handle
        self.build_info = build_info  # tt_object_build_info of Engine.build_object, None for create_object
        self._engine = engine

    def read(self, engine: "Engine" = None):
        """tt_object_read: (nodes, tris, leaf_of_triangle) copied back from the device. An object of create_object
        has no leaf order: (nodes, tris, None)."""
        eng = engine or self._engine
        info = self.info
        nodes, tris = np.zeros(info.n_nodes, NODE_DTYPE), np.zeros(info.n_tris, TRI_DTYPE)
        leaf = np.zeros(info.n_tris, np.int32) if self.build_info is not None else None
        eng._check(self.L.tt_object_read(eng.h, self.h, _ptr(nodes), _ptr(tris), _ptr(leaf)), "tt_object_read")
        return nodes, tris, leaf

    @property
    def leaf_order_device(self) -> int:
        """tt_object_leaf_order_device: the device address of leaf_of_triangle (n_tris int32), owned by the object;
        what Engine.blas_refit(..., device=True) takes."""
        p = C.c_void_p()
        _check(self.L.tt_object_leaf_order_device(self.h, C.byref(p)), "tt_object_leaf_order_device")
        return p.value

    @property
    def info(self) -> ObjectInfo:
        info = ObjectInfo()
        _check(self.L.tt_object_get_info(self.h, C.byref(info)), "tt_object_get_info")
        return info

    def destroy(self):
        if getattr(self, "h", None):
            self.L.tt_object_destroy(self.h)
            self.h = None

    __del__ = destroy


def _object_handles(objects):
    """A C array of tt_object* from SceneObjects (None -> NULL)."""
    return (C.c_void_p * max(1, len(objects)))(*[o.h if o is not None else None for o in objects])


class RefitPart:
    """One renderer of a deforming mesh (tt_blas_refit_part): `vertices` n x stride floats (position at +0, normal
    at +3), `indices` 3 per triangle local to it, `first_tri` its place among the mesh's source triangles,
    `transform` a row-major 4x4 (identity by default). Arrays are numpy arrays or device tensors."""

    def __init__(self, vertices, indices, first_tri: int = 0, transform=None, n_vertices=None, vertex_stride=None,
                 n_tris=None):
        two_d = hasattr(vertices, "shape") and len(vertices.shape) == 2
        self.vertices, self.indices, self.first_tri = vertices, indices, int(first_tri)
        self.n_vertices = int(n_vertices if n_vertices is not None else vertices.shape[0] if two_d else 0)
        self.vertex_stride = int(vertex_stride if vertex_stride is not None else vertices.shape[1] if two_d else 6)
        if n_tris is None:
            shape = getattr(indices, "shape", None)
            n_tris = 0 if not shape else int(shape[0]) // 3 if len(shape) == 1 else int(shape[0])
        self.n_tris = int(n_tris)
        self.transform = np.eye(4) if transform is None else np.asarray(transform)


class RefitItem:
    """One deforming mesh (tt_blas_refit_item): its _MeshData record, its BLAS's triangle count, leaf_of_triangle
    (Blas.leaf_order() or an object's leaf_order_device), its parts and, optionally, the row-major local_to_world
    whose world box goes to mesh_aabbs[mesh_index]."""

    def __init__(self, mesh_index: int, n_tris: int, leaf_of_triangle, parts, local_to_world=None):
        self.mesh_index, self.n_tris, self.leaf_of_triangle = int(mesh_index), int(n_tris), leaf_of_triangle
        self.parts, self.local_to_world = list(parts), local_to_world


def refit_item_array(items):
    """(ctypes array of tt_blas_refit_item, the objects that must outlive the call)."""
    arr = (BlasRefitItem * max(1, len(items)))()
    keep = []
    for i, it in enumerate(items):
        parts = (BlasRefitPart * max(1, len(it.parts)))()
        for k, p in enumerate(it.parts):
            parts[k].vertices, parts[k].indices = _ptr(p.vertices), _ptr(p.indices)
            parts[k].n_vertices, parts[k].vertex_stride = p.n_vertices, p.vertex_stride
            parts[k].n_tris, parts[k].first_tri = p.n_tris, p.first_tri
            parts[k].transform[:] = unity_colmajor(p.transform)
        arr[i].mesh_index, arr[i].n_tris = it.mesh_index, it.n_tris
        arr[i].leaf_of_triangle = _ptr(it.leaf_of_triangle)
        arr[i].parts = parts if it.parts else None
        arr[i].n_parts = len(it.parts)
        if it.local_to_world is not None:
            m = np.ascontiguousarray(unity_colmajor(np.asarray(it.local_to_world)), np.float32)
            arr[i].local_to_world = m.ctypes.data
            keep.append(m)
        keep.append(parts)
    return arr, keep


def blas_refit_items_validate(items, meshdata: np.ndarray, n_scene_tris: int, device: bool = False):
    """tt_blas_refit_items_validate (host only): (status, first violation) of an item list against a scene's
    _MeshData records and triangle count."""
    arr, keep = refit_item_array(items)
    md = np.ascontiguousarray(meshdata, MESH_DTYPE)
    why = C.create_string_buffer(256)
    st = hip_lib().tt_blas_refit_items_validate(arr if items else None, len(items), _ptr(md), len(md), int(n_scene_tris),
                                                TT_TRACE_DEVICE_PTRS if device else 0, why, 256)
    del keep
    return st, why.value.decode()


def object_validate(nodes: np.ndarray, tris: np.ndarray, root: int = 0):
    """tt_object_validate (host only): (status, first violation) of one BLAS's arrays against its own counts."""
    nodes, tris = np.ascontiguousarray(nodes, NODE_DTYPE), np.ascontiguousarray(tris, TRI_DTYPE)
    why = C.create_string_buffer(256)
    st = hip_lib().tt_object_validate(_ptr(nodes), len(nodes), _ptr(tris), len(tris), int(root), why, 256)
    return st, why.value.decode()


def scene_layout(objects, tlas_region: int):
    """tt_scene_layout_objects / _counts: AccumulateData's running sums over SceneObjects, or over plain
    (n_nodes, n_tris) pairs (host only). Returns (node_offsets, tri_offsets, n_nodes_total, n_tris_total)."""
    L = hip_lib()
    n = len(objects)
    no, to = np.zeros(max(1, n), np.uint32), np.zeros(max(1, n), np.uint32)
    tn, tt = C.c_uint32(), C.c_uint32()
    if n and all(isinstance(o, SceneObject) for o in objects):
        st = L.tt_scene_layout_objects(_object_handles(objects), n, int(tlas_region), _ptr(no), _ptr(to), C.byref(tn),
                                       C.byref(tt))
        _check(st, "tt_scene_layout_objects")
    else:
        cn = np.ascontiguousarray([o[0] for o in objects], np.uint32)
        ct = np.ascontiguousarray([o[1] for o in objects], np.uint32)
        st = L.tt_scene_layout_counts(_ptr(cn), _ptr(ct), n, int(tlas_region), _ptr(no), _ptr(to), C.byref(tn), C.byref(tt))
        _check(st, "tt_scene_layout_counts")
    return no[:n].copy(), to[:n].copy(), int(tn.value), int(tt.value)


class Engine:
    """One context per GPU (tt_ctx_create). ``trace`` is the kernel_trace dispatch."""

    def __init__(self, device: int = 0, max_rays: int = 0, stream: Optional[int] = None):
        L = hip_lib()
        cfg = Config(device=device, flags=0, max_rays=max_rays, stream=stream)
        h = C.c_void_p()
        st = L.tt_ctx_create(C.byref(cfg), C.byref(h))
        if st != TT_OK:
            raise TTError(st, "tt_ctx_create (no GPU visible?)")
        self.L, self.h = L, h.value
        _ENGINES.add(self)

    def _check(self, st, what):
        if st != TT_OK:
            raise TTError(st, f"{what}: {self.L.tt_last_error(self.h).decode()}")

    def _unlink_lender(self):
        """Drops this engine from its lender's borrower list (re-share or close)."""
        lender = getattr(self, "_lender", None)
        if lender is not None:
            lender._borrowers = [r for r in getattr(lender, "_borrowers", []) if r() is not None and r() is not self]
        self._lender = None

    def close(self):
        if getattr(self, "h", None):
            for b in list(getattr(self, "_borrowers", [])):  # contexts tracing this one's scene go first
                e = b()
                if e is not None:
                    e.close()
            self._borrowers = []
            self._unlink_lender()
            self.L.tt_ctx_destroy(self.h)
            self.h = None

    def share_scene(self, src: "Engine"):
        """tt_ctx_share_scene: trace `src`'s scene (its device buffers, no copy) on this context's stream."""
        import weakref

        self._check(self.L.tt_ctx_share_scene(self.h, src.h), "tt_ctx_share_scene")
        self._unlink_lender()  # a re-share leaves the previous lender's list
        self._lender = src  # keeps the lender alive while this context reads its buffers
        if not hasattr(src, "_borrowers"):
            src._borrowers = []
        src._borrowers.append(weakref.ref(self))

    def chunk_costs(self, bounce: int = 0, max_chunks: int = 1 << 22) -> np.ndarray:
        """tt_trace_chunk_costs: the last TT_TRACE_ADAPTIVE_ORDER launch's per-64-ray-chunk costs (max Reps;
        full-frame launches: one per 8x8 pixel tile, row-major over the (W/8) x (H/8) tile grid)."""
        out = np.zeros(max_chunks, np.uint32)
        n = C.c_uint32()
        self._check(self.L.tt_trace_chunk_costs(self.h, int(bounce), out.ctypes.data, max_chunks, C.byref(n)),
                    "tt_trace_chunk_costs")
        return out[: n.value].copy()

    def share_blas(self, src: "Engine", n_tlas_nodes: int):
        """tt_ctx_share_blas: a frame slot over `src`'s scene -- src's BLASes and triangles (no copy) under a TLAS,
        TLASBVH8Indices and _MeshData of this context's own (copied from src now), which tlas_refit /
        update_meshdata / update_nodes on this context change without waiting for src or other slots."""
        import weakref

        self._check(self.L.tt_ctx_share_blas(self.h, src.h, int(n_tlas_nodes)), "tt_ctx_share_blas")
        self._unlink_lender()
        self._lender = src
        if not hasattr(src, "_borrowers"):
            src._borrowers = []
        src._borrowers.append(weakref.ref(self))

    __del__ = close

    @property
    def stream(self) -> int:
        return self.L.tt_ctx_stream(self.h)

    def upload(self, s: Scene):
        """AssetManager.SetMeshTraceBuffers — copies the aggregated buffers into HBM."""
        st = self.L.tt_scene_upload(self.h, _ptr(s.nodes), len(s.nodes), _ptr(s.tris), len(s.tris), _ptr(s.tlas),
                                    len(s.tlas), _ptr(s.meshdata), len(s.meshdata), _ptr(s.materials),
                                    len(s.materials))
        self._check(st, "tt_scene_upload")
        if s.alpha_atlas is not None:
            self.upload_alpha_atlas(s.alpha_atlas)
        if s.texture_atlas is not None:
            self.upload_texture_atlas(s.texture_atlas)

    def create_object(self, blas_or_arrays, root: int = 0) -> "SceneObject":
        """tt_object_create: one BLAS (a Blas, or its (nodes, tris) arrays with BLAS-local indices) resident on this
        engine's device. The handle belongs to the device: any engine there may assemble it."""
        nodes, tris = blas_or_arrays.arrays() if isinstance(blas_or_arrays, Blas) else blas_or_arrays
        nodes, tris = np.ascontiguousarray(nodes, NODE_DTYPE), np.ascontiguousarray(tris, TRI_DTYPE)
        h = C.c_void_p()
        self._check(self.L.tt_object_create(self.h, _ptr(nodes), len(nodes), _ptr(tris), len(tris), int(root),
                                            C.byref(h)), "tt_object_create")
        return SceneObject(self.L, h.value)

    def build_object(self, mesh, lossy_scale=(1.0, 1.0, 1.0), device_arrays: dict = None) -> "SceneObject":
        """tt_object_build_device: `mesh` (a Mesh or ArrayMesh) built into an object on this engine's device, byte
        for byte the object create_object(Blas(mesh)) would be, without a host triangle record. device_arrays: device
        tensors (positions, normals, tangents, uvs, indices, matdat) replacing ALL of the mesh's arrays, passed with
        TT_TRACE_DEVICE_PTRS (`mesh` then only supplies the counts and the host presort's input). Where the device
        presort declines (TT_ERR_UNSUPPORTED: n <= 16, non-finite centroids), the host presort is used instead, as
        Blas(mesh, engine=...) does."""
        v = mesh.view()
        v.lossy_scale[:] = lossy_scale
        host = MeshInput.from_buffer_copy(v)  # the host arrays, for the retry's boxes
        flags = 0
        if device_arrays is not None:
            flags = TT_TRACE_DEVICE_PTRS
            for k in ("positions", "normals", "tangents", "uvs", "indices", "matdat"):
                setattr(v, k, _ptr(device_arrays.get(k)))
        h, info = C.c_void_p(), ObjectBuildInfo()
        st = self.L.tt_object_build_device(self.h, C.byref(v), None, flags, C.byref(h), C.byref(info))
        if st == TT_ERR_UNSUPPORTED:
            S = scene_lib()
            n = v.n_indices // 3
            aabbs, pre = np.zeros((n, 6), np.float32), np.zeros((3, n), np.int32)
            _check(S.tt_blas_prepare_aabbs(C.byref(host), aabbs.ctypes.data), "tt_blas_prepare_aabbs")
            _check(S.tt_bvh2_presort(aabbs.ctypes.data, n, pre.ctypes.data), "tt_bvh2_presort")
            st = self.L.tt_object_build_device(self.h, C.byref(v), pre.ctypes.data, flags, C.byref(h), C.byref(info))
        self._check(st, "tt_object_build_device")
        return SceneObject(self.L, h.value, build_info=info, engine=self)

    def build_objects_raw(self, views, presorted=None, flags: int = 0):
        """tt_objects_build_device as it stands: `views` a list of MeshInput, `presorted` None or a list of (3, n)
        int32 arrays / None per mesh. Returns (status, handles, infos, mesh_status): handles a list of ints / None."""
        M = len(views)
        arr = (MeshInput * max(1, M))(*views)
        lists = (C.c_void_p * max(1, M))()
        keep = []
        if presorted is not None:
            for m, p in enumerate(presorted):
                if p is not None:
                    keep.append(np.ascontiguousarray(p, np.int32))
                    lists[m] = keep[-1].ctypes.data
        out = (C.c_void_p * max(1, M))()
        infos = (ObjectBuildInfo * max(1, M))()
        status = (C.c_int32 * max(1, M))()
        st = self.L.tt_objects_build_device(self.h, arr, M, lists if presorted is not None else None, int(flags), out,
                                            infos, status)
        return st, [out[m] for m in range(M)], [infos[m] for m in range(M)], [status[m] for m in range(M)]

    def build_objects(self, meshes, lossy_scales=None, max_tris_per_call: int = 10_000_000):
        """tt_objects_build_device: every mesh of `meshes` (Mesh or ArrayMesh) built into an object of its own, each
        byte for byte what build_object makes of it, in as few calls as the triangle budget allows
        (plan_build_batches). Meshes the device presort declines (mesh_status TT_ERR_UNSUPPORTED: non-finite
        centroids, a depth-exhausted partition too large) are retried with host presorts, the others' staying on the
        device. Returns the SceneObjects in the order of `meshes`."""
        meshes = list(meshes)
        views = []
        for k, mesh in enumerate(meshes):
            v = mesh.view()
            v.lossy_scale[:] = (1.0, 1.0, 1.0) if lossy_scales is None else lossy_scales[k]
            views.append(v)
        objects = []
        try:
            for lo, hi in plan_build_batches([v.n_indices // 3 for v in views], max_tris_per_call):
                vs = views[lo:hi]
                st, hs, infos, status = self.build_objects_raw(vs)
                if st == TT_ERR_UNSUPPORTED:
                    S = scene_lib()
                    pre = [None] * len(vs)
                    for m, v in enumerate(vs):
                        if status[m] != TT_ERR_UNSUPPORTED:
                            continue
                        n = v.n_indices // 3
                        aabbs, pre[m] = np.zeros((n, 6), np.float32), np.zeros((3, n), np.int32)
                        _check(S.tt_blas_prepare_aabbs(C.byref(v), aabbs.ctypes.data), "tt_blas_prepare_aabbs")
                        _check(S.tt_bvh2_presort(aabbs.ctypes.data, n, pre[m].ctypes.data), "tt_bvh2_presort")
                    st, hs, infos, status = self.build_objects_raw(vs, pre)
                self._check(st, "tt_objects_build_device")
                objects += [SceneObject(self.L, h, build_info=ObjectBuildInfo.from_buffer_copy(i), engine=self)
                            for h, i in zip(hs, infos)]
        except Exception:
            for o in objects:
                o.destroy()
            raise
        return objects

    def assemble(self, objects, tlas_nodes: np.ndarray, tlas: np.ndarray, meshdata: np.ndarray, materials: np.ndarray):
        """tt_scene_assemble_objects: the scene tt_scene_upload would hold for the host-concatenated arrays, gathered
        on the device from `objects` (layout order) under the TLAS-region nodes, TLASBVH8Indices, _MeshData and
        materials given here."""
        tlas_nodes = np.ascontiguousarray(tlas_nodes, NODE_DTYPE)
        tlas = np.ascontiguousarray(tlas, np.int32)
        meshdata = np.ascontiguousarray(meshdata, MESH_DTYPE)
        materials = np.ascontiguousarray(materials, MAT_DTYPE)
        st = self.L.tt_scene_assemble_objects(self.h, _object_handles(objects), len(objects), _ptr(tlas_nodes),
                                              len(tlas_nodes), _ptr(tlas), len(tlas), _ptr(meshdata), len(meshdata),
                                              _ptr(materials), len(materials))
        self._check(st, "tt_scene_assemble_objects")

    def upload_alpha_atlas(self, atlas: np.ndarray):
        """_AlphaAtlas (AssetManager.cs:260-262): R8 texels, row 0 = v in [0, 1/height)."""
        a = np.ascontiguousarray(atlas, np.uint8)
        self._check(self.L.tt_scene_upload_alpha_atlas(self.h, _ptr(a), a.shape[1], a.shape[0]),
                    "tt_scene_upload_alpha_atlas")

    def upload_texture_atlas(self, atlas: np.ndarray):
        """_TextureAtlas (AssetManager.cs:275) decoded to RGBA half: float16 [height, width, 4]."""
        a = np.ascontiguousarray(atlas, np.float16)
        assert a.ndim == 3 and a.shape[2] == 4
        self._check(self.L.tt_scene_upload_texture_atlas(self.h, _ptr(a), a.shape[1], a.shape[0]),
                    "tt_scene_upload_texture_atlas")

    def upload_terrains(self, terrains, heightmap=None, check: bool = True):
        """tt_scene_upload_terrains: TERRAIN_DTYPE records and the Heightmap atlas as binary16 bits (uint16, or
        float16) [height, width]. No terrains (None or empty) clears the set."""
        t = np.zeros(0, TERRAIN_DTYPE) if terrains is None else np.ascontiguousarray(terrains, TERRAIN_DTYPE)
        if heightmap is None:
            hm, w, h = None, 0, 0
        else:
            hm = np.ascontiguousarray(heightmap)
            hm = hm.view(np.uint16) if hm.dtype == np.float16 else np.ascontiguousarray(hm, np.uint16)
            assert hm.ndim == 2
            h, w = hm.shape
        st = self.L.tt_scene_upload_terrains(self.h, _ptr(t) if len(t) else None, len(t), _ptr(hm), w, h)
        if check:
            self._check(st, "tt_scene_upload_terrains")
        return st

    def trace_heightmap(self, rays, n_rays: int, bounce: int, far_plane: float, width: int, height: int, info=None,
                        flags: int = 0, device: bool = False, stats: bool = False, check: bool = True,
                        asynchronous: bool = False):
        """tt_trace_heightmap (kernel_heightmap replacement): marches the uploaded terrains for the rays
        tt_trace_closest just traced; records and info texels are rewritten in place for terrain hits."""
        p = TraceParams(n_rays=n_rays, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                        flags=flags | (TT_TRACE_DEVICE_PTRS if device else 0) | (TT_TRACE_STATS if stats else 0)
                        | (TT_TRACE_ASYNC if asynchronous else 0))
        s = Stats()
        st = self.L.tt_trace_heightmap(self.h, C.byref(p), _ptr(rays), _ptr(info), C.byref(s))
        if check:
            self._check(st, "tt_trace_heightmap")
        return (s, st) if not check else s

    def trace_heightmap_hits(self, rays, hits_out, n_rays: int, bounce: int, far_plane: float, width: int, height: int,
                             info=None, flags: int = 0, device: bool = True, asynchronous: bool = False,
                             check: bool = True):
        """tt_trace_heightmap_hits: tt_trace_heightmap that also writes every record it rewrites to the contiguous
        hit stream hits_out (the buffer tt_trace_closest_hits filled for the same rays). Device pointers."""
        p = TraceParams(n_rays=n_rays, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                        flags=flags | (TT_TRACE_DEVICE_PTRS if device else 0) | (TT_TRACE_ASYNC if asynchronous else 0))
        st = self.L.tt_trace_heightmap_hits(self.h, C.byref(p), _ptr(rays), _ptr(info), _ptr(hits_out))
        if check:
            self._check(st, "tt_trace_heightmap_hits")
        return st

    def trace_heightmap_indirect(self, rays, n_rays_dev, capacity: int, bounce: int, far_plane: float, width: int,
                                 height: int, info=None, flags: int = 0, check: bool = True):
        """tt_trace_heightmap_indirect: min(*n_rays_dev, capacity) rays; device pointers, asynchronous."""
        p = TraceParams(n_rays=capacity, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                        flags=flags | TT_TRACE_DEVICE_PTRS)
        st = self.L.tt_trace_heightmap_indirect(self.h, C.byref(p), _ptr(n_rays_dev), _ptr(rays), _ptr(info))
        if check:
            self._check(st, "tt_trace_heightmap_indirect")
        return st

    def shadow_heightmap(self, shadow_rays, n_rays: int, bounce: int, width: int, height: int, visibility=None,
                         colors=None, nee_pos=None, cache=None, flags: int = 0, device: bool = False,
                         asynchronous: bool = False, n_rays_dev=None, check: bool = True):
        """tt_trace_shadow_heightmap (kernel_shadow_heightmap replacement); with n_rays_dev the indirect form
        (n_rays is then the capacity; device pointers, asynchronous)."""
        p = ShadowParams(n_rays=n_rays, bounce=bounce, screen_width=width, screen_height=height,
                         flags=flags | (TT_TRACE_DEVICE_PTRS if (device or n_rays_dev is not None) else 0)
                         | (TT_TRACE_ASYNC if asynchronous else 0))
        if n_rays_dev is not None:
            st = self.L.tt_trace_shadow_heightmap_indirect(self.h, C.byref(p), _ptr(n_rays_dev), _ptr(shadow_rays),
                                                           _ptr(visibility), _ptr(colors), _ptr(nee_pos), _ptr(cache))
        else:
            st = self.L.tt_trace_shadow_heightmap(self.h, C.byref(p), _ptr(shadow_rays), _ptr(visibility),
                                                  _ptr(colors), _ptr(nee_pos), _ptr(cache))
        if check:
            self._check(st, "tt_trace_shadow_heightmap")
        return st

    def update_nodes(self, first: int, nodes: np.ndarray):
        self._check(self.L.tt_scene_update_nodes(self.h, first, len(nodes), _ptr(nodes)), "tt_scene_update_nodes")

    def update_meshdata(self, first: int, md: np.ndarray):
        self._check(self.L.tt_scene_update_meshdata(self.h, first, len(md), _ptr(md)), "tt_scene_update_meshdata")

    def sync(self):
        self._check(self.L.tt_sync(self.h), "tt_sync")

    def async_overflows(self) -> int:
        """tt_async_overflows: stack overflows of all launches since the last call (then reset)."""
        n = C.c_uint64()
        st = self.L.tt_async_overflows(self.h, C.byref(n))
        if st not in (TT_OK, TT_ERR_STACK_OVERFLOW):
            self._check(st, "tt_async_overflows")
        return int(n.value)

    def timing_reset(self):
        self._check(self.L.tt_timing_reset(self.h), "tt_timing_reset")

    def set_timing(self, enabled: bool):
        """tt_ctx_set_timing: off, asynchronous calls record no HIP events (and add no timing entry)."""
        self._check(self.L.tt_ctx_set_timing(self.h, 1 if enabled else 0), "tt_ctx_set_timing")

    def set_frame_pixels(self, frame_pixels: int):
        """tt_ctx_set_frame_pixels: batched frames (PixelIndex + j W H) draw frame j's bounce random numbers
        at frames + j from their frame-local pixel; 0 restores the reference's form."""
        self._check(self.L.tt_ctx_set_frame_pixels(self.h, int(frame_pixels)), "tt_ctx_set_frame_pixels")

    def timing_read(self) -> np.ndarray:
        ms = np.zeros(256, np.float32)
        n = C.c_uint32()
        self._check(self.L.tt_timing_read(self.h, ms.ctypes.data, 256, C.byref(n)), "tt_timing_read")
        return ms[: n.value].copy()

    def diagnostics(self) -> dict:
        d = np.zeros(8, np.uint64)
        self._check(self.L.tt_trace_diagnostics(self.h, d.ctypes.data), "tt_trace_diagnostics")
        keys = ["iterations", "node_iters", "node_lanes", "tri_iters", "tri_lanes", "active_lanes", "lead_same_lanes",
                "uniform_node_iters"]
        return {k: int(v) for k, v in zip(keys, d)}

    def last_trace_form(self) -> int:
        """tt_trace_last_form: TT_TRACE_FORM_GENERIC or TT_TRACE_FORM_LEAF for the context's last trace launch."""
        f = C.c_uint32()
        self._check(self.L.tt_trace_last_form(self.h, C.byref(f)), "tt_trace_last_form")
        return int(f.value)

    def selftest_rcp(self) -> int:
        """Inputs (of all 2^32 fp32 bit patterns) where the kernels' fast reciprocal differs from the
        correctly rounded 1.0f/x on this device (tt_selftest_rcp); must be 0."""
        n = C.c_uint64()
        self._check(self.L.tt_selftest_rcp(self.h, C.addressof(n)), "tt_selftest_rcp")
        return n.value

    def scene_bytes(self) -> int:
        b = C.c_uint64()
        self._check(self.L.tt_scene_bytes(self.h, C.byref(b)), "tt_scene_bytes")
        return b.value

    def trace(self, rays, n_rays: int, bounce: int, far_plane: float, width: int, height: int, info=None,
              colors=None, flags: int = 0, device: bool = False, stats: bool = False, check: bool = True,
              asynchronous: bool = False, hits_out=None):
        p = TraceParams(n_rays=n_rays, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                        flags=flags | (TT_TRACE_DEVICE_PTRS if device else 0) | (TT_TRACE_STATS if stats else 0)
                        | (TT_TRACE_ASYNC if asynchronous else 0))
        s = Stats()
        if hits_out is not None:  # tt_trace_closest_hits: also the compact hit-record stream (no stats)
            st = self.L.tt_trace_closest_hits(self.h, C.byref(p), _ptr(rays), _ptr(info), _ptr(colors), _ptr(hits_out))
        else:
            st = self.L.tt_trace_closest(self.h, C.byref(p), _ptr(rays), _ptr(info), _ptr(colors), C.byref(s))
        if check:
            self._check(st, "tt_trace_closest")
        return (s, st) if not check else s

    def trace_indirect(self, rays, n_rays_dev, capacity: int, bounce: int, far_plane: float, width: int, height: int,
                       info=None, colors=None, flags: int = 0, check: bool = True):
        """tt_trace_closest_indirect: traces min(*n_rays_dev, capacity) rays, the count read on the device
        (a uint32 device tensor, e.g. the n_next_dev of enqueue_bounce_indirect); device pointers, async."""
        p = TraceParams(n_rays=capacity, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                        flags=flags | TT_TRACE_DEVICE_PTRS)
        st = self.L.tt_trace_closest_indirect(self.h, C.byref(p), _ptr(n_rays_dev), _ptr(rays), _ptr(info),
                                              _ptr(colors))
        if check:
            self._check(st, "tt_trace_closest_indirect")
        return st

    def tlas_refit(self, n_tlas_nodes: int, mesh_aabbs, device: bool = False, asynchronous: bool = False):
        """tt_tlas_refit (AssetManager.RefitTLAS): re-quantize TLAS nodes [0, n_tlas_nodes) in HBM from
        per-mesh world AABBs (n_mesh x {BBMax, BBMin})."""
        n = int(mesh_aabbs.shape[0]) if hasattr(mesh_aabbs, "shape") else len(mesh_aabbs) // 6
        flags = (TT_TRACE_DEVICE_PTRS if device else 0) | (TT_TRACE_ASYNC if asynchronous else 0)
        self._check(self.L.tt_tlas_refit(self.h, n_tlas_nodes, _ptr(mesh_aabbs), n, flags), "tt_tlas_refit")

    def update_tlas(self, nodes: np.ndarray, tlas_indices: np.ndarray, asynchronous: bool = False):
        """tt_scene_update_tlas: install a host-built TLAS (tlas_build) -- nodes [0, len(nodes)), the whole
        TLASBVH8Indices and the leaf records -- as one mutation; the arrays may be reused at once."""
        nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
        idx = np.ascontiguousarray(tlas_indices, np.int32)
        self._check(self.L.tt_scene_update_tlas(self.h, _ptr(nodes), len(nodes), _ptr(idx), len(idx),
                                                TT_TRACE_ASYNC if asynchronous else 0), "tt_scene_update_tlas")

    def tlas_rebuild(self, mesh_aabbs, device: bool = False) -> int:
        """tt_tlas_rebuild (AssetManager.CorrectRefit + the swap of RefitTLAS): build a new TLAS over per-mesh
        world AABBs (n_mesh x {BBMax, BBMin}) on the device and install it. Returns the new n_tlas_nodes."""
        n = int(mesh_aabbs.shape[0]) if hasattr(mesh_aabbs, "shape") else len(mesh_aabbs) // 6
        out = C.c_uint32()
        self._check(self.L.tt_tlas_rebuild(self.h, _ptr(mesh_aabbs), n, TT_TRACE_DEVICE_PTRS if device else 0,
                                           C.byref(out)), "tt_tlas_rebuild")
        return int(out.value)

    def scene_tlas_indices(self, first: int, count: int) -> np.ndarray:
        """Reads TLASBVH8Indices [first, first+count) back from HBM (the counterpart of scene_nodes)."""
        out = np.zeros(count, np.int32)
        self._check(self.L.tt_scene_read_tlas_indices(self.h, first, count, _ptr(out)), "tt_scene_read_tlas_indices")
        return out

    def blas_refit(self, mesh_index: int, vertices, indices, leaf_of_triangle, transform=None,
                   device: bool = False, asynchronous: bool = False):
        """tt_blas_refit (ParentObject.RefitMesh): re-derive the mesh's triangles from `vertices`
        (n x stride floats: position at +0, normal at +3) and refit its BLAS nodes in HBM.
        `transform` is a row-major 4x4 (identity by default)."""
        stride = int(vertices.shape[1]) if hasattr(vertices, "shape") and len(vertices.shape) == 2 else 6
        nv = int(vertices.shape[0]) if hasattr(vertices, "shape") and len(vertices.shape) == 2 else len(vertices) // 6
        n_tris = int(indices.shape[0]) // 3 if len(indices.shape) == 1 else int(indices.shape[0])
        p = BlasRefitParams(mesh_index=mesh_index, n_tris=n_tris, n_vertices=nv, vertex_stride=stride,
                            flags=(TT_TRACE_DEVICE_PTRS if device else 0) | (TT_TRACE_ASYNC if asynchronous else 0))
        p.transform[:] = unity_colmajor(np.eye(4) if transform is None else np.asarray(transform))
        self._check(self.L.tt_blas_refit(self.h, C.byref(p), _ptr(vertices), _ptr(indices), _ptr(leaf_of_triangle)),
                    "tt_blas_refit")

    def blas_refit_many(self, items, device: bool = False, asynchronous: bool = False, bounds_out=None,
                        mesh_aabbs=None, check: bool = True) -> int:
        """tt_blas_refit_many (ParentObject.RefitMesh for a frame's deforming meshes, renderer by renderer): `items`
        is a list of RefitItem. bounds_out (n_items x 6) and mesh_aabbs (n_mesh x 6, the array tlas_refit takes)
        are written in place: numpy arrays, or device tensors with device=True."""
        arr, keep = refit_item_array(items)
        flags = (TT_TRACE_DEVICE_PTRS if device else 0) | (TT_TRACE_ASYNC if asynchronous else 0)
        st = self.L.tt_blas_refit_many(self.h, arr, len(items), flags, _ptr(bounds_out), _ptr(mesh_aabbs))
        del keep
        if check:
            self._check(st, "tt_blas_refit_many")
        return st

    def scene_tris(self, first: int, count: int) -> np.ndarray:
        """Reads AggTris [first, first+count) back from HBM (parity checks of the BLAS refit)."""
        out = np.zeros(count, TRI_DTYPE)
        self._check(self.L.tt_scene_read_tris(self.h, first, count, _ptr(out)), "tt_scene_read_tris")
        return out

    def scene_nodes(self, first: int, count: int) -> np.ndarray:
        """Reads nodes [first, first+count) back from HBM (parity checks of the refit)."""
        out = np.zeros(count, NODE_DTYPE)
        self._check(self.L.tt_scene_read_nodes(self.h, first, count, _ptr(out)), "tt_scene_read_nodes")
        return out

    def trace_shadow(self, shadow_rays, n_rays: int, bounce: int, width: int, height: int, visibility=None,
                     colors=None, nee_pos=None, device: bool = False, stats: bool = False, check: bool = True,
                     asynchronous: bool = False, flags: int = 0, cache=None, legacy: bool = False):
        """tt_trace_shadow_ex (kernel_shadow replacement): any-hit visibility of ShadowRayData rays and
        the GlobalColors / CacheBuffer accumulations (flags: TT_SHADOW_*, TT_TRACE_USE_RESTIRGI).
        legacy=True calls tt_trace_shadow instead (Direct at bounce 0 + NEEPosA only, no cache)."""
        p = ShadowParams(n_rays=n_rays, bounce=bounce, screen_width=width, screen_height=height,
                         flags=flags | (TT_TRACE_DEVICE_PTRS if device else 0) | (TT_TRACE_STATS if stats else 0)
                         | (TT_TRACE_ASYNC if asynchronous else 0))
        s = Stats()
        if legacy:
            assert cache is None, "tt_trace_shadow takes no CacheBuffer"
            st = self.L.tt_trace_shadow(self.h, C.byref(p), _ptr(shadow_rays), _ptr(visibility), _ptr(colors),
                                        _ptr(nee_pos), C.byref(s))
        else:
            st = self.L.tt_trace_shadow_ex(self.h, C.byref(p), _ptr(shadow_rays), _ptr(visibility), _ptr(colors),
                                           _ptr(nee_pos), _ptr(cache), C.byref(s))
        if check:
            self._check(st, "tt_trace_shadow" if legacy else "tt_trace_shadow_ex")
        return (s, st) if not check else s

    def trace_shadow_indirect(self, shadow_rays, n_rays_dev, capacity: int, bounce: int, width: int, height: int,
                              visibility=None, colors=None, nee_pos=None, flags: int = 0, cache=None, check: bool = True):
        """tt_trace_shadow_ex_indirect: min(*n_rays_dev, capacity) shadow rays; device pointers, async."""
        p = ShadowParams(n_rays=capacity, bounce=bounce, screen_width=width, screen_height=height,
                         flags=flags | TT_TRACE_DEVICE_PTRS)
        st = self.L.tt_trace_shadow_ex_indirect(self.h, C.byref(p), _ptr(n_rays_dev), _ptr(shadow_rays),
                                                _ptr(visibility), _ptr(colors), _ptr(nee_pos), _ptr(cache))
        if check:
            self._check(st, "tt_trace_shadow_ex_indirect")
        return st

    def resolve_normals(self, rays, n_rays: int, bounce: int, far_plane: float, width: int, height: int,
                        out=None, device: bool = False):
        p = TraceParams(n_rays=n_rays, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                        flags=TT_TRACE_DEVICE_PTRS if device else 0)
        if out is None:
            out = np.zeros((n_rays, 6), np.float32)
        self._check(self.L.tt_resolve_normals(self.h, C.byref(p), _ptr(rays), _ptr(out)), "tt_resolve_normals")
        return out

    def generate(self, rays, cam_to_world, cam_inv_proj, width, height, near, far, jitter=0, frames=0,
                 max_bounce=3, device=False, asynchronous=False):
        cam = Camera()
        cam.cam_to_world[:] = unity_colmajor(cam_to_world)
        cam.cam_inv_proj[:] = unity_colmajor(cam_inv_proj)
        cam.near_plane, cam.far_plane, cam.width, cam.height = near, far, width, height
        cam.jitter, cam.frames_accumulated, cam.max_bounce = jitter, frames, max_bounce
        cam.flags = (TT_TRACE_DEVICE_PTRS if device else 0) | (TT_TRACE_ASYNC if (device and asynchronous) else 0)
        self._check(self.L.tt_generate_primary(self.h, C.byref(cam), _ptr(rays)), "tt_generate_primary")

    def enqueue_bounce(self, rays, n_rays, bounce, far_plane, width, height, frames=0, max_bounce=3,
                       device=False, terrain_bounce: bool = False) -> int:
        """terrain_bounce: TT_ENQUEUE_TERRAIN_BOUNCE (terrain hits bounce off the terrain instead of ending)."""
        p = TraceParams(n_rays=n_rays, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                        flags=(TT_TRACE_DEVICE_PTRS if device else 0)
                        | (TT_ENQUEUE_TERRAIN_BOUNCE if terrain_bounce else 0))
        n = C.c_uint32()
        self._check(self.L.tt_enqueue_diffuse_bounce(self.h, C.byref(p), _ptr(rays), frames, max_bounce,
                                                     C.byref(n)), "tt_enqueue_diffuse_bounce")
        return n.value

    def enqueue_bounce_indirect(self, rays, n_rays_dev, capacity, n_next_dev, bounce, far_plane, width, height,
                                frames=0, max_bounce=3, check: bool = True, terrain_bounce: bool = False):
        """tt_enqueue_diffuse_bounce_indirect: the traced count from n_rays_dev (None: capacity), the survivor
        count written to the device uint32 n_next_dev; no synchronization. terrain_bounce:
        TT_ENQUEUE_TERRAIN_BOUNCE."""
        p = TraceParams(n_rays=capacity, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                        flags=TT_TRACE_DEVICE_PTRS | (TT_ENQUEUE_TERRAIN_BOUNCE if terrain_bounce else 0))
        st = self.L.tt_enqueue_diffuse_bounce_indirect(self.h, C.byref(p), _ptr(n_rays_dev), _ptr(rays), frames,
                                                       max_bounce, _ptr(n_next_dev))
        if check:
            self._check(st, "tt_enqueue_diffuse_bounce_indirect")
        return st


    def upload_lights(self, lights: "Lights", check: bool = True):
        """tt_scene_upload_lights: the scene's LightNodes / LightTriangles / _LightMeshes."""
        st = self.L.tt_scene_upload_lights(self.h, _ptr(lights.nodes), len(lights.nodes), _ptr(lights.tris),
                                           len(lights.tris), _ptr(lights.meshes), len(lights.meshes))
        if check:
            self._check(st, "tt_scene_upload_lights")
        return st

    def update_light_nodes(self, first: int, nodes: np.ndarray, check: bool = True):
        st = self.L.tt_scene_update_light_nodes(self.h, first, len(nodes), _ptr(nodes))
        if check:
            self._check(st, "tt_scene_update_light_nodes")
        return st

    def refit_lights(self, mesh_indices=(), transforms=None, device=False, asynchronous=False, flags=0,
                     check: bool = True):
        """tt_lights_refit. mesh_indices: the _MeshData records whose light trees follow their refit triangles (host);
        transforms: LIGHT_TRANSFORM_DTYPE rows (host array, or a device buffer of them with device=True), None: no
        TLAS pass."""
        mi = np.ascontiguousarray(mesh_indices, np.uint32)
        if transforms is None:
            x, nx = None, 0
        elif isinstance(transforms, np.ndarray):
            x = np.ascontiguousarray(transforms, LIGHT_TRANSFORM_DTYPE)
            nx = len(x)
        else:  # a device tensor of bytes: 68 per row
            x, nx = transforms, transforms.numel() * transforms.element_size() // 68
        st = self.L.tt_lights_refit(self.h, _ptr(mi) if len(mi) else None, len(mi), _ptr(x), nx,
                                    flags | (TT_TRACE_DEVICE_PTRS if device else 0) | (TT_TRACE_ASYNC if asynchronous else 0))
        if check:
            self._check(st, "tt_lights_refit")
        return st

    def read_light_nodes(self, first: int, count: int) -> np.ndarray:
        out = np.zeros(count, LIGHT_NODE_DTYPE)
        self._check(self.L.tt_scene_read_light_nodes(self.h, first, count, _ptr(out)), "tt_scene_read_light_nodes")
        return out

    def read_light_tris(self, first: int, count: int) -> np.ndarray:
        out = np.zeros(count, LIGHT_TRI_DTYPE)
        self._check(self.L.tt_scene_read_light_tris(self.h, first, count, _ptr(out)), "tt_scene_read_light_tris")
        return out

    def emit_nee(self, rays, n_rays, bounce, far_plane, width, height, frames=0, max_bounce=3, samples=None,
                 shadow_rays=None, device=False, asynchronous=False, flags=0, check: bool = True):
        """tt_emit_nee: the survivor count (None when asynchronous); samples / shadow_rays are filled in place.
        check=False returns (status, count)."""
        p = TraceParams(n_rays=n_rays, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                        flags=flags | (TT_TRACE_DEVICE_PTRS if device else 0) | (TT_TRACE_ASYNC if asynchronous else 0))
        n = C.c_uint32()
        st = self.L.tt_emit_nee(self.h, C.byref(p), _ptr(rays), frames, max_bounce, _ptr(samples), _ptr(shadow_rays),
                                None if asynchronous else C.byref(n))
        if not check:
            return st, n.value
        self._check(st, "tt_emit_nee")
        return None if asynchronous else n.value

    def emit_nee_indirect(self, rays, n_rays_dev, capacity, n_shadow_dev, bounce, far_plane, width, height, frames=0,
                          max_bounce=3, samples=None, shadow_rays=None, flags=0, check: bool = True):
        """tt_emit_nee_indirect: the traced count from n_rays_dev (None: capacity), the survivor count written to the
        device uint32 n_shadow_dev; no synchronization."""
        p = TraceParams(n_rays=capacity, bounce=bounce, far_plane=far_plane, screen_width=width, screen_height=height,
                        flags=flags | TT_TRACE_DEVICE_PTRS)
        st = self.L.tt_emit_nee_indirect(self.h, C.byref(p), _ptr(n_rays_dev), _ptr(rays), frames, max_bounce,
                                         _ptr(samples), _ptr(shadow_rays), _ptr(n_shadow_dev))
        if check:
            self._check(st, "tt_emit_nee_indirect")
        return st


class DedicatedStream:
    """A HIP stream on a hardware queue of its own (tt_stream_create) wrapped as a torch ExternalStream.

    Concurrent trace launches (the parts / frame slots of ttlayout.FrameLayout, the gather stream) need
    streams that do not share a HW queue: a process's plain streams are dealt round-robin over a few
    queues, and two persistent grids on one queue run back to back instead of overlapping each other's
    drain (profiles/r04/streams/). ``close()`` synchronises and destroys it."""

    def __init__(self, torch, dev):
        L = hip_lib()
        h = C.c_void_p()
        _check(L.tt_stream_create(int(dev.index or 0), C.byref(h)), "tt_stream_create")
        self.handle = h.value
        self.stream = torch.cuda.ExternalStream(self.handle, device=dev)

    def close(self):
        if self.handle:
            _check(hip_lib().tt_stream_destroy(C.c_void_p(self.handle)), "tt_stream_destroy")
            self.handle = None
            self.stream = None


_DEDICATED = {}
_ENGINES = weakref.WeakSet()  # live contexts: closed before the dedicated streams they may issue on


def release_dedicated_streams():
    """Synchronises and destroys every process-wide dedicated stream (registered with atexit on the first
    one): a queue made with a CU mask that is still alive when the HIP runtime tears down takes the process
    down with it under rocprofv3 (exit status 139 in __cxa_finalize, gpurun_out/r04o). Torch's current
    stream is reset to the default stream first, so nothing issues on a destroyed handle."""
    if not _DEDICATED:
        return
    try:
        import torch

        for dev_i in {k[0] for k in _DEDICATED}:
            torch.cuda.synchronize(dev_i)
            torch.cuda.set_stream(torch.cuda.default_stream(dev_i))
    except Exception:  # noqa: BLE001 -- teardown: the streams go regardless
        pass
    for e in list(_ENGINES):  # a context synchronises its stream when destroyed: destroy it first
        try:
            e.close()
        except Exception:  # noqa: BLE001
            pass
    for d in list(_DEDICATED.values()):
        try:
            d.close()
        except Exception:  # noqa: BLE001
            pass
    _DEDICATED.clear()


def dedicated_stream(torch, dev, i: int):
    """The i-th process-wide stream with a HW queue of its own (a DedicatedStream made on first use and
    kept for the process's lifetime), as a torch ExternalStream. Layouts take streams 0, 1, ... in turn,
    so a process holds as many dedicated queues as its widest layout needs however many layouts it
    builds (tools/strong_replay.py builds one per rank), and a stream outlives every tensor, event and
    collective that was ever ordered on it."""
    key = (int(dev.index or 0), int(i))
    d = _DEDICATED.get(key)
    if d is None:
        if not _DEDICATED:
            import atexit

            atexit.register(release_dedicated_streams)
        d = DedicatedStream(torch, dev)
        _DEDICATED[key] = d
    return d.stream


def validate(s: Scene):
    """tt_scene_validate: (status, message) of the structural check tt_scene_upload runs."""
    buf = C.create_string_buffer(512)
    st = hip_lib().tt_scene_validate(_ptr(s.nodes), len(s.nodes), _ptr(s.tris), len(s.tris), _ptr(s.tlas),
                                     len(s.tlas), _ptr(s.meshdata), len(s.meshdata), _ptr(s.materials),
                                     len(s.materials), buf, 512)
    return st, buf.value.decode()


def device_count() -> int:
    try:
        return hip_lib().tt_device_count()
    except (FileNotFoundError, OSError):
        return 0


# ---------------------------------------------------------------- multi-GPU group (tt_group_*)
TT_GROUP_COPY_GATHER = 1 << 0
TT_GROUP_BOUNCE = 1 << 1
TT_GROUP_INFO = 1 << 2
GROUP_SYMBOLS = ["tt_group_create", "tt_group_unique_id", "tt_group_create_rank", "tt_group_destroy",
                 "tt_group_last_error", "tt_group_local_members", "tt_group_member_ctx", "tt_group_scene_upload",
                 "tt_group_trace_frame", "tt_group_sync", "tt_group_frame_rays", "tt_group_tile_pixels", "tt_shutdown"]


class GroupConfig(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("tile", C.c_uint32), ("slots", C.c_uint32),
                ("flags", C.c_uint32), ("batch", C.c_uint32)]


def _group_lib():
    L = hip_lib()
    if not getattr(L, "_group_bound", False):
        _bind_group(L)
    return L


def _bind_group(L):
    if True:
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
        L.tt_group_create.argtypes = [vp, u32, C.POINTER(GroupConfig), C.POINTER(vp)]
        L.tt_group_unique_id.argtypes = [vp]
        L.tt_group_create_rank.argtypes = [vp, u32, u32, i32, C.POINTER(GroupConfig), C.POINTER(vp)]
        L.tt_group_destroy.argtypes = [vp]
        L.tt_group_last_error.argtypes = [vp]
        L.tt_group_last_error.restype = C.c_char_p
        L.tt_group_local_members.argtypes = [vp]
        L.tt_group_local_members.restype = u32
        L.tt_group_member_ctx.argtypes = [vp, u32]
        L.tt_group_member_ctx.restype = vp
        L.tt_group_scene_upload.argtypes = [vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32]
        L.tt_group_trace_frame.argtypes = [vp, C.POINTER(Camera), vp, vp, u32]
        L.tt_group_scene_upload_alpha_atlas.argtypes = [vp, vp, u32, u32]
        L.tt_group_scene_update_meshdata.argtypes = [vp, u32, u32, vp]
        L.tt_group_scene_update_nodes.argtypes = [vp, u32, u32, vp]
        L.tt_group_tlas_refit.argtypes = [vp, u32, vp, u32, u32]
        L.tt_group_scene_upload_texture_atlas.argtypes = [vp, vp, u32, u32]
        if hasattr(L, "tt_group_scene_upload_terrains"):  # (absent from older variant libraries)
            L.tt_group_scene_upload_terrains.argtypes = [vp, vp, u32, vp, u32, u32]
            L.tt_group_scene_upload_terrains.restype = i32
        if hasattr(L, "tt_group_tlas_rebuild"):  # (absent from older libraries)
            L.tt_group_tlas_rebuild.argtypes = [vp, vp, u32, u32, C.POINTER(u32)]
            L.tt_group_tlas_rebuild.restype = i32
            L.tt_group_scene_update_tlas.argtypes = [vp, vp, u32, vp, u32, u32]
            L.tt_group_scene_update_tlas.restype = i32
        L.tt_group_sync.argtypes = [vp]
        L.tt_group_frame_rays.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(vp)]
        L.tt_group_tile_pixels.argtypes = [u32, u32, u32, u32, u32, vp, u32, C.POINTER(u32)]
        for s in ["tt_group_create", "tt_group_unique_id", "tt_group_create_rank", "tt_group_destroy",
                  "tt_group_scene_upload", "tt_group_trace_frame", "tt_group_sync", "tt_group_frame_rays",
                  "tt_group_tile_pixels", "tt_shutdown", "tt_group_scene_upload_alpha_atlas",
                  "tt_group_scene_upload_texture_atlas", "tt_group_scene_update_meshdata",
                  "tt_group_scene_update_nodes", "tt_group_tlas_refit"]:
            getattr(L, s).restype = i32
        L._group_bound = True


def group_tile_pixels(width: int, height: int, world: int, rank: int, tile: int = 64) -> np.ndarray:
    """tt_group_tile_pixels: the library's own shard of `rank` (host arithmetic, no GPU)."""
    L = _group_lib()
    n = C.c_uint32()
    _check(L.tt_group_tile_pixels(width, height, tile, world, rank, None, 0, C.byref(n)), "tt_group_tile_pixels")
    out = np.zeros(max(1, n.value), np.uint32)
    _check(L.tt_group_tile_pixels(width, height, tile, world, rank, out.ctypes.data, n.value, C.byref(n)),
           "tt_group_tile_pixels")
    return out[: n.value]


def group_unique_id() -> bytes:
    """tt_group_unique_id: the 128-byte RCCL id rank 0 makes for tt_group_create_rank."""
    buf = (C.c_uint8 * 128)()
    _check(_group_lib().tt_group_unique_id(C.addressof(buf)), "tt_group_unique_id")
    return bytes(buf)


def shutdown():
    """tt_shutdown: destroys every library stream still alive (hosts tracing from a non-main thread)."""
    _check(hip_lib().tt_shutdown(), "tt_shutdown")


class Group:
    """A multi-GPU tile-sharded frame (tt_group_*): ``devices`` in one process (tt_group_create), or this
    process as ``rank`` of ``world`` on ``device`` with the RCCL id ``uid`` (tt_group_create_rank)."""

    def __init__(self, width: int, height: int, devices=None, tile: int = 64, slots: int = 2, bounce: bool = False,
                 copy: bool = False, rank: int = None, world: int = None, uid: bytes = None, device: int = None,
                 info: bool = False, batch: int = 1):
        L = _group_lib()
        cfg = GroupConfig(width=width, height=height, tile=tile, slots=slots, batch=batch,
                          flags=(TT_GROUP_BOUNCE if bounce else 0) | (TT_GROUP_COPY_GATHER if copy else 0)
                          | (TT_GROUP_INFO if info else 0))
        h = C.c_void_p()
        if devices is not None:
            devs = np.ascontiguousarray(devices, np.int32)
            st = L.tt_group_create(devs.ctypes.data, len(devs), C.byref(cfg), C.byref(h))
            self.world = len(devs)
        else:
            idb = (C.c_uint8 * 128).from_buffer_copy(uid)
            st = L.tt_group_create_rank(C.addressof(idb), world, rank, device, C.byref(cfg), C.byref(h))
            self.world = world
        if st != TT_OK:
            raise TTError(st, "tt_group_create")
        self.L, self.h = L, h.value
        self.width, self.height, self.bounce, self.batch = width, height, bounce, max(1, batch)

    def _check(self, st, what):
        if st != TT_OK:
            raise TTError(st, f"{what}: {self.L.tt_group_last_error(self.h).decode()}")

    def local_members(self) -> int:
        return int(self.L.tt_group_local_members(self.h))

    def member_ctx(self, m: int) -> int:
        return self.L.tt_group_member_ctx(self.h, m)

    def upload(self, s: Scene):
        st = self.L.tt_group_scene_upload(self.h, _ptr(s.nodes), len(s.nodes), _ptr(s.tris), len(s.tris),
                                          _ptr(s.tlas), len(s.tlas), _ptr(s.meshdata), len(s.meshdata),
                                          _ptr(s.materials), len(s.materials))
        self._check(st, "tt_group_scene_upload")
        if s.alpha_atlas is not None:
            a = np.ascontiguousarray(s.alpha_atlas, np.uint8)
            self._check(self.L.tt_group_scene_upload_alpha_atlas(self.h, a.ctypes.data, a.shape[1], a.shape[0]),
                        "tt_group_scene_upload_alpha_atlas")
        if s.texture_atlas is not None:
            t = np.ascontiguousarray(s.texture_atlas, np.float16)
            self._check(self.L.tt_group_scene_upload_texture_atlas(self.h, t.ctypes.data, t.shape[1], t.shape[0]),
                        "tt_group_scene_upload_texture_atlas")

    def upload_terrains(self, terrains, heightmap=None, check: bool = True):
        """tt_group_scene_upload_terrains: the terrain set of every local member (as Engine.upload_terrains); no
        terrains (None or empty) clears it."""
        t = np.zeros(0, TERRAIN_DTYPE) if terrains is None else np.ascontiguousarray(terrains, TERRAIN_DTYPE)
        hm = None if heightmap is None else _half_bits(heightmap)
        h, w = (0, 0) if hm is None else hm.shape
        st = self.L.tt_group_scene_upload_terrains(self.h, _ptr(t) if len(t) else None, len(t), _ptr(hm), w, h)
        if check:
            self._check(st, "tt_group_scene_upload_terrains")
        return st

    def trace_frame(self, hits_out, cam_to_world, cam_inv_proj, near, far, jitter=1, frames=0, max_bounce=1,
                    asynchronous=False, info_out=None):
        cam = Camera()
        cam.cam_to_world[:] = unity_colmajor(cam_to_world)
        cam.cam_inv_proj[:] = unity_colmajor(cam_inv_proj)
        cam.near_plane, cam.far_plane, cam.width, cam.height = near, far, self.width, self.height
        cam.jitter, cam.frames_accumulated, cam.max_bounce = jitter, frames, max_bounce
        cam.flags = TT_TRACE_DEVICE_PTRS
        self._check(self.L.tt_group_trace_frame(self.h, C.byref(cam), _ptr(hits_out), _ptr(info_out),
                                                TT_TRACE_ASYNC if asynchronous else 0), "tt_group_trace_frame")

    def sync(self):
        self._check(self.L.tt_group_sync(self.h), "tt_group_sync")

    def update_meshdata(self, first: int, md: np.ndarray):
        self._check(self.L.tt_group_scene_update_meshdata(self.h, first, len(md), _ptr(md)),
                    "tt_group_scene_update_meshdata")

    def update_nodes(self, first: int, nodes: np.ndarray):
        self._check(self.L.tt_group_scene_update_nodes(self.h, first, len(nodes), _ptr(nodes)),
                    "tt_group_scene_update_nodes")

    def tlas_refit(self, n_tlas_nodes: int, mesh_aabbs: np.ndarray, asynchronous: bool = False):
        a = np.ascontiguousarray(mesh_aabbs, np.float32)
        self._check(self.L.tt_group_tlas_refit(self.h, n_tlas_nodes, a.ctypes.data, a.shape[0],
                                               TT_TRACE_ASYNC if asynchronous else 0), "tt_group_tlas_refit")

    def tlas_rebuild(self, mesh_aabbs: np.ndarray) -> int:
        """tt_group_tlas_rebuild: every member rebuilds its TLAS over the (host) boxes; the new n_tlas_nodes."""
        a = np.ascontiguousarray(mesh_aabbs, np.float32)
        out = C.c_uint32()
        self._check(self.L.tt_group_tlas_rebuild(self.h, a.ctypes.data, a.shape[0], 0, C.byref(out)),
                    "tt_group_tlas_rebuild")
        return int(out.value)

    def update_tlas(self, nodes: np.ndarray, tlas_indices: np.ndarray, asynchronous: bool = False):
        nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
        idx = np.ascontiguousarray(tlas_indices, np.int32)
        self._check(self.L.tt_group_scene_update_tlas(self.h, _ptr(nodes), len(nodes), _ptr(idx), len(idx),
                                                      TT_TRACE_ASYNC if asynchronous else 0),
                    "tt_group_scene_update_tlas")

    def frame_rays(self, m: int = 0):
        """(n_primary, n_bounce, device pointer of the ray buffer) of member m's latest frame."""
        a, b, p = C.c_uint32(), C.c_uint32(), C.c_void_p()
        self._check(self.L.tt_group_frame_rays(self.h, m, C.byref(a), C.byref(b), C.byref(p)), "tt_group_frame_rays")
        return a.value, b.value, p.value

    def close(self):
        if getattr(self, "h", None):
            self.L.tt_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
