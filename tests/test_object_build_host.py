"""Device-built objects without a GPU: tt_scene_assemble_tlas (the TLAS side from per-object summaries, no tt_blas)
against tt_scene_assemble on the same BLASes, the walk tt_object_build_device runs on its node mirror (no host
triangles) in a stand-alone program under the host sanitizers, and the agreement of the header, the ctypes
prototypes and the C# binding for the new entry points."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np

import assemble_cases as AC
import golden_io
import tthip

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _hdr(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


HDR, SCENE_HDR = _hdr("truetrace_hip.h"), _hdr("truetrace_scene.h")
NEW = ["tt_object_build_device", "tt_object_read", "tt_object_leaf_order_device"]


class _Summary:
    """What Engine.build_object reports for a BLAS, taken from the host build: assemble_objects reads nothing else."""

    def __init__(self, blas):
        i = blas.info
        self.build_info = tthip.ObjectBuildInfo(n_nodes=i.n_nodes, n_tris=i.n_tris, bvh2_depth=i.bvh2_depth)
        self.build_info.aabb_min[:], self.build_info.aabb_max[:] = i.aabb_min[:], i.aabb_max[:]


class _Recorder:
    """Stands in for an Engine: keeps what assemble_objects hands to Engine.assemble."""

    def assemble(self, objects, tlas_nodes, tlas, meshdata, materials):
        self.got = (objects, tlas_nodes, tlas, meshdata, materials)


def _assert_tlas_side_equals(am_objects, s):
    rec = _Recorder()
    s2, objs = am_objects.assemble_objects(rec)
    region = 2 * len(s.meshdata)
    assert len(s2.nodes) == region and s2.nodes.tobytes() == s.nodes[:region].tobytes(), "TLAS-region nodes"
    assert np.array_equal(s2.tlas, s.tlas), "TLASBVH8Indices"
    assert s2.meshdata.tobytes() == s.meshdata.tobytes(), "_MeshData"
    assert s2.meta["mesh_aabbs"].tobytes() == s.meta["mesh_aabbs"].tobytes(), "mesh AABBs"
    assert (s2.meta["n_nodes_total"], s2.meta["n_tris_total"], s2.tlas_nodes) == (len(s.nodes), len(s.tris), s.tlas_nodes)
    assert s2.materials.tobytes() == s.materials.tobytes() and len(s2.tris) == 0
    assert rec.got[0] == objs == am_objects.blases() and rec.got[1].tobytes() == s2.nodes.tobytes()


def test_tlas_side_of_scene_s_equals_the_full_assembly():
    am, s = AC.scene_s()
    _, bl = AC.meshes_and_blases()
    n_par = len(AC.PARENT_TRIS)
    am2 = tthip.AssetManager()
    for k, b in enumerate(bl[:n_par]):
        am2.add_parent_object(_Summary(b), tthip.trs_matrix(AC.PARENT_POS[k % len(AC.PARENT_POS)], 20.0 * k),
                              np.zeros(2, tthip.MAT_DTYPE))
    for b in bl[n_par:]:
        am2.add_instance_parent_object(_Summary(b), np.zeros(1, tthip.MAT_DTYPE))
    for ip, pos in AC.INSTANCES:
        am2.add_instance(ip, tthip.trs_matrix(pos, 35.0 * (ip + 1), 1.25))
    _assert_tlas_side_equals(am2, s)


def test_tlas_side_of_the_instanced_goldens_shape_equals_the_full_assembly():
    """One parent, one instance parent of another mesh, six instances (tests/golden/make_golden.py): the build
    equals the committed golden, and the TLAS side from summaries equals the build."""
    a, b = tthip.Blas(tthip.Mesh.soup(31, 600, 1.0, 0.1)), tthip.Blas(tthip.Mesh.prop(32, 800))
    am, am2 = tthip.AssetManager(), tthip.AssetManager()
    am.add_parent(a, tthip.trs_matrix((0, 0, 0), 10.0, 1.0), np.zeros(2, tthip.MAT_DTYPE))
    am2.add_parent_object(_Summary(a), tthip.trs_matrix((0, 0, 0), 10.0, 1.0), np.zeros(2, tthip.MAT_DTYPE))
    ip = am.add_instance_parent(b, np.zeros(3, tthip.MAT_DTYPE))
    assert am2.add_instance_parent_object(_Summary(b), np.zeros(3, tthip.MAT_DTYPE)) == ip
    for k in range(6):
        for m in (am, am2):
            m.add_instance(ip, tthip.trs_matrix((-6.0 + 2.5 * k, -1.0, -3.0 - k), 37.0 * k, 0.3 + 0.05 * k))
    s = am.build()
    g = golden_io.load("instanced")["scene"]
    assert s.nodes.tobytes() == g.nodes.tobytes() and s.meshdata.tobytes() == g.meshdata.tobytes()
    _assert_tlas_side_equals(am2, s)


def test_assemble_tlas_refusals():
    L = tthip.scene_lib()
    h = C.c_void_p()
    d = (tthip.ObjectDesc * 1)()
    inst = (tthip.InstanceDesc * 1)()
    assert L.tt_scene_assemble_tlas(None, 0, None, 0, None, 0, C.byref(h)) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_scene_assemble_tlas(C.addressof(d), 1, None, 0, None, 0, None) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_scene_assemble_tlas(C.addressof(d), 1, None, 0, None, 0, C.byref(h)) == tthip.TT_ERR_INVALID_ARG  # no nodes
    d[0].n_nodes = d[0].n_tris = 1
    inst[0].instance_parent = 0  # no instance parent to point at
    assert L.tt_scene_assemble_tlas(C.addressof(d), 1, None, 0, C.addressof(inst), 1, C.byref(h)) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_scene_build_get_totals(None, None, None) == tthip.TT_ERR_INVALID_ARG
    am = tthip.AssetManager()
    am.add_parent_object(_Summary(AC.meshes_and_blases()[1][0]))
    try:
        am.build()
    except TypeError:
        pass
    else:
        raise AssertionError("AssetManager.build accepted an object that is no Blas")


# ------------------------------------------------------------------ the walk on a node mirror, under sanitizers
def test_walk_without_host_triangles_under_sanitizers(tmp_path):
    _, bl = AC.meshes_and_blases()
    cases = [(b.arrays() + (0,), 1) for b in bl]
    nodes, tris = bl[2].arrays()
    cases += [(v, 0) for _, v in sorted(AC.bad_objects(nodes, tris).items())]
    blob = struct.pack("<I", len(cases))
    for (a, t, root), ok in cases:
        blob += struct.pack("<4I", len(a), len(t), root, ok) + a.tobytes() + t.tobytes()
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    exe = tmp_path / "object_build_kat"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "truetrace-unity-pathtracer_amd", "csrc"),
                    "-o", str(exe), os.path.join(HERE, "native", "object_build_kat_main.cpp")], check=True)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(cases)} cases, 0 mismatches" in r.stdout and "runtime error" not in r.stderr


# ------------------------------------------------------------------ header / ctypes / C# agreement
def _params(hdr, name):
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def test_new_entry_points_are_exported_with_matching_prototypes():
    L, S = tthip.hip_lib(), tthip.scene_lib()
    for lib, hdr, names in ((L, HDR, NEW), (S, SCENE_HDR, ["tt_scene_assemble_tlas", "tt_scene_build_get_totals"])):
        for name in names:
            assert hasattr(lib, name), name
            f = getattr(lib, name)
            assert f.argtypes is not None and len(f.argtypes) == len(_params(hdr, name)), name
            assert f.restype is C.c_int32, name
    assert set(NEW) <= set(tthip.HIP_SYMBOLS) and "tt_scene_assemble_tlas" in tthip.SCENE_SYMBOLS
    assert len(_params(SCENE_HDR, "tt_scene_assemble_tlas")) == len(_params(SCENE_HDR, "tt_scene_assemble")) == 7


def test_struct_layouts_match_the_headers():
    assert C.sizeof(tthip.ObjectBuildInfo) == 48
    assert re.search(r"TT_STATIC_ASSERT\(sizeof\(tt_object_build_info\) == 48", HDR)
    offs = {n: getattr(tthip.ObjectBuildInfo, n).offset for n, _ in tthip.ObjectBuildInfo._fields_}
    assert offs == {"n_nodes": 0, "n_tris": 4, "bvh2_depth": 8, "max_matdat": 12, "aabb_min": 16, "aabb_max": 28,
                    "presorted_on_host": 40, "pad": 44}
    # tt_mesh_input moved to truetrace_hip.h (the scene header includes it): one definition, the same fields
    assert "typedef struct tt_mesh_input" in HDR and "typedef struct tt_mesh_input" not in SCENE_HDR
    fields = re.search(r"typedef struct tt_mesh_input \{(.*?)\} tt_mesh_input;", HDR, re.S).group(1)
    assert re.findall(r"\b(\w+)(?:\[3\])?;", fields) == [n for n, _ in tthip.MeshInput._fields_]
    assert C.sizeof(tthip.MeshInput) == 80 and C.sizeof(tthip.ObjectDesc) == 4 * (2 + 6 + 32 + 1)
    fields = re.search(r"typedef struct tt_object_desc \{(.*?)\} tt_object_desc;", SCENE_HDR, re.S).group(1)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?[;,]", fields) == [n for n, _ in tthip.ObjectDesc._fields_]


def test_csharp_binding_imports_every_new_function():
    cs = open(os.path.join(REPO, "bindings", "csharp", "TrueTraceHip.cs")).read()
    for name in NEW:
        m = re.search(r"\[DllImport\(Lib\)\][^;]*?\b" + name + r"\s*\(([^)]*)\)", cs, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_params(HDR, name)), name
    fields = re.search(r"public struct TTObjectBuildInfo\s*\{(.*?)\}", cs, re.S).group(1)
    assert len(re.findall(r"\b(?:uint|float)\b", fields)) == 3 and fields.count(",") + fields.count(";") == 12
    assert "public struct TTMeshInput" in cs and "LeafOrderDevice" in cs


def test_null_handles_are_rejected():
    L = tthip.hip_lib()
    h, p = C.c_void_p(), C.c_void_p()
    assert L.tt_object_build_device(None, None, None, 0, C.byref(h), None) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_object_read(None, None, None, None, None) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_object_leaf_order_device(None, C.byref(p)) == tthip.TT_ERR_INVALID_ARG
