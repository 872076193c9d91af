"""GPU-resident objects without a GPU: AccumulateData's layout sums against AssetManager.build(), every refusal
of the object validator (tt_object_validate is stricter than the whole-scene check: an object must stand
alone), the same inputs through a stand-alone program under the host sanitizers, and the agreement of the
header, the ctypes prototypes and the C# binding."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import assemble_cases as AC
import tthip

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "truetrace_hip.h")).read(), flags=re.S)
NEW = ["tt_object_validate", "tt_object_create", "tt_object_get_info", "tt_object_destroy", "tt_scene_layout_objects",
       "tt_scene_layout_counts", "tt_scene_assemble_objects"]
BAD = ["child index == n_nodes", "triangle index == n_tris", "inner meta with child bits 2",
       "leaf meta reaching bit 24", "root >= n_nodes"]


def _counts():
    _, bl = AC.meshes_and_blases()
    return [(b.n_nodes, b.n_tris) for b in bl]


def _big():
    """The 4,097-triangle BLAS: it has inner nodes, so every violation can be planted in it."""
    _, bl = AC.meshes_and_blases()
    return bl[2].arrays()


# ------------------------------------------------------------------ layout
def test_layout_reproduces_the_asset_managers_offsets():
    am, s = AC.scene_s()
    n_par, n_ip = len(AC.PARENT_TRIS), len(AC.INSTANCE_PARENT_TRIS)
    assert len(s.meshdata) == n_par + len(AC.INSTANCES) and len(am.blases()) == n_par + n_ip
    region = 2 * len(s.meshdata)  # AssetManager.cs:995
    no, to, tn, tt = tthip.scene_layout(_counts(), region)
    assert tn == len(s.nodes) and tt == len(s.tris) and no[0] == region and to[0] == 0
    md = s.meshdata
    for k in range(n_par):  # a parent's record carries its own pair
        assert (md["NodeOffset"][k], md["TriOffset"][k]) == (no[k], to[k])
        assert md["mesh_data_bvh_offsets"][k] & 0x7FFFFFFF == no[k]
    for i, (ip, _) in enumerate(AC.INSTANCES):  # an instance's record its instance parent's
        k = n_par + i
        assert (md["NodeOffset"][k], md["TriOffset"][k]) == (no[n_par + ip], to[n_par + ip])
    # the GPU tests rely on it: some object's 88-byte triangles start 8- but not 16-byte aligned
    assert any((int(t) * 88) % 16 == 8 for t in to)


def test_layout_refuses_an_empty_list_and_sums_beyond_32_bits():
    with pytest.raises(tthip.TTError) as e:
        tthip.scene_layout([], 4)
    assert e.value.status == tthip.TT_ERR_INVALID_ARG
    with pytest.raises(tthip.TTError):
        tthip.scene_layout([(0xFFFFFFF0, 1), (0x20, 1)], 0)
    L = tthip.hip_lib()
    assert L.tt_scene_layout_objects(None, 0, 0, None, None, None, None) == tthip.TT_ERR_INVALID_ARG
    null = (C.c_void_p * 1)(None)
    assert L.tt_scene_layout_objects(null, 1, 0, None, None, None, None) == tthip.TT_ERR_INVALID_ARG


# ------------------------------------------------------------------ validator
def test_validator_accepts_every_blas_of_the_scene():
    _, bl = AC.meshes_and_blases()
    for b in bl:
        nodes, tris = b.arrays()
        assert tthip.object_validate(nodes, tris) == (tthip.TT_OK, "")


@pytest.mark.parametrize("name", BAD)
def test_validator_refuses(name):
    nodes, tris = _big()
    bad = AC.bad_objects(nodes, tris)
    assert sorted(bad) == sorted(BAD)
    a, t, root = bad[name]
    st, why = tthip.object_validate(a, t, root)
    assert st == tthip.TT_ERR_INVALID_ARG and why, name


def test_validator_is_stricter_than_the_whole_scene_check():
    """A BLAS reaching one node into its neighbour passes tt_scene_validate when a neighbour is there; as an
    object of its own it is refused."""
    import dataclasses

    _, s = AC.scene_s()
    assert tthip.validate(s)[0] == tthip.TT_OK
    k = 1  # the 65-triangle parent: the 4,097-triangle one follows it
    nodes, tris = AC.meshes_and_blases()[1][k].arrays()
    bad, _, _ = AC.bad_objects(nodes, tris)["child index == n_nodes"]
    st, why = tthip.object_validate(bad, tris)
    assert st == tthip.TT_ERR_INVALID_ARG and "child index" in why
    no = int(s.meshdata["NodeOffset"][k])
    merged = s.nodes.copy()
    merged[no:no + len(bad)] = bad
    assert tthip.validate(dataclasses.replace(s, nodes=merged))[0] == tthip.TT_OK


def test_validator_refuses_missing_arrays():
    L = tthip.hip_lib()
    why = C.create_string_buffer(64)
    assert L.tt_object_validate(None, 0, None, 0, 0, why, 64) == tthip.TT_ERR_INVALID_ARG and why.value
    nodes, tris = _big()
    assert L.tt_object_validate(nodes.ctypes.data, len(nodes), None, 0, 0, None, 0) == tthip.TT_ERR_INVALID_ARG


# ------------------------------------------------------------------ sanitizers
def test_validator_and_layout_under_sanitizers(tmp_path):
    """The stand-alone KAT program (its own main, no Python in the run) built with ASan + UBSan over
    csrc/tt_assemble_host.h, on the good and bad inputs above."""
    _, bl = AC.meshes_and_blases()
    cases = [(b.arrays() + (0,), 1) for b in bl]
    nodes, tris = _big()
    cases += [(v, 0) for _, v in sorted(AC.bad_objects(nodes, tris).items())]
    blob = struct.pack("<I", len(cases))
    for (a, t, root), ok in cases:
        blob += struct.pack("<4I", len(a), len(t), root, ok) + a.tobytes() + t.tobytes()
    _, s = AC.scene_s()
    region = 2 * len(s.meshdata)
    cnt = _counts()
    no, to, tn, tt = [], [], region, 0
    for n, t in cnt:  # the sums restated here, checked against build() above
        no.append(tn)
        to.append(tt)
        tn, tt = tn + n, tt + t
    assert (tn, tt) == (len(s.nodes), len(s.tris))
    blob += struct.pack("<2I", len(cnt), region)
    for (n, t), a, b in zip(cnt, no, to):
        blob += struct.pack("<4I", n, t, a, b)
    blob += struct.pack("<2I", tn, tt)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    exe = tmp_path / "assemble_kat"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "truetrace-unity-pathtracer_amd", "csrc"),
                    "-o", str(exe), os.path.join(HERE, "native", "assemble_kat_main.cpp")], check=True)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(cases)} cases + layout, 0 mismatches" in r.stdout and "runtime error" not in r.stderr


# ------------------------------------------------------------------ header / ctypes / C# agreement
def _params(name):
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", HDR)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def test_new_entry_points_are_exported_with_matching_prototypes():
    L = tthip.hip_lib()
    for name in NEW:
        assert hasattr(L, name), name
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == len(_params(name)), name
        assert f.restype is C.c_int32, name
    assert set(NEW) <= set(tthip.HIP_SYMBOLS)
    assert len(_params("tt_scene_assemble_objects")) == len(_params("tt_scene_upload")) == 11


def test_object_info_layout():
    assert C.sizeof(tthip.ObjectInfo) == 24
    assert re.search(r"TT_STATIC_ASSERT\(sizeof\(tt_object_info\) == 24", HDR)
    offs = {n: getattr(tthip.ObjectInfo, n).offset for n, _ in tthip.ObjectInfo._fields_}
    assert offs == {"n_nodes": 0, "n_tris": 4, "device": 8, "root": 12, "bytes": 16}
    fields = re.search(r"typedef struct tt_object_info \{(.*?)\} tt_object_info;", HDR, re.S).group(1)
    assert re.findall(r"\b(\w+);", fields) == [n for n, _ in tthip.ObjectInfo._fields_]


def test_csharp_binding_imports_every_new_function():
    cs = open(os.path.join(REPO, "bindings", "csharp", "TrueTraceHip.cs")).read()
    for name in NEW:
        m = re.search(r"\[DllImport\(Lib\)\][^;]*?\b" + name + r"\s*\(([^)]*)\)", cs, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_params(name)), name
    assert "class TrueTraceHipObject : IDisposable" in cs
    fields = re.search(r"public struct TTObjectInfo\s*\{(.*?)\}", cs, re.S).group(1)
    assert re.sub(r"\s+", " ", fields).strip() == "public uint nNodes, nTris; public int device; public uint root; public ulong bytes;"


def test_null_handles_are_rejected():
    L = tthip.hip_lib()
    info = tthip.ObjectInfo()
    assert L.tt_object_get_info(None, C.byref(info)) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_object_destroy(None) == tthip.TT_ERR_INVALID_ARG
    h = C.c_void_p()
    assert L.tt_object_create(None, None, 0, None, 0, 0, C.byref(h)) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_scene_assemble_objects(None, None, 0, None, 0, None, 0, None, 0, None, 0) == tthip.TT_ERR_INVALID_ARG
