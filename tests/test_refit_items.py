"""tt_blas_refit_items_validate, the host-only half of tt_blas_refit_many's checks, on a scene built with
AssetManager: a well-formed item list passes, and every refusal that needs neither node data nor a device names
its first violation. The GPU side is tests/test_gpu_refit_many.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tthip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scene():
    meshes = [tthip.Mesh.soup(1, 120, 3.0, 0.3), tthip.Mesh.prop(3, 50), tthip.Mesh.prop(4, 300)]
    blases = [tthip.Blas(m) for m in meshes]
    am = tthip.AssetManager()
    am.add_parent(blases[0])
    am.add_parent(blases[1], tthip.trs_matrix((1.0, 0.0, 0.5)))
    ip = am.add_instance_parent(blases[2])
    am.add_instance(ip, tthip.trs_matrix((2.0, 0.0, 0.0)))
    am.add_instance(ip, tthip.trs_matrix((4.0, 0.0, 0.0)))
    return am.build(), meshes, blases


def item(scene, record, which, cuts=None, stride=10, **kw):
    """An item for _MeshData record `record` over mesh `which`, its source triangles cut into parts at `cuts`."""
    _, meshes, blases = scene
    pos, nrm, idx = meshes[which].arrays()
    n = blases[which].n_tris
    v = np.ascontiguousarray(np.concatenate([pos, nrm, np.zeros((len(pos), 4), np.float32)], axis=1)[:, :stride])
    cuts = [0, n] if cuts is None else cuts
    parts = [tthip.RefitPart(v, np.ascontiguousarray(idx[3 * a:3 * b]), first_tri=a) for a, b in zip(cuts[:-1], cuts[1:])]
    return tthip.RefitItem(record, kw.pop("n_tris", n), blases[which].leaf_order(), parts, **kw)


def validate(scene, items, device=False):
    sc = scene[0]
    return tthip.blas_refit_items_validate(items, sc.meshdata, len(sc.tris), device=device)


def test_a_well_formed_list_passes(scene):
    items = [item(scene, 1, 1, [0, 1, 17, 50]), item(scene, 0, 0), item(scene, 3, 2, [0, 299, 300], stride=6)]
    items[0].parts.reverse()  # parts in any order
    assert validate(scene, items) == (tthip.TT_OK, "")
    assert validate(scene, items, device=True) == (tthip.TT_OK, "")


def test_empty_and_null_lists(scene):
    st, why = validate(scene, [])
    assert st == tthip.TT_ERR_INVALID_ARG and "no items" in why
    it = item(scene, 1, 1)
    it.leaf_of_triangle = None
    st, why = validate(scene, [item(scene, 0, 0), it])
    assert st == tthip.TT_ERR_INVALID_ARG and "item 1" in why and "null" in why
    it = item(scene, 1, 1)
    it.parts[0].indices = None
    st, why = validate(scene, [it])
    assert st == tthip.TT_ERR_INVALID_ARG and "item 0: part 0" in why and "null" in why
    it = item(scene, 1, 1)
    it.parts = []
    st, why = validate(scene, [it])
    assert st == tthip.TT_ERR_INVALID_ARG and "item 0" in why


def test_stride_mesh_index_and_duplicates(scene):
    st, why = validate(scene, [item(scene, 1, 1, stride=5)])
    assert st == tthip.TT_ERR_INVALID_ARG and "vertex_stride < 6" in why
    st, why = validate(scene, [item(scene, 4, 1)])
    assert st == tthip.TT_ERR_INVALID_ARG and "mesh_index 4 out of range" in why
    st, why = validate(scene, [item(scene, 1, 1), item(scene, 0, 0), item(scene, 1, 1)])
    assert st == tthip.TT_ERR_INVALID_ARG and "item 2" in why and "item 0" in why and "mesh_index 1" in why


def test_two_instances_of_one_parent_share_a_blas(scene):
    sc = scene[0]
    assert sc.meshdata["NodeOffset"][2] == sc.meshdata["NodeOffset"][3]
    st, why = validate(scene, [item(scene, 2, 2), item(scene, 1, 1), item(scene, 3, 2)])
    assert st == tthip.TT_ERR_INVALID_ARG and "item 2" in why and "shares NodeOffset" in why and "item 0" in why


def test_parts_must_tile_the_mesh(scene):
    st, why = validate(scene, [item(scene, 1, 1, [0, 20, 50])])
    assert st == tthip.TT_OK
    it = item(scene, 1, 1, [0, 20, 50])
    it.parts[1].first_tri = 19  # overlaps part 0 and leaves the last triangle out
    it.parts[1].n_tris = 30
    st, why = validate(scene, [it])
    assert st == tthip.TT_ERR_INVALID_ARG and "overlaps" in why
    it = item(scene, 1, 1, [0, 20, 50])
    it.parts[0].n_tris = 19
    st, why = validate(scene, [it])
    assert st == tthip.TT_ERR_INVALID_ARG and "gap" in why and "[19, 20)" in why
    it = item(scene, 1, 1, [0, 20, 50])
    del it.parts[1]
    st, why = validate(scene, [it])
    assert st == tthip.TT_ERR_INVALID_ARG and "gap" in why and "[20, 50)" in why
    it = item(scene, 1, 1, [0, 20, 50])
    it.parts[1].n_tris = 31
    st, why = validate(scene, [it])
    assert st == tthip.TT_ERR_INVALID_ARG and "leave the mesh" in why


def test_triangle_range_beyond_the_scene(scene):
    sc, _, blases = scene
    # the last BLAS's record claiming more triangles than the scene holds behind its TriOffset
    n = len(sc.tris) - int(sc.meshdata["TriOffset"][3]) + 1
    it = item(scene, 3, 2, n_tris=n)
    st, why = validate(scene, [it])
    assert st == tthip.TT_ERR_INVALID_ARG and "exceeds the scene's triangles" in why


def test_root_that_is_not_the_first_node_is_unsupported(scene):
    sc = scene[0]
    md = sc.meshdata.copy()
    md["mesh_data_bvh_offsets"][1] += 1
    st, why = tthip.blas_refit_items_validate([item(scene, 1, 1)], md, len(sc.tris))
    assert st == tthip.TT_ERR_UNSUPPORTED and "root is not its first node" in why


def test_host_arrays_are_range_checked(scene):
    it = item(scene, 1, 1)
    it.parts[0].indices = it.parts[0].indices.copy()
    it.parts[0].indices[7] = it.parts[0].n_vertices
    st, why = validate(scene, [it])
    assert st == tthip.TT_ERR_INVALID_ARG and "index" in why and "out of range" in why
    assert validate(scene, [it], device=True)[0] == tthip.TT_OK  # device arrays are never read on the host
    it = item(scene, 1, 1)
    it.leaf_of_triangle = it.leaf_of_triangle.copy()
    it.leaf_of_triangle[4] = 50
    st, why = validate(scene, [it])
    assert st == tthip.TT_ERR_INVALID_ARG and "leaf_of_triangle[4]" in why


def test_total_triangle_limit(scene):
    sc = scene[0]
    hdr = open(os.path.join(REPO, "include", "truetrace_hip.h")).read()
    limit = int(re.search(r"#define TT_BLAS_REFIT_MANY_MAX_TRIS \(1u << (\d+)\)", hdr).group(1))
    md = sc.meshdata.copy()
    md["TriOffset"][:] = 0
    big = (1 << limit) // 2 + 1
    items = []
    for record, which in ((0, 0), (1, 1)):  # (device flag: the arrays are never read)
        it = item(scene, record, which, n_tris=big)
        it.parts[0].n_tris = big
        items.append(it)
    st, why = tthip.blas_refit_items_validate(items, md, 1 << 30, device=True)
    assert st == tthip.TT_ERR_INVALID_ARG and "item 1" in why and "triangles in all" in why


def test_the_checks_under_the_host_sanitizers(tmp_path):
    """csrc/tt_refit_items_host.h in a stand-alone program: every array exactly as long as the checks may read."""
    exe = tmp_path / "refit_items_kat"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "truetrace-unity-pathtracer_amd", "csrc"),
                    "-o", str(exe), os.path.join(REPO, "tests", "native", "refit_items_kat_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout and "runtime error" not in r.stderr


def test_bindings_carry_the_new_calls():
    L = tthip.hip_lib()
    for name in ("tt_blas_refit_many", "tt_blas_refit_items_validate"):
        assert hasattr(L, name) and name in tthip.HIP_SYMBOLS and getattr(L, name).argtypes is not None
    cs = open(os.path.join(REPO, "bindings", "csharp", "TrueTraceHip.cs")).read()
    assert "tt_blas_refit_many" in cs and "tt_blas_refit_items_validate" in cs
    # the ctypes mirrors have the C layout (LP64: pointers 8-aligned)
    assert C.sizeof(tthip.BlasRefitPart) == 96 and tthip.BlasRefitPart.transform.offset == 32
    assert C.sizeof(tthip.BlasRefitItem) == 40 and tthip.BlasRefitItem.local_to_world.offset == 32
