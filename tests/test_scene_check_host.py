"""The host scene checks (csrc/tt_scene_check_host.h) without a GPU: the library's answers on the differential
corpus (tests/scene_check_cases.py) byte for byte against the recorded answers of the commit before the three
hand-copied CWBVH walks became one, and the same corpus, the two-array (overlay) view, a lone walk_mesh and a lone
TLAS-level walk through a stand-alone program under the host sanitizers.

tests/golden/scene_check_parent.json was recorded from a build of that commit (the parent of the one that added
this file), from the repository root:

    git worktree add ../parent <this commit>^ && make -C ../parent/truetrace-unity-pathtracer_amd
    TT_HIP_LIB=../parent/truetrace-unity-pathtracer_amd/lib/libtruetrace_hip.so \\
        python tests/scene_check_cases.py tests/golden/scene_check_parent.json
"""
import collections
import dataclasses
import json
import os
import struct
import subprocess

import numpy as np

import assemble_cases as AC
import scene_check_cases as SC
import tthip

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
# every refusal of the scene walk, by the text that tells it from the others
SCENE_KINDS = ("node index", "triangle index", "TLAS leaf slot", "TLASBVH8Indices entry", "inner meta", "leaf meta spills",
               "negative mesh offsets")


def _golden():
    with open(os.path.join(HERE, "golden", "scene_check_parent.json")) as f:
        return json.load(f)


def test_the_recorded_corpus_meets_every_refusal_from_both_sides():
    g = _golden()["scene"]
    assert len(g) == len(SC.base_scenes()) * len(SC.SCENE_KINDS) * SC.PER_KIND >= 1050
    assert all((st == tthip.TT_OK) == (why == "") and st in (tthip.TT_OK, tthip.TT_ERR_INVALID_ARG) for _, st, why in g)
    hits = collections.Counter(k for _, _, why in g for k in SCENE_KINDS if why.startswith(k))
    assert sum(hits.values()) == sum(1 for _, st, _ in g if st != tthip.TT_OK)  # no refusal outside the seven kinds
    assert all(hits[k] >= 5 for k in SCENE_KINDS), hits
    assert 0.3 <= sum(1 for _, st, _ in g if st == tthip.TT_OK) / len(g) <= 0.7
    o = _golden()["object"]
    assert len(o) == 5 * len(SC.OBJECT_KINDS) * SC.PER_KIND
    assert 0.3 <= sum(1 for _, st, _ in o if st == tthip.TT_OK) / len(o) <= 0.7


def test_answers_are_the_parents_byte_for_byte():
    assert SC.answers() == _golden()


# ------------------------------------------------------------------ sanitizers
def _reach(nodes, root, node_offset=0):
    """The nodes IntersectBVH's child arithmetic reaches from `root`, in the order a LIFO stack that pushes a
    node's children in slot order pops them. For accepted inputs only: no index is checked."""
    seen, order, work = set(), [], [root]
    imask = nodes["e_imask"] >> 24
    meta = np.ascontiguousarray(nodes["meta"]).view(np.uint8).reshape(len(nodes), 8)
    while work:
        ni = work.pop()
        if ni in seen:
            continue
        seen.add(ni)
        order.append(ni)
        for m in meta[ni]:
            if (m & 0x18) == 0x18:
                before = int(imask[ni]) & ((1 << ((int(m) & 0x1F) - 24)) - 1)
                work.append((int(nodes["base_child"][ni]) + node_offset + bin(before).count("1")) & 0xFFFFFFFF)
    return order


def _keys(meshdata):
    return sorted({(int(r["mesh_data_bvh_offsets"]) & 0x7FFFFFFF, int(r["NodeOffset"]), int(r["TriOffset"])) for r in meshdata})


def _blas_reach(nodes, keys):
    return sorted({n for root, no, _ in keys for n in _reach(nodes, root, no)})


def _case(mode, s, ok, why, tl=None, n_tl=None, record=None):
    """One case of the program's file, and what an accepted one must report: (tlas_visit, BLAS nodes, keys)."""
    n_tl = len(s.nodes) if n_tl is None else n_tl
    why = why.encode()
    blob = struct.pack("<9I", mode, tl is not None, n_tl, len(s.nodes), len(s.tris), len(s.tlas), len(s.meshdata), ok, len(why))
    blob += why + (tl.tobytes() if tl is not None else b"") + s.nodes.tobytes() + s.tlas.astype("<i4").tobytes()
    blob += s.meshdata.tobytes() + (record.tobytes() if record is not None else b"")
    if not ok or mode == 3:
        return blob, None
    tlas_visit = _reach(s.nodes if tl is None else tl, 0) if mode in (0, 1) else []
    keys = _keys(s.meshdata) if mode == 0 else _keys(record) if mode == 2 else []
    return blob, (tlas_visit, _blas_reach(s.nodes, keys), keys if mode == 0 else [])


def _extra_cases():
    """The paths of the per-frame calls, on the assembled scene of assemble_cases."""
    _, s = AC.scene_s()
    n_tl, n_mesh = s.tlas_nodes, len(s.meshdata)
    assert 0 < n_tl < len(s.nodes)
    own = s.nodes[:n_tl].copy()
    out = [_case(1, s, 1, "", tl=own, n_tl=n_tl)]  # an overlay borrower: its TLAS copy, the lender's nodes
    past = own.copy()  # slot 7 of the root becomes an inner child one past the TLAS copy (popped first)
    AC.set_meta(past, 0, 7, (1 << 5) | 24)
    past["base_child"][0] = n_tl
    out.append(_case(1, s, 0, f"node index {n_tl} out of range of the context's own TLAS nodes", tl=past, n_tl=n_tl))
    # tt_scene_update_meshdata: record 0 re-pointed to the last record's BLAS, off the triangle array, below zero
    rec = s.meshdata[:1].copy()
    for f in ("NodeOffset", "TriOffset", "mesh_data_bvh_offsets"):
        rec[f] = s.meshdata[f][n_mesh - 1]
    assert _keys(rec) != _keys(s.meshdata[:1])
    out.append(_case(2, s, 1, "", record=rec))
    off = rec.copy()
    off["TriOffset"] = len(s.tris)
    out.append(_case(2, s, 0, "triangle index out of range", record=off))
    off = rec.copy()
    off["NodeOffset"] = -1
    out.append(_case(2, s, 0, "negative mesh offsets", record=off))
    # tt_scene_update_nodes, a TLAS-only rewrite: the TLAS level alone, good and with a leaf naming no mesh record
    out.append(_case(1, s, 1, ""))
    tl = s.tlas.copy()
    tl[0] = n_mesh
    out.append(_case(1, dataclasses.replace(s, tlas=tl), 0, "TLASBVH8Indices entry out of range"))
    return out


def test_scene_checks_under_sanitizers(tmp_path):
    """The stand-alone program (its own main, no Python in the run) built with ASan + UBSan over
    csrc/tt_scene_check_host.h: every answer as recorded, and what the accepted cases reached against _reach."""
    g = _golden()
    cases = [_case(0, s, st == tthip.TT_OK, why) for (_, s), (_, st, why) in zip(SC.scene_cases(), g["scene"])]
    cases += _extra_cases()
    for (_, nodes, tris), (_, st, why) in zip(SC.object_cases(), g["object"]):
        empty = np.zeros(0, tthip.MESH_DTYPE)
        obj = tthip.Scene(nodes, tris, np.zeros(0, np.int32), empty, empty)
        cases.append(_case(3, obj, st == tthip.TT_OK, why))
    path, reached = tmp_path / "cases.bin", tmp_path / "reached.txt"
    path.write_bytes(struct.pack("<I", len(cases)) + b"".join(b for b, _ in cases))
    exe = tmp_path / "scene_check_kat"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "truetrace-unity-pathtracer_amd", "csrc"),
                    "-o", str(exe), os.path.join(HERE, "native", "scene_check_kat_main.cpp")], check=True)
    r = subprocess.run([str(exe), str(path), str(reached)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(cases)} cases, 0 mismatches" in r.stdout and "runtime error" not in r.stderr
    got = {}
    for line in reached.read_text().splitlines():
        i, rest = line.split(" T", 1)
        t, rest = rest.split(" B")
        b, k = rest.split(" K")
        k = [int(x) for x in k.split()]
        got[int(i)] = ([int(x) for x in t.split()], [int(x) for x in b.split()], list(zip(k[0::3], k[1::3], k[2::3])))
    want = {i: w for i, (_, w) in enumerate(cases) if w is not None}
    assert len(want) > 700 and got == want
