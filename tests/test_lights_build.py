"""The light-BVH builders (tt_light_bvh_build_mesh / _tlas, tt_lights_assemble) against the float64 invariants of
tests/lights.py on the scenes of tests/lights_cases.py; determinism; and control mutants of the buffers, each of
which the model must report by name."""
import numpy as np
import pytest

import lights
import lights_cases as LC
import tthip


@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_build_invariants(name):
    case = LC.CASES[name]()
    rep = lights.check_build(case.lights, case.scene, case.parents, case.instances)
    print(name, "nodes checked", rep.nodes_checked, "full-sphere cones", rep.full_sphere)
    assert rep.ok, (rep.failed(), rep.box[:3], rep.cone[:3], rep.phi[:3], rep.tlas[:3], rep.rows[:3])
    assert rep.nodes_checked == sum(2 * len(t) - 1 for t, _ in case.parents)
    st, why = tthip.lights_validate(case.lights, case.scene.meshdata, len(case.scene.tris))
    assert st == tthip.TT_OK, why


def test_shapes_of_the_three_scenes():
    l1, l2, l3 = LC.l1_room(), LC.l2_single(), LC.l3_deep()
    assert [len(t) for t, _ in l1.parents] == [4, 37, 6] and len(l1.lights.meshes) == 4
    md = l1.scene.meshdata
    assert md["LightNodeOffset"][2] == md["LightNodeOffset"][3], "the two instances share one light tree"
    assert (md["LightNodeOffset"] % 2 == 0).all() and (md["LightNodeOffset"] >= 2 * 4).all()
    assert len(l2.lights.tris) == 1 and l2.lights.nodes["left"][0] == -1 and l2.lights.nodes["left"][2] == -1
    assert len(l3.lights.tris) == 1024
    assert lights.depth_below(l3.lights.nodes, int(l3.scene.meshdata["LightNodeOffset"][0]), 0) >= 10


@pytest.mark.parametrize("name", ["L1", "L3"])
def test_build_is_deterministic(name):
    case = LC.CASES[name]()
    md = case.scene.meshdata.copy()
    again = tthip.lights_assemble(case.parents, case.instances, md)
    assert again.nodes.tobytes() == case.lights.nodes.tobytes()
    assert again.tris.tobytes() == case.lights.tris.tobytes() and again.meshes.tobytes() == case.lights.meshes.tobytes()
    assert md.tobytes() == case.scene.meshdata.tobytes()


def test_a_tie_in_the_presort_keeps_index_order():
    """Two identical triangles: the stable presort puts the lower index first on every axis."""
    t = np.zeros(3, tthip.LIGHT_TRI_DTYPE)
    t["pos0"] = [(0, 0, 0), (0, 0, 0), (5, 0, 0)]
    t["posedge1"], t["posedge2"] = (1, 0, 0), (0, 0, 1)
    nodes, root = tthip.light_bvh_build_mesh(t, np.tile(np.float32([0, 1, 0]), (3, 1)))
    leaves = [(k, -(int(l) + 1)) for k, l in enumerate(nodes["left"]) if l < 0 and k != 1]
    order = [v for _, v in sorted(leaves)]
    assert order.index(0) < order.index(1)
    assert root["LightCount"][0] == 3 and abs(root["phi"][0] - 0.3) < 1e-6


def _mutants(case):
    L = case.lights
    off = int(case.scene.meshdata["LightNodeOffset"][1])  # the 37-triangle tree
    inner = [k for k in range(off, off + 2 * 37) if L.nodes["left"][k] >= 0 and (L.nodes["cosTheta_oe"][k] & 0xFFFF) not in (0, 32767)]
    leaves = [k for k in range(off, off + 2 * 37) if L.nodes["left"][k] < 0 and k != off + 1]

    def edit(fn):
        c = tthip.Lights(L.nodes.copy(), L.tris.copy(), L.meshes.copy())
        fn(c)
        return c

    def shrink(c):
        c.nodes["BBMax"][off] -= 0.05

    def narrow(c):
        k = inner[0]
        c.nodes["cosTheta_oe"][k] = (c.nodes["cosTheta_oe"][k] & 0xFFFF0000) | 32767  # cos_o = 1

    def drop(c):
        c.nodes["left"][leaves[0]] = c.nodes["left"][leaves[1]]

    def swap(c):
        c.meshes["StartIndex"][0], c.meshes["StartIndex"][1] = c.meshes["StartIndex"][1], c.meshes["StartIndex"][0]

    return {"box": edit(shrink), "cone": edit(narrow), "bijection": edit(drop), "rows": edit(swap)}


@pytest.mark.parametrize("mutant", ["box", "cone", "bijection", "rows"])
def test_control_mutants_are_reported_by_name(mutant):
    case = LC.l1_room()
    rep = lights.check_build(_mutants(case)[mutant], case.scene, case.parents, case.instances)
    assert mutant in rep.failed(), rep.failed()
