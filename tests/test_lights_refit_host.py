"""The light-BVH refit on the host: the pinned asin / acos / sin / cos against numpy float64, the float64 pin of
tests/lights_refit.py on tt_lights_refit_host's output over L1 / L2 / L3 x poses x both modes, its control mutants,
the call's refusals, and the bindings."""
import os
import re

import numpy as np
import pytest

import lights_cases as LC
import lights_refit as LR
import lights_refit_cases as RC
import tthip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONS = tthip.TT_LIGHT_REFIT_CONSERVATIVE


# ------------------------------------------------------------------ the pinned math
def _ulps(got, x, f):
    """|got - f(x)| in float32 ulps of the true value (x: the float32 arguments, f in float64)."""
    true = f(x.astype(np.float64))
    ulp = np.spacing(np.abs(true).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got.astype(np.float64) - true) / ulp))


@pytest.mark.parametrize("fn,f,lo,hi,ends", [
    ("asin", np.arcsin, -1.0, 1.0, [-1.0, 1.0, 0.5, -0.5, 0.708, np.sqrt(0.5), 1e-30]),
    ("acos", np.arccos, -1.0, 1.0, [-1.0, 1.0, 0.5, -0.5, 1.0 - 2.0 ** -24, -1.0 + 2.0 ** -24]),
    ("sin", np.sin, 0.0, np.pi, [np.pi, np.pi / 2, np.pi / 4, 3 * np.pi / 4, 3.14159, 1e-30]),
    ("cos", np.cos, 0.0, np.pi, [np.pi, np.pi / 2, np.pi / 4, 3 * np.pi / 4, 3.14159, 1e-30]),
])
def test_pinned_math_is_within_one_ulp_of_float64(fn, f, lo, hi, ends):
    """A double evaluation good to about 2^-40 rounds to one of the two floats around the true value: 1 ulp."""
    x = np.concatenate([np.linspace(lo, hi, 1_000_001), ends]).astype(np.float32)
    x = x[(x >= np.float32(lo)) & (x <= np.float32(hi)) & ((fn not in ("asin",)) | (x != 0))]
    worst = _ulps(tthip.light_refit_math(fn, x), x, f)
    print(f"{fn}: worst {worst:.4f} ulp over {len(x)} arguments")
    assert worst <= 1.0


def test_pinned_math_is_total():
    nan = np.float32(np.nan)
    for fn in ("asin", "acos"):
        out = tthip.light_refit_math(fn, [1.0000001, -1.0000001, 3.0, np.inf, nan])
        assert np.isnan(out).all()
    for fn in ("sin", "cos"):
        assert np.isnan(tthip.light_refit_math(fn, [np.inf, -np.inf, nan, 2.0 ** 21])).all()
        got = tthip.light_refit_math(fn, [-3.0, 7.5, 100.0, -1000.0])
        assert _ulps(got, np.float32([-3.0, 7.5, 100.0, -1000.0]), getattr(np, fn)) <= 1.0
    assert tthip.light_refit_math("asin", [0.0])[0] == 0 and tthip.light_refit_math("acos", [1.0])[0] == 0


# ------------------------------------------------------------------ the pin on the host reference
def test_scenes_have_the_shapes_the_refit_is_tested_on():
    l2, l3 = LC.l2_single(), LC.l3_deep()
    assert (l2.lights.nodes["left"][[0, int(l2.scene.meshdata["LightNodeOffset"][0])]] < 0).all()  # both trees one leaf
    off = int(l3.scene.meshdata["LightNodeOffset"][0])
    order, height = LR._bfs(l3.lights.nodes["left"], off)
    assert sum(1 for k in order if l3.lights.nodes["left"][k] < 0) == 1024 and height[off] >= 10  # four 256-thread blocks
    l1 = LC.l1_room()
    assert len(l1.lights.meshes) == 4 and RC.solid_offsets(l1)[2] == RC.solid_offsets(l1)[3]
    assert 37 in [int(n) for n in l1.scene.meshdata["LightTriCount"]]


@pytest.mark.parametrize("conservative", [False, True])
@pytest.mark.parametrize("pose", RC.POSES)
@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_host_reference_passes_the_pin(name, pose, conservative):
    case = LC.CASES[name]()
    deform = name in RC.DEFORMED
    after = RC.host_refit(name, pose, "both", deform, conservative)
    scene, records, x = RC.scenario(name, pose, "both", deform)
    rep = LR.pin(case.lights, after, scene, records, x, conservative)
    print("\n".join(rep.lines()))
    assert rep.ok, rep.lines()
    assert rep.leaves == len(case.lights.tris) and rep.tlas_leaves == len(case.lights.meshes)
    if name != "L2" and not conservative:
        assert rep.branch["union"] > 0
    if pose == "rotated" and not conservative:
        assert rep.abs_exception > 0, "no rotated instance pins the absolute-value exception"
    if conservative and name != "L2":
        assert rep.containment_checked > 0 and rep.containment_failures == 0


@pytest.mark.parametrize("part", ["mesh", "tlas"])
def test_one_pass_leaves_the_other_trees_alone(part):
    case = LC.l1_room()
    after = RC.host_refit("L1", "rotated", part, True)
    scene, records, x = RC.scenario("L1", "rotated", part, True)
    rep = LR.pin(case.lights, after, scene, records, x)
    assert rep.ok, rep.lines()
    assert (rep.leaves == 0) == (part == "tlas") and (rep.tlas_leaves == 0) == (part == "mesh")


def test_unreachable_slots_keep_their_bytes():
    case = LC.l1_room()
    poisoned = tthip.Lights(case.lights.nodes.copy(), case.lights.tris.copy(), case.lights.meshes)
    slots = [1] + [off + 1 for off in set(RC.solid_offsets(case))]
    poisoned.nodes.view(np.uint8).reshape(-1, 40)[slots] = 0xCD
    scene, records, x = RC.scenario("L1", "scaled", "both")
    after = tthip.lights_refit_host(poisoned, scene, records, x)
    assert (after.nodes.view(np.uint8).reshape(-1, 40)[slots] == 0xCD).all()
    assert LR.pin(poisoned, after, scene, records, x).ok


@pytest.mark.parametrize("mutant", sorted(LR.MUTANTS))
def test_every_mutant_of_the_model_is_reported_by_name(mutant):
    before = RC.varied_lights("L1")  # (leaves with different cosTheta_e codes: see there)
    scene, records, x = RC.scenario("L1", "rotated", "both", True)
    after = tthip.lights_refit_host(before, scene, records, x)
    if mutant == sorted(LR.MUTANTS)[0]:
        assert LR.pin(before, after, scene, records, x).ok
    rep = LR.pin(before, after, scene, records, x, mutant=mutant)
    print("\n".join(rep.lines()))
    assert LR.MUTANTS[mutant] in rep.failures, (mutant, rep.lines())


def test_refit_is_a_pure_function_of_the_leaves():
    """Refitting twice from the same inputs changes nothing, and the order of the listed records does not matter."""
    case = LC.l1_room()
    scene, records, x = RC.scenario("L1", "translated", "both", True)
    once = RC.host_refit("L1", "translated", "both", True)
    twice = tthip.lights_refit_host(once, scene, records[::-1], x)
    assert once.nodes.tobytes() == twice.nodes.tobytes() and once.tris.tobytes() == twice.tris.tobytes()


# ------------------------------------------------------------------ refusals
def _refused(case, scene, records, x):
    st, why, _ = tthip.lights_refit_host(case.lights, scene, records, x, check=False)
    return st, why


def test_refusals_name_the_index():
    case = LC.l1_room()
    x = RC.transforms("L1", "translated")
    md = case.scene.meshdata.copy()
    md["LightTriCount"][1] = 0
    st, why = _refused(case, RC.with_tris(case.scene, case.scene.tris, md), [0, 1], None)
    assert st == tthip.TT_ERR_INVALID_ARG and "mesh_indices[1]" in why and "LightTriCount" in why
    st, why = _refused(case, case.scene, [0, 2, 3], None)
    assert st == tthip.TT_ERR_INVALID_ARG and "mesh_indices[1]" in why and "mesh_indices[2]" in why
    st, why = _refused(case, case.scene, [], x[:3])
    assert st == tthip.TT_ERR_INVALID_ARG and "3 transforms for 4" in why
    for bad in (-1, len(case.lights.nodes)):
        y = x.copy()
        y["SolidOffset"][2] = bad
        st, why = _refused(case, case.scene, [], y)
        assert st == tthip.TT_ERR_INVALID_ARG and "transforms[2]" in why
    y = x.copy()
    y["SolidOffset"][0] = 2  # a TLAS node: in range, but no mesh tree's root
    st, why = _refused(case, case.scene, [], y)
    assert st == tthip.TT_ERR_INVALID_ARG and "transforms[0]" in why and "root of a mesh tree" in why
    st, why = _refused(case, case.scene, [9], None)
    assert st == tthip.TT_ERR_INVALID_ARG and "mesh_indices[0]" in why
    assert _refused(case, case.scene, [], None)[0] == tthip.TT_OK  # nothing to do is fine


def test_trees_that_share_a_node_are_refused():
    """tt_lights_validate looks at each light mesh alone; the refit's plan needs disjoint trees."""
    case = LC.l1_room()
    bad = RC.overlapping_lights()
    assert tthip.lights_validate(bad, case.scene.meshdata, len(case.scene.tris))[0] == tthip.TT_OK
    for records, x in (([0], None), ([], RC.transforms("L1", "translated")), ([], None)):
        st, why, out = tthip.lights_refit_host(bad, case.scene, records, x, check=False)
        assert st == tthip.TT_ERR_INVALID_ARG and "cannot be refitted" in why and "another tree" in why, why
        assert out.nodes.tobytes() == bad.nodes.tobytes()


# ------------------------------------------------------------------ bindings
def test_bindings_cover_the_new_calls():
    L = tthip.hip_lib()
    for name in ("tt_lights_refit", "tt_scene_read_light_nodes", "tt_scene_read_light_tris"):
        assert hasattr(L, name) and name in tthip.HIP_SYMBOLS and getattr(L, name).argtypes is not None
    for name in ("tt_lights_refit_host", "tt_light_refit_math"):
        assert name in tthip.SCENE_SYMBOLS and getattr(tthip.scene_lib(), name).argtypes is not None
    assert tthip.LIGHT_TRANSFORM_DTYPE.itemsize == 68 and tthip.LIGHT_TRANSFORM_DTYPE.fields["SolidOffset"][1] == 64
    hdr = open(os.path.join(REPO, "include", "truetrace_hip.h")).read()
    bit = int(re.search(r"TT_LIGHT_REFIT_CONSERVATIVE\s*=\s*1u\s*<<\s*(\d+)", hdr).group(1))
    assert CONS == 1 << bit
    taken = {int(b) for b in re.findall(r"TT_(?:TRACE|ENQUEUE|NEE)_\w+\s*=\s*1u\s*<<\s*(\d+)", hdr)}
    assert bit not in taken
    cs = open(os.path.join(REPO, "bindings", "csharp", "TrueTraceHip.cs")).read()
    assert re.search(r"LightRefitConservative\s*=\s*1u\s*<<\s*%d\b" % bit, cs)
    m = re.search(r"struct TTLightTransform\s*\{(.*?)\}", cs, re.S)
    assert m and "fixed float transform[16]" in m.group(1) and "int solidOffset" in m.group(1)
    for name in ("RefitLights", "ReadLightNodes", "ReadLightTris"):
        assert re.search(r"public unsafe void %s\(" % name, cs)


def test_transforms_are_column_major():
    m = np.arange(16, dtype=np.float64).reshape(4, 4)
    x = tthip.light_transforms([m], [6])
    assert x["Transform"][0][1 * 4 + 2] == m[2, 1] and x["SolidOffset"][0] == 6  # element (r, c) at [c * 4 + r]
