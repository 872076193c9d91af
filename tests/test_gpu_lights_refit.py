"""tt_lights_refit on the device against its scalar host reference (tt_lights_refit_host), byte for byte, over L1 / L2 /
L3 x the poses of tests/lights_refit_cases.py x {mesh only, TLAS only, both} x {host pointers, device pointers,
asynchronous} x both modes; consecutive refits (the counter reset) and a refit after a restructured TLAS (the plan
rebuild); the float64 pin of tests/lights_refit.py on the device's output; the chain into tt_emit_nee, alone and
through a tt_ctx_share_scene borrower; and the refusals."""
import numpy as np
import pytest
import torch

import lights_cases as LC
import lights_refit as LR
import lights_refit_cases as RC
import tthip

pytestmark = pytest.mark.gpu

CONS = tthip.TT_LIGHT_REFIT_CONSERVATIVE
FORMS = ("host", "device", "async")


@pytest.fixture(scope="module")
def engines():
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    made = {name: tthip.Engine(0) for name in LC.CASES}
    yield made
    for e in made.values():
        e.close()


def fresh(e, case, lights=None, deform=None):
    """The case as uploaded, then (deform: a name) the deformed vertex set through tt_blas_refit."""
    e.upload(case.scene)
    e.upload_lights(lights or case.lights)
    if deform:
        rec, V, idx, leaf, scene = RC.deformed(deform)
        e.blas_refit(rec, V, idx, leaf)
        return scene
    return case.scene


def refit(e, records, x, form, flags=0):
    if form == "host":
        e.refit_lights(records, x, flags=flags)
    else:
        xd = None if x is None else torch.from_numpy(x.view(np.uint8).copy()).cuda()
        e.refit_lights(records, xd, device=True, asynchronous=form == "async", flags=flags)
        if form == "async":
            e.sync()


def read_back(e, lights):
    return tthip.Lights(e.read_light_nodes(0, len(lights.nodes)), e.read_light_tris(0, len(lights.tris)), lights.meshes)


def same(a, b):
    return a.nodes.tobytes() == b.nodes.tobytes() and a.tris.tobytes() == b.tris.tobytes()


@pytest.mark.parametrize("part", RC.PARTS)
@pytest.mark.parametrize("pose", RC.POSES)
@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_refit_equals_the_host_reference_in_every_form(engines, name, pose, part):
    e, case = engines[name], LC.CASES[name]()
    deform = name in RC.DEFORMED and part != "tlas"
    scene = fresh(e, case, deform=name if deform else None)
    if deform:
        off, end = LC._mesh_tri_range(case.scene, RC.DEFORMED[name])
        assert e.scene_tris(off, end - off).tobytes() == scene.tris[off:end].tobytes(), "tt_blas_refit differs from the oracle"
    _, records, x = RC.scenario(name, pose, part, deform)
    for conservative in (False, True):
        want = RC.host_refit(name, pose, part, deform, conservative)
        assert not same(want, case.lights)
        for form in FORMS:
            e.upload_lights(case.lights)
            refit(e, records, x, form, CONS if conservative else 0)
            got = read_back(e, case.lights)
            assert got.tris.tobytes() == want.tris.tobytes(), (form, conservative, "LightTriangles differ")
            bad = np.nonzero((got.nodes.view(np.uint8).reshape(-1, 40) != want.nodes.view(np.uint8).reshape(-1, 40)).any(1))[0]
            assert len(bad) == 0, (form, conservative, f"{len(bad)} nodes differ from tt_lights_refit_host, first {bad[:8]}")


def test_unreachable_slots_keep_their_upload_bytes(engines):
    e, case = engines["L1"], LC.l1_room()
    poisoned = tthip.Lights(case.lights.nodes.copy(), case.lights.tris.copy(), case.lights.meshes)
    slots = [1] + [off + 1 for off in set(RC.solid_offsets(case))]
    poisoned.nodes.view(np.uint8).reshape(-1, 40)[slots] = 0xCD
    scene = fresh(e, case, lights=poisoned)
    _, records, x = RC.scenario("L1", "scaled", "both")
    refit(e, records, x, "host")
    got = read_back(e, poisoned)
    assert (got.nodes.view(np.uint8).reshape(-1, 40)[slots] == 0xCD).all()
    assert same(got, tthip.lights_refit_host(poisoned, scene, records, x))


@pytest.mark.parametrize("name", ["L1", "L3"])
def test_two_refits_in_a_row_equal_the_host_reference_chained(engines, name):
    """The completing thread resets its counter: the second refit starts from zeros without a memset."""
    e, case = engines[name], LC.CASES[name]()
    fresh(e, case)
    _, records, xa = RC.scenario(name, "translated", "both")
    want = RC.host_refit(name, "translated", "both")
    refit(e, records, xa, "async")
    assert same(read_back(e, case.lights), want)
    rec, V, idx, leaf, scene = RC.deformed(name)
    e.blas_refit(rec, V, idx, leaf)
    xb = RC.transforms(name, "rotated")
    for form in ("device", "host"):  # the third refit repeats the second's inputs
        refit(e, records, xb, form, CONS)
        assert same(read_back(e, case.lights), tthip.lights_refit_host(want, scene, records, xb, CONS)), form


def test_refit_after_a_restructured_tlas_rebuilds_the_plan(engines):
    """A host-built TLAS of another shape with permuted instances, pushed through tt_scene_update_light_nodes."""
    e, case = engines["L1"], LC.l1_room()
    scene = fresh(e, case)
    _, records, x = RC.scenario("L1", "rotated", "both")
    refit(e, records, x, "host")  # a plan for the uploaded shape exists
    tl = case.lights.nodes[:8].copy()
    assert tl["left"][0] == 2
    chain = tl["left"][2] < 0 or tl["left"][3] < 0
    perm = [2, 0, 3, 1]
    if chain:  # two pairs instead
        lefts = {0: 2, 2: 4, 3: 6, 4: -(perm[0] + 1), 5: -(perm[1] + 1), 6: -(perm[2] + 1), 7: -(perm[3] + 1)}
    else:      # a chain instead
        lefts = {0: 2, 2: -(perm[0] + 1), 3: 4, 4: -(perm[1] + 1), 5: 6, 6: -(perm[2] + 1), 7: -(perm[3] + 1)}
    for k, v in lefts.items():
        tl["left"][k] = v
    assert not np.array_equal(tl["left"], case.lights.nodes["left"][:8])
    e.update_light_nodes(0, tl)
    host = tthip.Lights(case.lights.nodes.copy(), case.lights.tris.copy(), case.lights.meshes)
    host = tthip.lights_refit_host(host, scene, records, x)  # what the device held before the update ...
    host.nodes[:8] = tl                                      # ... with the new TLAS part over it
    y = RC.transforms("L1", "scaled")
    refit(e, records, y, "device")
    got = read_back(e, case.lights)
    want = tthip.lights_refit_host(host, scene, records, y)
    assert same(got, want)
    rep = LR.pin(host, got, scene, records, y)
    assert rep.ok and rep.tlas_leaves == 4, rep.lines()


@pytest.mark.parametrize("name,pose,conservative", [("L1", "rotated", False), ("L1", "rotated", True), ("L3", "scaled", False),
                                                    ("L3", "scaled", True), ("L2", "rotated", False)])
def test_the_pin_on_the_devices_output(engines, name, pose, conservative):
    e, case = engines[name], LC.CASES[name]()
    deform = name in RC.DEFORMED
    scene = fresh(e, case, deform=name if deform else None)
    _, records, x = RC.scenario(name, pose, "both", deform)
    refit(e, records, x, "device", CONS if conservative else 0)
    got = read_back(e, case.lights)
    rep = LR.pin(case.lights, got, scene, records, x, conservative)
    print("\n".join(rep.lines()))
    assert rep.ok, rep.lines()
    host = LR.pin(case.lights, RC.host_refit(name, pose, "both", deform, conservative), scene, records, x, conservative)
    assert rep.lines() == host.lines()


def test_the_chain_into_the_emit_and_a_borrower(engines):
    e, case = engines["L1"], LC.l1_room()
    fresh(e, case)
    rays, n, bounce, w, h = LC.ray_sets("L1")["b0"]
    kw = dict(frames=LC.FRAMES, max_bounce=LC.MAX_BOUNCE)

    def emit(eng):
        smp, sh = np.zeros(n, tthip.LIGHT_SAMPLE_DTYPE), np.zeros(n, tthip.SHADOW_DTYPE)
        cnt = eng.emit_nee(rays, n, bounce, LC.FAR, w, h, samples=smp, shadow_rays=sh, **kw)
        return smp, sh[:cnt]

    before_smp, before_sh = emit(e)
    mats = RC.pose_matrices("L1", "across")
    rec = int(case.lights.meshes["LockedMeshIndex"][2])
    md = case.scene.meshdata.copy()
    md["W2L"][rec] = tthip.unity_colmajor(np.linalg.inv(mats[2]))  # the emit reads the moved instance's W2L
    b = tthip.Engine(0)
    try:
        b.share_scene(e)
        e.update_meshdata(rec, md[rec:rec + 1])
        x = RC.transforms("L1", "across")
        e.refit_lights([], x, asynchronous=True)
        smp, sh = emit(b)  # the borrower's stream waits for the lender's refit
        lights = read_back(b, case.lights)
        assert same(lights, tthip.lights_refit_host(case.lights, case.scene, [], x))
        ref_smp, ref_sh = tthip.emit_nee_host(lights, RC.with_tris(case.scene, case.scene.tris, md), rays, n, bounce, LC.FAR, w, h, **kw)
        assert smp.tobytes() == ref_smp.tobytes() and sh.tobytes() == ref_sh.tobytes()
        own_smp, own_sh = emit(e)
        assert own_smp.tobytes() == ref_smp.tobytes() and own_sh.tobytes() == ref_sh.tobytes()
        assert smp.tobytes() != before_smp.tobytes() and len(sh) > 0 and len(before_sh) > 0
        with pytest.raises(tthip.TTError) as err:
            b.refit_lights([], x)
        assert err.value.status == tthip.TT_ERR_INVALID_ARG and "shared scene" in str(err.value)
    finally:
        b.close()


def test_refusals(engines):
    e, case = engines["L1"], LC.l1_room()
    fresh(e, case)
    x = RC.transforms("L1", "translated")

    def refused(status, *words, **kw):
        with pytest.raises(tthip.TTError) as err:
            e.refit_lights(**kw)
        assert err.value.status == status, str(err.value)
        for wd in words:
            assert wd in str(err.value), str(err.value)

    refused(tthip.TT_ERR_INVALID_ARG, "mesh_indices[1]", "mesh_indices[2]", mesh_indices=[0, 2, 3])
    refused(tthip.TT_ERR_INVALID_ARG, "3 transforms for 4", transforms=x[:3])
    y = x.copy()
    y["SolidOffset"][1] = len(case.lights.nodes)
    refused(tthip.TT_ERR_INVALID_ARG, "transforms[1]", transforms=y)
    y = x.copy()
    y["SolidOffset"][3] = 2  # a TLAS node: in range, but no mesh tree's root
    refused(tthip.TT_ERR_INVALID_ARG, "transforms[3]", "root of a mesh tree", transforms=y)
    refused(tthip.TT_ERR_INVALID_ARG, "mesh_indices[0]", mesh_indices=[99])
    refused(tthip.TT_ERR_INVALID_ARG, "not device memory", transforms=x, device=True)
    before = read_back(e, case.lights)
    assert same(before, case.lights), "a refused call wrote"
    # a record without light triangles
    md = case.scene.meshdata.copy()
    md["LightTriCount"][1] = 0
    e.upload(RC.with_tris(case.scene, case.scene.tris, md))
    e.upload_lights(case.lights)
    refused(tthip.TT_ERR_INVALID_ARG, "mesh_indices[1]", "LightTriCount", mesh_indices=[0, 1])
    # no lights; a frame slot
    e.upload(case.scene)
    refused(tthip.TT_ERR_NO_SCENE, mesh_indices=[0])
    with pytest.raises(tthip.TTError) as err:
        e.read_light_nodes(0, 1)
    assert err.value.status == tthip.TT_ERR_NO_SCENE
    e.upload_lights(case.lights)
    slot = tthip.Engine(0)
    try:
        slot.share_blas(e, case.scene.tlas_nodes)
        with pytest.raises(tthip.TTError) as err:
            slot.refit_lights([0])
        assert err.value.status == tthip.TT_ERR_UNSUPPORTED
    finally:
        slot.close()
    with pytest.raises(tthip.TTError) as err:
        e.read_light_tris(len(case.lights.tris), 1)
    assert err.value.status == tthip.TT_ERR_INVALID_ARG


def test_a_group_member_carries_no_lights(engines):
    import ctypes as C

    case = LC.l1_room()
    L = tthip.hip_lib()
    g = tthip.Group(64, 64, devices=[0, 0], copy=True)
    try:
        g.upload(case.scene)
        ctx = g.member_ctx(0)
        mi = np.array([0], np.uint32)
        x = RC.transforms("L1", "translated")
        for args in ((tthip._ptr(mi), 1, None, 0), (None, 0, tthip._ptr(x), len(x))):
            assert L.tt_lights_refit(ctx, *args, 0) == tthip.TT_ERR_UNSUPPORTED
            assert b"group" in L.tt_last_error(ctx)
        out = np.zeros(1, tthip.LIGHT_NODE_DTYPE)
        assert L.tt_scene_read_light_nodes(ctx, 0, 1, tthip._ptr(out)) == tthip.TT_ERR_NO_SCENE
        assert b"no lights" in L.tt_last_error(ctx)
        out = np.zeros(1, tthip.LIGHT_TRI_DTYPE)
        assert L.tt_scene_read_light_tris(ctx, 0, 1, tthip._ptr(out)) == tthip.TT_ERR_NO_SCENE
        assert C.c_char_p(L.tt_last_error(ctx)).value.startswith(b"tt_scene_read_light_tris")
    finally:
        g.close()


def test_trees_that_share_a_node_upload_but_do_not_refit(engines):
    """tt_lights_validate looks at each light mesh alone; a refit needs disjoint trees and says so before it writes."""
    e, case = engines["L1"], LC.l1_room()
    bad = RC.overlapping_lights()
    fresh(e, case, lights=bad)
    for kw in (dict(mesh_indices=[0]), dict(transforms=RC.transforms("L1", "translated"))):
        with pytest.raises(tthip.TTError) as err:
            e.refit_lights(**kw)
        assert err.value.status == tthip.TT_ERR_INVALID_ARG and "cannot be refitted" in str(err.value)
    assert same(read_back(e, bad), bad)
    fresh(e, case)
    e.refit_lights([0])  # the same context refits again once the lights are sound
