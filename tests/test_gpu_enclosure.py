"""The float64 enclosure model (tests/enclosure.py) on the bytes every node-writing kernel leaves in HBM, read back
through the accessors of the other GPU tests, with no oracle and no host builder in between: the BLAS refits
(NodeUpdate + NodeCompress), the device BLAS and object builds (k_fill8 and the object kernels), the TLAS refit, the
device TLAS build and the installation of a host-built one, and the on-device scene assembly.

Largest excess over a slot box seen on an MI355X, in units of U (enclosure.py), against the derived limits (2 U for
triangles, 1 U for instance boxes, 1 for the world level's ratio to its own limit):
  builder (tt_blas_build_device, tt_object_build_device, tt_objects_build_device, the assembled scene)  0.50 U
  refit (tt_blas_refit_many with general part transforms, tt_blas_refit)                                0.50 U
  TLAS (tt_tlas_refit on every quantiser edge and on moved instances, tt_tlas_rebuild, tt_scene_update_tlas)  0 U
  world level, mesh_aabbs written by tt_blas_refit_many under translations and under general matrices (kernel boxes:
  7 mag_r + inv_r)                                 0.10 and 0.09 of the limit (0.84 and 0.72 in units of 2^-24 mag_r)
  world level, the host-made mesh_aabbs of the scene of device-built objects and of assemble_cases' scene S (host
  boxes: 9 mag_r + inv_r)                          0.15 and 0.09 of the limit (1.49 and 0.94 in units of 2^-24 mag_r)
The tests print the figures of the run (pytest -s)."""
import numpy as np
import pytest

import assemble_cases as AC
import enclosure as E
import enclosure_cases as EC
import refit_many_cases as R
import tlas_rebuild_cases as T
import tthip

pytestmark = pytest.mark.gpu


def _say(name, rep):
    print(f"{name}: {rep.n_slots} slots, worst {rep.ratio:.3f} U of {rep.limit} ({rep.worst})")
    return rep


def _read(e, n_nodes, n_tris):
    return e.scene_nodes(0, n_nodes), e.scene_tris(0, n_tris)


# ------------------------------------------------------------------ BLAS refits
def test_blas_refit_many_and_blas_refit(engine):
    c = R.case()
    sc = c.sc
    layouts = [R.Layout(r, R.vertices(r, 2.1), cuts, strides=(6, 10),
                        transforms=[R.general_matrix(r + 2 * k) for k in range(len(cuts) - 1)], reverse=r % 2 == 0)
               for r, cuts in zip(R.RECORDS, R.CUTS)]
    engine.upload(sc)
    boxes = np.ascontiguousarray(sc.meta["mesh_aabbs"], np.float32).copy()
    engine.blas_refit_many([L.item(c.l2w[L.record]) for L in layouts], mesh_aabbs=boxes)
    engine.tlas_refit(sc.tlas_nodes, boxes)
    nodes, tris = _read(engine, len(sc.nodes), len(sc.tris))
    assert not np.array_equal(nodes, sc.nodes) and not np.array_equal(tris, sc.tris)
    reps = E.scene(nodes, tris, sc.tlas, sc.meshdata, boxes, sc.tlas_nodes, "tt_blas_refit_many")
    assert len(reps) == 1 + 7
    for k, r in reps.items():
        _say(k, r)
    E.check_all(reps)
    ratio, plain, where = E.world_level(boxes, sc.meshdata, tris, E.KERNEL_BOX, records=R.RECORDS)
    print(f"world level: worst excess {ratio:.3f} of its limit, {plain:.3f} x 2^-24 mag, at (record, axis, side) {where}")
    assert ratio <= E.LIMIT_WORLD
    # general local_to_world matrices (the scene's are translations): the boxes of the pinned corner chain against
    # the world triangles through inv(float32 W2L), W2L what a host would put into _MeshData for these matrices
    gen = {L.record: R.general_matrix(5 + L.record) for L in layouts}
    md = sc.meshdata.copy()
    for r, m in gen.items():
        md["W2L"][r] = tthip.unity_colmajor(np.linalg.inv(m))
    boxes_gen = boxes.copy()
    engine.blas_refit_many([L.item(gen[L.record]) for L in layouts], mesh_aabbs=boxes_gen)
    assert not np.array_equal(boxes_gen[1:], boxes[1:])
    ratio, plain, where = E.world_level(boxes_gen, md, engine.scene_tris(0, len(sc.tris)), E.KERNEL_BOX, records=R.RECORDS)
    print(f"world level, general matrices: worst excess {ratio:.3f} of its limit, {plain:.3f} x 2^-24 mag, at {where}")
    assert ratio <= E.LIMIT_WORLD
    # tt_blas_refit (blas_construct and refit_tree, kernels of its own) on every mesh: one node, a just-needed second
    # level, leaf pairs ending inside a 256-thread block (300, 600), several blocks
    for r in R.RECORDS:
        L = R.Layout(r, R.vertices(r, 0.9), [0, c.blases[r].n_tris])
        engine.blas_refit(r, L.parts[0].vertices, L.parts[0].indices, L.leaf, R.general_matrix(7 + r))
    nodes2, tris2 = _read(engine, len(sc.nodes), len(sc.tris))
    assert not np.array_equal(nodes2, nodes)
    reps = E.scene(nodes2, tris2, sc.tlas, sc.meshdata, boxes, sc.tlas_nodes, "tt_blas_refit")
    for r in R.RECORDS:
        at = slice(int(sc.meshdata["TriOffset"][r]), int(sc.meshdata["TriOffset"][r]) + c.blases[r].n_tris)
        assert not np.array_equal(tris2[at], tris[at]), f"record {r} was not refit"
        _say(f"blas{r}", reps[f"blas{r}"]).check()


# ------------------------------------------------------------------ TLAS refit
@pytest.mark.parametrize("n", EC.EDGE_SIZES)
def test_tlas_refit_on_the_quantiser_edges(engine, n):
    sc = EC.edge_scene(n)
    engine.upload(sc)
    worst = 0.0
    for name, boxes in EC.edge_boxes(n):
        engine.tlas_refit(sc.tlas_nodes, boxes)
        nodes = engine.scene_nodes(0, sc.tlas_nodes)
        rep = E.tlas(nodes, sc.tlas, boxes, sc.tlas_nodes, f"tt_tlas_refit, {n} instances, {name}").check()
        worst = max(worst, rep.ratio)
    print(f"{n} instances, {len(EC.edge_boxes(n))} edge cases: worst {worst:.3f} U")
    # the kept finding: a box with BBMax.x < -10000 is the refit's empty slot
    boxes = EC.far_box_case(n)
    engine.tlas_refit(sc.tlas_nodes, boxes)
    rep = E.tlas(engine.scene_nodes(0, sc.tlas_nodes), sc.tlas, boxes, sc.tlas_nodes, "far box")
    at = int(np.nonzero(sc.tlas == 3)[0][0])
    assert not rep.structure and rep.slots_over() == {tuple(int(x) for x in rep.item_slot[at])}, rep.describe()


def test_tlas_refit_after_moving_every_instance(engine):
    a = T.base_scene(EC.SEED_40, 40)
    md, boxes = T.moved_pose(a, 7)
    engine.upload(a)
    engine.update_meshdata(0, md)
    engine.tlas_refit(a.tlas_nodes, boxes)
    nodes = engine.scene_nodes(0, len(a.nodes))
    assert not np.array_equal(nodes[:a.tlas_nodes], a.nodes[:a.tlas_nodes])
    reps = E.scene(nodes, engine.scene_tris(0, len(a.tris)), a.tlas, md, boxes, a.tlas_nodes, "moved")
    _say("tlas", reps["tlas"])
    E.check_all(reps)


# ------------------------------------------------------------------ TLAS rebuild and installation
def test_tlas_rebuild_on_the_device_and_install_of_a_host_build():
    import torch

    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    a = T.base_scene(EC.SEED_40, 40)
    e = tthip.Engine(0)
    try:
        e.upload(a)
        for route, perm_seed in (("device", 5), ("host", 6), ("device pointers", 8)):
            md, boxes = T.permuted_pose(EC.SEED_40, 40, perm_seed)
            e.update_meshdata(0, md)
            if route == "host":
                built, built_idx = tthip.tlas_build(boxes)
                e.update_tlas(built, built_idx)
                n = len(built)
            elif route == "device":
                n = e.tlas_rebuild(boxes)
            else:
                n = e.tlas_rebuild(torch.from_numpy(boxes).to("cuda:0"), device=True)
            nodes, tris = _read(e, len(a.nodes), len(a.tris))
            idx = e.scene_tlas_indices(0, len(a.tlas))
            assert sorted(idx.tolist()) == list(range(len(md))), "the rebuilt TLASBVH8Indices"
            reps = E.scene(nodes, tris, idx, md, boxes, n, route)
            _say(route, reps["tlas"])
            assert reps["tlas"].n_slots >= len(md)
            E.check_all(reps)
    finally:
        e.close()


# ------------------------------------------------------------------ builds on the device
@pytest.mark.parametrize("name", list(EC.build_meshes()))
def test_blas_and_object_build_on_the_device(engine, name):
    mesh = EC.build_meshes()[name]
    nodes, tris = tthip.Blas(mesh, engine=engine).arrays()
    _say("tt_blas_build_device " + name, E.blas(nodes, tris, what=name)).check()
    obj = engine.build_object(mesh)
    try:
        nodes, tris, leaf = obj.read()
        assert sorted(leaf.tolist()) == list(range(len(tris)))
        rep = _say("tt_object_build_device " + name, E.blas(nodes, tris, what=name)).check()
        assert (rep.item_slot[:, 0] >= 0).all()
    finally:
        obj.destroy()


def _object_manager(objects):
    """The six build meshes' objects as three parents, three instance parents and five instances under rotations and
    scales. A scene of its own beside assemble_cases.scene_s (below): its BLASes are the device-built objects of the
    sizes this file pins (1 .. 5,000 triangles and the coplanar grid), which scene S does not hold."""
    am = tthip.AssetManager()
    for k, o in enumerate(objects[:3]):
        am.add_parent_object(o, tthip.trs_matrix((3.0 * k, 0.5 * k, -1.0), 20.0 * k, 1.0 + 0.5 * k), np.zeros(2, tthip.MAT_DTYPE))
    for o in objects[3:]:
        am.add_instance_parent_object(o, np.zeros(1, tthip.MAT_DTYPE))
    for i, ip in enumerate((0, 1, 2, 1, 0)):
        am.add_instance(ip, tthip.trs_matrix((-4.0 + 2.5 * i, 0.25 * i, 3.0 + i), 35.0 * (i + 1), 0.5 + 0.25 * i))
    return am


def _walk_assembled(engine, s, n_nodes, n_tris, n_blas, what):
    """The whole assembled scene as the device holds it, from the TLAS root through every record's BLAS under its
    NodeOffset / TriOffset, and the world level of the host-made mesh_aabbs."""
    nodes, tris = _read(engine, n_nodes, n_tris)
    boxes = s.meta["mesh_aabbs"]
    reps = E.scene(nodes, tris, engine.scene_tlas_indices(0, len(s.tlas)), s.meshdata, boxes, s.tlas_nodes, what)
    assert len(reps) == 1 + n_blas
    for k, r in reps.items():
        _say(k, r)
    E.check_all(reps)
    assert sum(r.n_slots for k, r in reps.items() if k != "tlas") >= n_tris // 3
    ratio, plain, where = E.world_level(boxes, s.meshdata, tris, E.HOST_BOX)
    print(f"{what}, world level: worst excess {ratio:.3f} of its limit, {plain:.3f} x 2^-24 mag, at (record, axis, side) {where}")
    assert ratio <= E.LIMIT_WORLD


def test_batched_object_build_and_the_assembled_scene(engine):
    objects = engine.build_objects(list(EC.build_meshes().values()))
    try:
        for name, o in zip(EC.build_meshes(), objects):
            nodes, tris, _ = o.read()
            _say("tt_objects_build_device " + name, E.blas(nodes, tris, what=name)).check()
        s, _ = _object_manager(objects).assemble_objects(engine)
        n_nodes, n_tris = s.meta["n_nodes_total"], s.meta["n_tris_total"]
        assert n_tris == sum(len(o.read()[1]) for o in objects)
        _walk_assembled(engine, s, n_nodes, n_tris, 6, "device-built objects")
    finally:
        for o in objects:
            o.destroy()


def test_assemble_cases_scene_s_assembled_on_the_device(engine):
    """Scene S of tests/assemble_cases.py (1, 65, 4,097, 63 and 373 triangles; odd prefix sums), gathered on the device
    from one object per host-built BLAS."""
    am, s = AC.scene_s()
    objects = [engine.create_object(b) for b in am.blases()]
    try:
        s2, _ = am.assemble(engine, objects)
        _walk_assembled(engine, s2, len(s.nodes), len(s.tris), 5, "scene S")
    finally:
        for o in objects:
            o.destroy()
