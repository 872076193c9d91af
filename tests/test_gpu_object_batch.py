"""Many meshes built into GPU-resident objects in one call (tt_objects_build_device: the forest forms of
csrc/tt_build.hip, the batched mesh passes of csrc/tt_object_build.hip). Every object must equal the host build of its
mesh (tthip.Blas: tt_blas_build) byte for byte -- nodes, leaf-ordered triangles, the leaf order, both info structs --
whatever else is in the call and in whatever order: mixed sizes from 1 to 20,001 triangles, the root small-sort
branches and the root-is-leaf form (n = 1..16), identical meshes side by side (no scan may cross a mesh boundary), a
mesh far deeper than its neighbours (bvh2_depth is per mesh), host presort lists for some meshes only, device-pointer
inputs, per-mesh lossy scales. A failure is all or nothing, names every declined mesh and leaves the context usable.
The objects are independent of each other. A control shows the comparison can fail."""
import numpy as np
import pytest

import assemble_cases as AC
import object_batch_cases as BC
import tthip

pytestmark = pytest.mark.gpu
C = tthip.C
OK, INVALID, UNSUPPORTED = tthip.TT_OK, tthip.TT_ERR_INVALID_ARG, tthip.TT_ERR_UNSUPPORTED


def _views(meshes, scales=None):
    vs = []
    for k, m in enumerate(meshes):
        v = m.view()
        v.lossy_scale[:] = (1.0, 1.0, 1.0) if scales is None else scales[k]
        vs.append(v)
    return vs


def _objects(engine, handles, infos):
    return [tthip.SceneObject(engine.L, h, build_info=tthip.ObjectBuildInfo.from_buffer_copy(i), engine=engine)
            for h, i in zip(handles, infos)]


def _host_presort(mesh):
    S = tthip.scene_lib()
    v = mesh.view()
    n = v.n_indices // 3
    aabbs, pre = np.zeros((n, 6), np.float32), np.zeros((3, n), np.int32)
    assert S.tt_blas_prepare_aabbs(C.byref(v), aabbs.ctypes.data) == OK
    assert S.tt_bvh2_presort(aabbs.ctypes.data, n, pre.ctypes.data) == OK
    return pre


def _check_all(objects, meshes, names=None):
    assert len(objects) == len(meshes)
    for k, (o, m) in enumerate(zip(objects, meshes)):
        BC.assert_equals_host_build(o, BC.host_build(m), f"mesh {k}" + (f" ({names[k]})" if names else ""))


# ------------------------------------------------------------------ 1: mixed sizes
def test_mixed_sizes_in_one_call_and_reversed(engine):
    names, meshes = list(BC.mixed().keys()), list(BC.mixed().values())
    objs = engine.build_objects(meshes)
    _check_all(objs, meshes, names)
    assert [o.build_info.presorted_on_host for o in objs] == [0] * len(meshes)
    rev = engine.build_objects(meshes[::-1])
    _check_all(rev, meshes[::-1], names[::-1])
    for a, b in zip(objs, rev[::-1]):
        for x, y in zip(a.read(), b.read()):
            assert x.tobytes() == y.tobytes()
    BC.destroy(objs + rev)


# ------------------------------------------------------------------ 2: tiny meshes
def test_tiny_meshes_in_one_call(engine):
    meshes = BC.tiny()
    assert len(meshes) == 135 and {len(m.arrays()[2]) // 3 for m in meshes} >= {1, 2, 3, 4, 16, 17}
    objs = engine.build_objects(meshes)
    _check_all(objs, meshes)
    assert all(o.build_info.presorted_on_host == 0 for o in objs)
    BC.destroy(objs)


# ------------------------------------------------------------------ 3: adjacent identical meshes
@pytest.mark.parametrize("name", ["pedestal", "signed_zeros", "single", "unity_cube"])
def test_adjacent_identical_meshes(engine, name):
    mx = BC.mixed()
    same = mx[name]
    meshes = [mx["soup_17"], same, same, same, mx["grid_40x25"]]
    objs = engine.build_objects(meshes)
    _check_all(objs, meshes)
    BC.destroy(objs)


# ------------------------------------------------------------------ 4: depth imbalance
@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_deep_mesh_among_shallow_ones_keeps_every_depth(engine, where):
    chain, soup600, soup17 = BC.chain(), tthip.Mesh.soup(31, 600, 1.0, 0.1), BC.mixed()["soup_17"]
    assert BC.host_build(chain).info.bvh2_depth == 25, "the chain is the deep mesh the case is about"
    assert BC.host_build(soup600).info.bvh2_depth < 16 and BC.host_build(soup17).info.bvh2_depth == 6
    meshes = [soup600, soup17]
    meshes.insert(where, chain)
    objs = engine.build_objects(meshes)
    assert [o.build_info.bvh2_depth for o in objs] == [BC.host_build(m).info.bvh2_depth for m in meshes]
    _check_all(objs, meshes)
    BC.destroy(objs)


# ------------------------------------------------------------------ 5: a batch of one
def test_a_batch_of_one_equals_the_single_call(engine):
    for name in ("soup_4097", "unity_cube"):  # the cube: the single call declines the device presort, the batch sorts it
        mesh = BC.mixed()[name]
        single = engine.build_object(mesh)
        (one,) = engine.build_objects([mesh])
        for x, y in zip(single.read(), one.read()):
            assert x.tobytes() == y.tobytes()
        a, b = single.build_info, one.build_info
        assert bytes(a)[:40] == bytes(b)[:40]  # everything but presorted_on_host
        assert (a.presorted_on_host, b.presorted_on_host) == ((1, 0) if name == "unity_cube" else (0, 0))
        assert bytes(single.info) == bytes(one.info)
        BC.assert_equals_host_build(one, BC.host_build(mesh), name)
        BC.destroy([single, one])


# ------------------------------------------------------------------ 6: host lists for some meshes
def test_host_presort_lists_for_some_meshes(engine):
    mx = BC.mixed()
    meshes = [mx["soup_17"], mx["pedestal"], mx["unity_cube"], mx["duplicates"], mx["single"], mx["soup_4097"]]
    supplied = [True, False, True, True, False, False]
    pre = [_host_presort(m) if s else None for m, s in zip(meshes, supplied)]
    st, hs, infos, status = engine.build_objects_raw(_views(meshes), pre)
    assert st == OK and status == [OK] * len(meshes), engine.L.tt_last_error(engine.h).decode()
    objs = _objects(engine, hs, infos)
    _check_all(objs, meshes)
    assert [o.build_info.presorted_on_host for o in objs] == [int(s) for s in supplied]
    BC.destroy(objs)


# ------------------------------------------------------------------ 7: a NaN position
def _nan_set(whole_vertex=False):
    """Mesh 3 of 5 has a NaN position: the y coordinate of triangle 40's first vertex.

    The case ends in a comparison with the host build, so the mesh has to be one the host builder builds. With one NaN
    coordinate it does: the triangle's box is NaN in y alone, its y centroid is NaN (the device presort declines the
    mesh), Extend skips the NaN component, and the triangle alone has the identity's y extent, a surface area of -inf and
    with it a split `cost <= float.MaxValue` accepts. With the whole vertex NaN (whole_vertex=True; the mesh of
    tests/test_gpu_object_build.py) the lone triangle's box is the identity, every split that isolates it costs +inf,
    and no builder goes on: the reference's partition_sah returns dimension -1 and indexes with it, tt_blas_build
    crashes the same way, the device builders decline in the BVH2 stage."""
    pos, _, idx = tthip.Mesh.soup(5, 100, 1.5, 0.35).arrays()
    if whole_vertex:
        pos[int(idx[3 * 40])] = np.nan
    else:
        pos[int(idx[3 * 40]), 1] = np.nan
    mx = BC.mixed()
    return [mx["soup_17"], mx["pedestal"], mx["single"], tthip.ArrayMesh(pos, idx), mx["grid_40x25"]], 3


@pytest.mark.parametrize("whole_vertex", [False, True])
def test_a_nan_position_is_declined_for_its_mesh_only(engine, whole_vertex):
    meshes, k = _nan_set(whole_vertex)
    live = engine.L.tt_stream_live_count()
    st, hs, infos, status = engine.build_objects_raw(_views(meshes))
    why = engine.L.tt_last_error(engine.h).decode()
    assert st == UNSUPPORTED and "presort" in why and f"mesh {k}" in why
    assert status == [UNSUPPORTED if m == k else OK for m in range(5)] and hs == [None] * 5
    assert engine.L.tt_stream_live_count() == live
    good = [m for j, m in enumerate(meshes) if j != k]  # the context is intact: a following call succeeds
    objs = engine.build_objects(good)
    _check_all(objs, good)
    BC.destroy(objs)


def test_a_nan_mesh_with_a_host_list_builds_and_equals_the_host_build(engine):
    """With a host list for mesh k the call succeeds and every object equals the host build, NaN words included
    (the edges from the NaN vertex: pass 2 subtracts as the host does). So does the single call's object."""
    meshes, k = _nan_set()
    pre = [None] * 5
    pre[k] = _host_presort(meshes[k])
    assert all(sorted(axis) == list(range(100)) for axis in pre[k].tolist()), "the host list is three permutations"
    st, hs, infos, status = engine.build_objects_raw(_views(meshes), pre)
    print("status", st, "mesh_status", status, engine.L.tt_last_error(engine.h).decode())
    assert st == OK and status == [OK] * 5
    objs = _objects(engine, hs, infos)
    _check_all(objs, meshes)
    assert [o.build_info.presorted_on_host for o in objs] == [int(m == k) for m in range(5)]
    nan_words = np.isnan(objs[k].read()[1]["posedge1"]).sum() + np.isnan(objs[k].read()[1]["posedge2"]).sum()
    assert nan_words == 2, "the comparison covered the NaN edges"
    single = engine.build_object(meshes[k])
    assert single.build_info.presorted_on_host == 1
    BC.assert_equals_host_build(single, BC.host_build(meshes[k]), "the single call")
    BC.destroy(objs + [single])


def _spy_on_raw_calls(engine, monkeypatch):
    calls, raw = [], engine.build_objects_raw

    def spy(views, presorted=None, flags=0):
        calls.append(None if presorted is None else [p is not None for p in presorted])
        return raw(views, presorted, flags)

    monkeypatch.setattr(engine, "build_objects_raw", spy)
    return calls


def test_build_objects_retries_declined_meshes_with_host_presorts(engine, monkeypatch):
    """Engine.build_objects retries the declined mesh itself: a second call with a host presort for that mesh and for
    no other, and the objects it returns equal the host builds."""
    meshes, k = _nan_set()
    calls = _spy_on_raw_calls(engine, monkeypatch)
    objs = engine.build_objects(meshes)
    assert calls == [None, [m == k for m in range(5)]]
    _check_all(objs, meshes)
    assert [o.build_info.presorted_on_host for o in objs] == [int(m == k) for m in range(5)]
    BC.destroy(objs)


def test_a_mesh_no_builder_builds_is_declined_again_after_the_retry(engine, monkeypatch):
    """A whole NaN vertex (see _nan_set): the retry is made, the BVH2 stage then declines the mesh, and what the
    builder says about it reaches the caller with its stage and mesh index, from the raw call and from
    Engine.build_objects; nothing is created and the engine goes on building."""
    meshes, k = _nan_set(whole_vertex=True)
    pre = [None] * 5
    pre[k] = _host_presort(meshes[k])
    st, hs, _, status = engine.build_objects_raw(_views(meshes), pre)
    why = engine.L.tt_last_error(engine.h).decode()
    assert st == UNSUPPORTED and "BVH2" in why and f"mesh {k}" in why
    assert status == [UNSUPPORTED if m == k else OK for m in range(5)] and hs == [None] * 5
    calls = _spy_on_raw_calls(engine, monkeypatch)
    with pytest.raises(tthip.TTError) as e:
        engine.build_objects(meshes)
    assert calls == [None, [m == k for m in range(5)]]
    assert e.value.status == UNSUPPORTED and "BVH2" in str(e.value) and f"mesh {k}" in str(e.value)
    monkeypatch.undo()
    objs = engine.build_objects(meshes[:k])  # and the engine goes on building
    _check_all(objs, meshes[:k])
    BC.destroy(objs)


# ------------------------------------------------------------------ 8: refusals
def _device_views(meshes):
    import torch

    keep, vs = [], []
    for m in meshes:
        v = m.view()
        for name, a in BC.view_arrays(m).items():
            if a is None:
                continue
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            keep.append(t)
            setattr(v, name, t.data_ptr())
        vs.append(v)
    torch.cuda.synchronize()
    return vs, keep


def test_an_index_equal_to_n_vertices_is_refused_for_its_mesh(engine):
    mx = BC.mixed()
    good = mx["soup_4097"]
    idx = good.indices.copy()
    idx[3 * 2222 + 1] = len(good.positions)
    bad = tthip.ArrayMesh(good.positions, idx, good.normals, good.tangents, good.uvs, good.matdat)
    meshes, k = [mx["soup_17"], mx["grid_40x25"], bad, mx["pedestal"]], 2
    dviews, keep = _device_views(meshes)  # (keep: the tensors behind the views)
    for views, flags in [(_views(meshes), 0), (dviews, tthip.TT_TRACE_DEVICE_PTRS)]:
        st, hs, _, status = engine.build_objects_raw(views, None, flags)
        why = engine.L.tt_last_error(engine.h).decode()
        assert st == INVALID and "index" in why and f"mesh {k}" in why
        assert status == [INVALID if m == k else OK for m in range(4)] and hs == [None] * 4
    objs = engine.build_objects([mx["soup_17"]])  # the context still builds
    _check_all(objs, [mx["soup_17"]])
    BC.destroy(objs)


def test_malformed_mesh_sets_are_refused_before_any_launch(engine):
    mx = BC.mixed()
    meshes = [mx["soup_17"], mx["pedestal"], mx["grid_40x25"]]
    vs = _views(meshes)
    vs[1].n_indices -= 1
    st, hs, _, status = engine.build_objects_raw(vs)
    assert (st, status, hs) == (INVALID, [OK, INVALID, OK], [None] * 3)
    assert "argument checks" in engine.L.tt_last_error(engine.h).decode()
    vs = _views(meshes)
    vs[0].positions = None
    vs[2].indices = None
    st, hs, _, status = engine.build_objects_raw(vs)
    assert (st, status, hs) == (INVALID, [INVALID, OK, INVALID], [None] * 3)
    assert "mesh 0" in engine.L.tt_last_error(engine.h).decode()
    st, hs, _, _ = engine.build_objects_raw([])
    assert st == INVALID and "argument checks" in engine.L.tt_last_error(engine.h).decode()
    pre = [None, _host_presort(meshes[1]), None]
    pre[1][2, 7] = 48  # pedestal has 48 triangles
    st, hs, _, status = engine.build_objects_raw(_views(meshes), pre)
    assert (st, status, hs) == (INVALID, [OK, INVALID, OK], [None] * 3)
    st, hs, _, _ = engine.build_objects_raw(_views(meshes), None, tthip.TT_TRACE_DEVICE_PTRS)  # host memory
    assert st == INVALID and hs == [None] * 3
    h = C.c_void_p()
    assert engine.L.tt_objects_build_device(None, None, 0, None, 0, C.byref(h), None, None) == INVALID
    objs = engine.build_objects(meshes)
    _check_all(objs, meshes)
    BC.destroy(objs)


# ------------------------------------------------------------------ 9: device pointers, per-mesh scales
def test_device_pointer_inputs_and_per_mesh_lossy_scales(engine):
    mx = BC.mixed()
    meshes = [mx["soup_17"], mx["grid_40x25"], mx["attributes_65_no_normals"], mx["soup_4097"]]
    scales = [(1.0, 1.0, 1.0), (2.0, 0.5, 4.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)]
    hosts = [BC.host_build(m, s if s != (1.0, 1.0, 1.0) else None) for m, s in zip(meshes, scales)]
    assert hosts[1].arrays()[0].tobytes() != BC.host_build(meshes[1]).arrays()[0].tobytes(), "the scale changes the boxes"
    objs = engine.build_objects(meshes, lossy_scales=scales)
    for k, (o, h) in enumerate(zip(objs, hosts)):
        BC.assert_equals_host_build(o, h, f"host arrays, mesh {k}")
    vs, keep = _device_views(meshes)
    for v, s in zip(vs, scales):
        v.lossy_scale[:] = s
    st, hs, infos, status = engine.build_objects_raw(vs, None, tthip.TT_TRACE_DEVICE_PTRS)
    assert st == OK and status == [OK] * 4, engine.L.tt_last_error(engine.h).decode()
    dev = _objects(engine, hs, infos)
    for k, (o, h) in enumerate(zip(dev, hosts)):
        BC.assert_equals_host_build(o, h, f"device arrays, mesh {k}")
    BC.destroy(objs + dev)


# ------------------------------------------------------------------ 10: independence
def test_objects_are_destroyed_in_any_order_while_the_rest_are_read(engine):
    names, meshes = list(BC.mixed().keys()), list(BC.mixed().values())
    objs = engine.build_objects(meshes)
    single = engine.build_object(meshes[names.index("pedestal")])
    assert objs[names.index("pedestal")].info.bytes == single.info.bytes
    single.destroy()
    order = np.random.default_rng(10).permutation(len(objs))
    alive = set(range(len(objs)))
    for k in order:
        objs[k].destroy()
        alive.discard(int(k))
        for j in sorted(alive)[:3] + sorted(alive)[-2:]:
            BC.assert_equals_host_build(objs[j], BC.host_build(meshes[j]), f"{names[j]} after destroying {names[k]}")


def test_batch_built_objects_assemble_trace_and_refit(engine):
    import torch

    import test_gpu_assemble as TA
    from test_blas_refit import deform, vertex_buffer

    am, s = AC.scene_s()
    meshes, blases = AC.meshes_and_blases()
    n_par = len(AC.PARENT_TRIS)
    A, B = tthip.Engine(0), engine
    try:
        A.upload(s)
        objects = B.build_objects(meshes)
        assert [o.build_info.presorted_on_host for o in objects] == [0] * len(meshes)
        am2 = tthip.AssetManager()  # AC.manager's scene, every BLAS a batch-built object
        for k, o in enumerate(objects[:n_par]):
            am2.add_parent_object(o, tthip.trs_matrix(AC.PARENT_POS[k % len(AC.PARENT_POS)], 20.0 * k), np.zeros(2, tthip.MAT_DTYPE))
        for o in objects[n_par:]:
            am2.add_instance_parent_object(o, np.zeros(1, tthip.MAT_DTYPE))
        for ip, pos in AC.INSTANCES:
            am2.add_instance(ip, tthip.trs_matrix(pos, 35.0 * (ip + 1), 1.25))
        s2, objs = am2.assemble_objects(B)
        (na, ta), (nb, tb) = TA.read_all(A, s), TA.read_all(B, s)
        assert nb.tobytes() == na.tobytes() == s.nodes.tobytes(), "assembled nodes differ from the upload"
        assert tb.tobytes() == ta.tobytes() == s.tris.tobytes(), "assembled triangles differ from the upload"
        fb = TA.frame(B)
        fo = TA.oracle_frame(s, fb["gen"])
        assert fo["nb"] == fb["nb"]
        assert np.array_equal(fb["rays"]["hits"][:TA.N + fb["nb"]], fo["rays"]["hits"][:TA.N + fo["nb"]])
        assert np.array_equal(fb["info"], fo["info"]) and TA.same_floats(fb["vis"], fo["vis"])
        assert (fb["rays"]["hits"][:TA.N, 1] != 0xFFFFFFFF).sum() > TA.N // 20, "the frame sees the scene"
        # tt_blas_refit through a batch-built object's device-resident leaf order, against a singly built one's
        single = B.build_object(meshes[2])
        assert np.array_equal(objects[2].read()[2], single.read()[2])
        pos, nrm, idx = meshes[2].arrays()
        V = vertex_buffer(deform(pos, 0.7), nrm)
        Vd, Id = torch.from_numpy(np.ascontiguousarray(V)).cuda(), torch.from_numpy(np.ascontiguousarray(idx)).cuda()
        torch.cuda.synchronize()
        B.blas_refit(2, Vd, Id, single.leaf_order_device, device=True)
        want = TA.read_all(B, s)
        am2.assemble_objects(B)  # the unrefitted scene again
        assert TA.read_all(B, s)[1].tobytes() == s.tris.tobytes()
        B.blas_refit(2, Vd, Id, objects[2].leaf_order_device, device=True)
        got = TA.read_all(B, s)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert got[1].tobytes() != s.tris.tobytes(), "the refit rewrote the mesh"
        A.blas_refit(2, V, idx, blases[2].leaf_order())  # and both equal the host leaf order's refit
        ha = TA.read_all(A, s)
        assert got[0].tobytes() == ha[0].tobytes() and got[1].tobytes() == ha[1].tobytes()
        single.destroy()
        BC.destroy(objects)
    finally:
        A.close()


# ------------------------------------------------------------------ 11: control
def test_control_a_neighbours_host_build_does_not_compare_equal(engine):
    names, meshes = list(BC.mixed().keys()), list(BC.mixed().values())
    objs = engine.build_objects(meshes)
    for m in range(len(meshes) - 1):
        assert BC.differences(objs[m], BC.host_build(meshes[m + 1])), f"{names[m]} compared equal to {names[m + 1]}"
    # and within one size: the same triangles without their normals differ in the triangle records alone
    a, b = names.index("attributes_65"), names.index("attributes_65_no_normals")
    assert BC.differences(objs[a], BC.host_build(meshes[b])) == ["leaf-ordered triangles"]
    BC.destroy(objs)
