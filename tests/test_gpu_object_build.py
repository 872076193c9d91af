"""A mesh built into a GPU-resident object on the device (tt_object_build_device, csrc/tt_object_build.hip): what
tt_object_read returns must equal the host build (tthip.Blas: tt_blas_build) byte for byte -- nodes, leaf-ordered
triangles, the leaf order, aabb_untransformed as bit patterns and the BVH2 depth -- for meshes that reach every path:
the host-presort retry (n <= 16), the first size the device presort takes (17), flat boxes that Validate pads,
tie-heavy and signed-zero inputs (an order-dependent root box shows there), several blocks and introsort levels, an
88-byte tail at an 8-byte aligned end (odd counts), every nullable attribute absent in turn, degenerate normals, and
device-pointer inputs. Scene S assembled from device-built objects under tt_scene_assemble_tlas must hold what
tt_scene_upload of AssetManager.build() holds and trace the oracle's frame. Bad inputs are refused with nothing
created, and the engine goes on working."""
import functools
import os

import numpy as np
import pytest

import assemble_cases as AC
import oracle_ctypes as O
import tthip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
C = tthip.C


def _grid(nx, nz):  # a flat grid of quads (y = 0): every box is padded by Validate, every SAH sweep full of ties
    xs, zs = np.meshgrid(np.arange(nx + 1, dtype=np.float32), np.arange(nz + 1, dtype=np.float32), indexing="ij")
    pos = np.stack([xs.ravel(), np.zeros(xs.size, np.float32), zs.ravel()], 1)
    idx = []
    for i in range(nx):
        for j in range(nz):
            a, b, c, d = i * (nz + 1) + j, (i + 1) * (nz + 1) + j, i * (nz + 1) + j + 1, (i + 1) * (nz + 1) + j + 1
            idx += [a, b, c, c, b, d]
    return tthip.ArrayMesh(pos, np.array(idx, np.int32))


def _with_attributes(mesh, seed):
    """The mesh's positions and indices with random normals, tangents, uvs and MatDat."""
    pos, _, idx = mesh.arrays()
    rng = np.random.default_rng(seed)
    nv = len(pos)
    return tthip.ArrayMesh(pos, idx, normals=rng.normal(size=(nv, 3)), tangents=rng.normal(size=(nv, 4)),
                           uvs=rng.random((nv, 2)) * 4 - 2, matdat=rng.integers(0, 5, len(idx) // 3))


def _attributes_65():
    """65 triangles whose normals are degenerate in every way normalized() and PackOctahedral distinguish."""
    pos, _, idx = tthip.Mesh.soup(77, 65, 1.5, 0.35).arrays()
    rng = np.random.default_rng(65)
    nv = len(pos)
    nrm = rng.normal(size=(nv, 3)).astype(np.float32)
    nrm[0::7] = 0.0                                    # zero length: normalized -> 0, the pack divides 0 by 0
    nrm[1::7] = np.float32([1e-6, 0.0, 0.0])           # below normalized()'s 1e-5 threshold
    nrm[2::7] = np.float32([6e-6, 6e-6, 6e-6])         # magnitude just above it
    nrm[3::7, 2] = -np.abs(nrm[3::7, 2]) - 0.1         # z < 0: the octahedral fold
    nrm[4::7, 0] = -0.0                                # -0 components (x >= 0 holds for -0)
    nrm[5::7] = np.float32([-0.0, -0.0, -1.0])
    tan = rng.normal(size=(nv, 4)).astype(np.float32)
    tan[0::5, :3] = 0.0
    tan[1::5, 1] = -0.0
    return dict(positions=pos, indices=idx, normals=nrm, tangents=tan,
                uvs=(rng.random((nv, 2)) * 8 - 4).astype(np.float32), matdat=(np.arange(65) % 8).astype(np.int32))


@functools.lru_cache(maxsize=None)
def _meshes():
    z = np.load(os.path.join(HERE, "golden", "pedestal_mesh.npz"))
    cube = np.load(os.path.join(HERE, "golden", "unity_cube_pins.npz"))
    rng = np.random.default_rng(7)  # the tie-heavy inputs of tests/test_gpu_builder.py, restated
    dup = rng.random((300, 3), dtype=np.float32) * 4 - 2
    dup_pos = np.concatenate([dup, dup, np.round(dup)])  # duplicated and snapped triangles
    signed = rng.integers(-2, 3, (600, 3)).astype(np.float32)
    signed[rng.random(signed.shape) < 0.3] = -0.0  # -0 and +0 coordinates
    a65 = _attributes_65()
    m = {
        "single": tthip.ArrayMesh(np.eye(3, dtype=np.float32), np.array([0, 1, 2], np.int32)),
        "unity_cube": tthip.ArrayMesh(cube["cube_v"], cube["cube_i"]),
        "soup_17": tthip.Mesh.soup(21, 17, 1.5, 0.35),
        "pedestal": tthip.ArrayMesh(z["positions"].astype(np.float32), z["indices"]),
        "grid_40x25": _grid(40, 25),
        "duplicates": tthip.ArrayMesh(dup_pos, np.arange(len(dup_pos), dtype=np.int32)),
        "signed_zeros": tthip.ArrayMesh(signed, np.arange(600, dtype=np.int32)),
        "soup_4097": _with_attributes(tthip.Mesh.soup(1002, 4097, 1.5, 0.35), 1),
        "soup_20001": _with_attributes(tthip.Mesh.soup(31, 20001, 3.0, 0.2), 2),
        "attributes_65": tthip.ArrayMesh(**a65),
    }
    for drop in ("normals", "tangents", "uvs", "matdat"):
        m["attributes_65_no_" + drop] = tthip.ArrayMesh(**{k: v for k, v in a65.items() if k != drop})
    return m


HOST_PRESORT = {"single", "unity_cube"}  # n <= 16: the device presort declines, build_object retries


def _bits(a):
    return np.array(list(a), np.float32).view(np.uint32).tolist()


def _assert_equals_host_build(obj, blas):
    nodes, tris, leaf = obj.read()
    hn, ht = blas.arrays()
    assert nodes.tobytes() == hn.tobytes(), "CWBVH8 nodes differ"
    assert len(tris) == len(ht)
    bad = np.nonzero((tris.view(np.uint8).reshape(-1, 88) != ht.view(np.uint8).reshape(-1, 88)).any(1))[0]
    assert bad.size == 0, f"{bad.size} leaf-ordered triangles differ, first at {bad[:4]}: {tris[bad[:1]]} vs {ht[bad[:1]]}"
    assert np.array_equal(leaf, blas.leaf_order()), "leaf order differs"
    bi, hi = obj.build_info, blas.info
    assert (bi.n_nodes, bi.n_tris, bi.bvh2_depth) == (hi.n_nodes, hi.n_tris, hi.bvh2_depth)
    assert _bits(bi.aabb_min) == _bits(hi.aabb_min) and _bits(bi.aabb_max) == _bits(hi.aabb_max), "aabb_untransformed"
    assert bi.max_matdat == int(ht["MatDat"].max())
    i = obj.info
    assert (i.n_nodes, i.n_tris, i.root) == (hi.n_nodes, hi.n_tris, 0)
    return nodes, tris, leaf


@pytest.mark.parametrize("name", list(_meshes().keys()))
def test_built_object_equals_the_host_build(engine, name):
    mesh = _meshes()[name]
    obj = engine.build_object(mesh)
    _assert_equals_host_build(obj, tthip.Blas(mesh))
    assert obj.build_info.presorted_on_host == (1 if name in HOST_PRESORT else 0)
    obj.destroy()


def test_flat_grid_with_a_lossy_scale(engine):
    """ParentScale = 0.001 / lossyScale per axis: the y padding of the flat grid is 0.002 here."""
    mesh, scale = _meshes()["grid_40x25"], (2.0, 0.5, 4.0)
    obj = engine.build_object(mesh, lossy_scale=scale)
    _assert_equals_host_build(obj, tthip.Blas(mesh, lossy_scale=scale))
    assert _bits(obj.build_info.aabb_max)[1] == _bits([np.float32(0.001) / np.float32(0.5)])[0]
    obj.destroy()


def test_device_pointer_inputs_give_the_same_bytes(engine):
    import torch

    mesh = _meshes()["soup_4097"]
    host = engine.build_object(mesh)
    dev = {k: torch.from_numpy(getattr(mesh, k)).cuda() for k in ("positions", "normals", "tangents", "uvs", "indices", "matdat")}
    torch.cuda.synchronize()
    obj = engine.build_object(mesh, device_arrays=dev)
    for a, b in zip(obj.read(), host.read()):
        assert a.tobytes() == b.tobytes()
    _assert_equals_host_build(obj, tthip.Blas(mesh))
    assert obj.build_info.presorted_on_host == 0
    dev.pop("normals")  # nullable arrays stay nullable with device pointers
    obj2 = engine.build_object(mesh, device_arrays=dev)
    no_normals = tthip.ArrayMesh(mesh.positions, mesh.indices, None, mesh.tangents, mesh.uvs, mesh.matdat)
    _assert_equals_host_build(obj2, tthip.Blas(no_normals))
    for o in (host, obj, obj2):
        o.destroy()


# ------------------------------------------------------------------ scene S from device-built objects
def test_device_built_objects_assemble_and_trace(engine):
    import torch

    import test_gpu_assemble as TA
    from test_blas_refit import deform, vertex_buffer

    am, s = AC.scene_s()
    meshes, blases = AC.meshes_and_blases()
    n_par = len(AC.PARENT_TRIS)
    A, B = tthip.Engine(0), engine
    try:
        A.upload(s)
        objects = [B.build_object(m) for m in meshes]
        assert [o.build_info.presorted_on_host for o in objects] == [1, 0, 0, 0, 0]
        am2 = tthip.AssetManager()  # AC.manager's scene, every BLAS a device-built object
        for k, o in enumerate(objects[:n_par]):
            am2.add_parent_object(o, tthip.trs_matrix(AC.PARENT_POS[k % len(AC.PARENT_POS)], 20.0 * k), np.zeros(2, tthip.MAT_DTYPE))
        for o in objects[n_par:]:
            am2.add_instance_parent_object(o, np.zeros(1, tthip.MAT_DTYPE))
        for ip, pos in AC.INSTANCES:
            am2.add_instance(ip, tthip.trs_matrix(pos, 35.0 * (ip + 1), 1.25))
        s2, objs = am2.assemble_objects(B)
        region = 2 * len(s.meshdata)
        assert s2.nodes.tobytes() == s.nodes[:region].tobytes() and len(s2.tris) == 0
        assert np.array_equal(s2.tlas, s.tlas) and s2.meshdata.tobytes() == s.meshdata.tobytes()
        assert (s2.meta["n_nodes_total"], s2.meta["n_tris_total"]) == (len(s.nodes), len(s.tris))
        (na, ta), (nb, tb) = TA.read_all(A, s), TA.read_all(B, s)
        assert nb.tobytes() == na.tobytes() == s.nodes.tobytes(), "assembled nodes differ from the upload"
        assert tb.tobytes() == ta.tobytes() == s.tris.tobytes(), "assembled triangles differ from the upload"
        fb = TA.frame(B)
        fo = TA.oracle_frame(s, fb["gen"])
        assert fo["nb"] == fb["nb"]
        assert np.array_equal(fb["rays"]["hits"][:TA.N + fb["nb"]], fo["rays"]["hits"][:TA.N + fo["nb"]])
        assert np.array_equal(fb["info"], fo["info"]) and TA.same_floats(fb["vis"], fo["vis"])
        assert (fb["rays"]["hits"][:TA.N, 1] != 0xFFFFFFFF).sum() > TA.N // 20, "the frame sees the scene"
        # tt_blas_refit through the object's device-resident leaf order, against the host leaf order on A
        pos, nrm, idx = meshes[2].arrays()
        V = vertex_buffer(deform(pos, 0.7), nrm)
        A.blas_refit(2, V, idx, blases[2].leaf_order())
        Vd, Id = torch.from_numpy(np.ascontiguousarray(V)).cuda(), torch.from_numpy(np.ascontiguousarray(idx)).cuda()
        torch.cuda.synchronize()
        B.blas_refit(2, Vd, Id, objects[2].leaf_order_device, device=True)
        (na, ta), (nb, tb) = TA.read_all(A, s), TA.read_all(B, s)
        assert tb.tobytes() == ta.tobytes() and nb.tobytes() == na.tobytes()
        assert tb.tobytes() != s.tris.tobytes(), "the refit rewrote the mesh"
    finally:
        A.close()


# ------------------------------------------------------------------ refusals
def _raw_build(engine, view, presorted=None, flags=0):
    h, info = C.c_void_p(), tthip.ObjectBuildInfo()
    st = engine.L.tt_object_build_device(engine.h, C.byref(view) if view is not None else None,
                                         None if presorted is None else presorted.ctypes.data, flags, C.byref(h),
                                         C.byref(info))
    return st, h.value, engine.L.tt_last_error(engine.h).decode()


def _builds_and_traces(engine):
    """The engine still works: a good mesh built on the device, assembled, traced against the oracle."""
    mesh = tthip.Mesh.cornell()
    am = tthip.AssetManager()
    am.add_parent_object(engine.build_object(mesh), None, np.zeros(8, tthip.MAT_DTYPE))
    am.assemble_objects(engine)
    scene = tthip.single_object_scene(mesh)
    W = H = 32
    c2w, ip = tthip.unity_camera((0, 0, 3.4), (0, 0, -1), (0, 1, 0), 40, W, H, 0.3, 1000.0)
    rays = tthip.camera_rays_host(c2w, ip, W, H, 0.3, 1000.0)
    ref = rays.copy()
    engine.trace(rays, W * H, 0, 1000.0, W, H)
    assert O.trace(scene, ref, W * H, 0, 1000.0, W, H)[0] == 0
    assert np.array_equal(rays["hits"], ref["hits"]) and (rays["hits"][:W * H, 1] != 0xFFFFFFFF).any()


def test_an_index_equal_to_n_vertices_is_refused_for_host_and_device_arrays(engine):
    import torch

    mesh = _meshes()["soup_4097"]
    idx = mesh.indices.copy()
    idx[3 * 2222 + 1] = len(mesh.positions)
    bad = tthip.ArrayMesh(mesh.positions, idx, mesh.normals, mesh.tangents, mesh.uvs, mesh.matdat)
    st, h, why = _raw_build(engine, bad.view())
    assert (st, h) == (tthip.TT_ERR_INVALID_ARG, None) and "index" in why
    v = bad.view()
    dev = {k: torch.from_numpy(getattr(bad, k)).cuda() for k in ("positions", "normals", "tangents", "uvs", "indices", "matdat")}
    torch.cuda.synchronize()
    for k, t in dev.items():
        setattr(v, k, t.data_ptr())
    st, h, why = _raw_build(engine, v, flags=tthip.TT_TRACE_DEVICE_PTRS)
    assert (st, h) == (tthip.TT_ERR_INVALID_ARG, None) and "index" in why
    idx[3 * 2222 + 1] = -1
    st, h, _ = _raw_build(engine, tthip.ArrayMesh(mesh.positions, idx).view())
    assert (st, h) == (tthip.TT_ERR_INVALID_ARG, None)
    _builds_and_traces(engine)


def test_malformed_meshes_are_refused(engine):
    mesh = _meshes()["soup_17"]
    v = mesh.view()
    v.n_indices -= 1
    assert _raw_build(engine, v)[:2] == (tthip.TT_ERR_INVALID_ARG, None)
    v = mesh.view()
    v.positions = None
    assert _raw_build(engine, v)[:2] == (tthip.TT_ERR_INVALID_ARG, None)
    assert _raw_build(engine, None)[:2] == (tthip.TT_ERR_INVALID_ARG, None)
    v = mesh.view()
    assert _raw_build(engine, v, flags=tthip.TT_TRACE_DEVICE_PTRS)[:2] == (tthip.TT_ERR_INVALID_ARG, None)  # host memory
    pre = np.zeros((3, 17), np.int32)
    pre[1, 5] = 17
    assert _raw_build(engine, mesh.view(), presorted=pre)[:2] == (tthip.TT_ERR_INVALID_ARG, None)
    _builds_and_traces(engine)


def test_a_nan_position_is_declined_by_the_device_presort(engine):
    pos, _, idx = tthip.Mesh.soup(5, 100, 1.5, 0.35).arrays()
    pos[int(idx[3 * 40])] = np.nan
    st, h, why = _raw_build(engine, tthip.ArrayMesh(pos, idx).view())
    assert (st, h) == (tthip.TT_ERR_UNSUPPORTED, None) and "presort" in why
    st, h, _ = _raw_build(engine, _meshes()["unity_cube"].view())  # n <= 16
    assert (st, h) == (tthip.TT_ERR_UNSUPPORTED, None)
    _builds_and_traces(engine)


def test_leaf_order_exists_on_built_objects_only(engine):
    blas = AC.meshes_and_blases()[1][1]
    obj = engine.create_object(blas)
    n = blas.n_tris
    nodes, tris, leaf = np.zeros(blas.n_nodes, tthip.NODE_DTYPE), np.zeros(n, tthip.TRI_DTYPE), np.zeros(n, np.int32)
    L = engine.L
    assert L.tt_object_read(engine.h, obj.h, nodes.ctypes.data, tris.ctypes.data, None) == tthip.TT_OK
    hn, ht = blas.arrays()
    assert nodes.tobytes() == hn.tobytes() and tris.tobytes() == ht.tobytes()
    assert L.tt_object_read(engine.h, obj.h, None, None, leaf.ctypes.data) == tthip.TT_ERR_INVALID_ARG
    p = C.c_void_p(1)
    assert L.tt_object_leaf_order_device(obj.h, C.byref(p)) == tthip.TT_ERR_INVALID_ARG and not p.value
    assert obj.build_info is None and obj.read(engine)[2] is None
    built = engine.build_object(AC.meshes_and_blases()[0][1])
    assert built.leaf_order_device
    assert L.tt_object_read(engine.h, None, None, None, None) == tthip.TT_ERR_INVALID_ARG
    obj.destroy()
    built.destroy()
