"""Meshes and comparisons for the batched object build (tt_objects_build_device): the mesh set of
tests/test_gpu_object_build.py restated, the tiny soups, the depth-imbalanced chain, and the byte comparison of a
device-built object against the host build (tthip.Blas), which needs neither a GPU reference nor the oracle. The host
builds are made once per process and shared."""
import ctypes as C
import functools
import os

import numpy as np

import tthip

HERE = os.path.dirname(os.path.abspath(__file__))


def grid(nx, nz):  # a flat grid of quads (y = 0): every box is padded by Validate, every SAH sweep full of ties
    xs, zs = np.meshgrid(np.arange(nx + 1, dtype=np.float32), np.arange(nz + 1, dtype=np.float32), indexing="ij")
    pos = np.stack([xs.ravel(), np.zeros(xs.size, np.float32), zs.ravel()], 1)
    idx = []
    for i in range(nx):
        for j in range(nz):
            a, b, c, d = i * (nz + 1) + j, (i + 1) * (nz + 1) + j, i * (nz + 1) + j + 1, (i + 1) * (nz + 1) + j + 1
            idx += [a, b, c, c, b, d]
    return tthip.ArrayMesh(pos, np.array(idx, np.int32))


def with_attributes(mesh, seed):
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
    nrm[0::7] = 0.0
    nrm[1::7] = np.float32([1e-6, 0.0, 0.0])
    nrm[2::7] = np.float32([6e-6, 6e-6, 6e-6])
    nrm[3::7, 2] = -np.abs(nrm[3::7, 2]) - 0.1
    nrm[4::7, 0] = -0.0
    nrm[5::7] = np.float32([-0.0, -0.0, -1.0])
    tan = rng.normal(size=(nv, 4)).astype(np.float32)
    tan[0::5, :3] = 0.0
    tan[1::5, 1] = -0.0
    return dict(positions=pos, indices=idx, normals=nrm, tangents=tan,
                uvs=(rng.random((nv, 2)) * 8 - 4).astype(np.float32), matdat=(np.arange(65) % 8).astype(np.int32))


@functools.lru_cache(maxsize=None)
def mixed():
    """name -> mesh: one triangle to 20,001, in the order the mixed-sizes test passes them."""
    z = np.load(os.path.join(HERE, "golden", "pedestal_mesh.npz"))
    cube = np.load(os.path.join(HERE, "golden", "unity_cube_pins.npz"))
    rng = np.random.default_rng(7)
    dup = rng.random((300, 3), dtype=np.float32) * 4 - 2
    dup_pos = np.concatenate([dup, dup, np.round(dup)])
    signed = rng.integers(-2, 3, (600, 3)).astype(np.float32)
    signed[rng.random(signed.shape) < 0.3] = -0.0
    a65 = _attributes_65()
    m = {
        "single": tthip.ArrayMesh(np.eye(3, dtype=np.float32), np.array([0, 1, 2], np.int32)),
        "unity_cube": tthip.ArrayMesh(cube["cube_v"], cube["cube_i"]),
        "soup_17": tthip.Mesh.soup(21, 17, 1.5, 0.35),
        "pedestal": tthip.ArrayMesh(z["positions"].astype(np.float32), z["indices"]),
        "attributes_65": tthip.ArrayMesh(**a65),
    }
    for drop in ("normals", "tangents", "uvs", "matdat"):
        m["attributes_65_no_" + drop] = tthip.ArrayMesh(**{k: v for k, v in a65.items() if k != drop})
    m.update({
        "signed_zeros": tthip.ArrayMesh(signed, np.arange(600, dtype=np.int32)),
        "duplicates": tthip.ArrayMesh(dup_pos, np.arange(len(dup_pos), dtype=np.int32)),
        "grid_40x25": grid(40, 25),
        "soup_4097": with_attributes(tthip.Mesh.soup(1002, 4097, 1.5, 0.35), 1),
        "soup_20001": with_attributes(tthip.Mesh.soup(31, 20001, 3.0, 0.2), 2),
    })
    return m


TINY_SIZES = list(range(1, 41)) + [64, 65, 255, 256, 257]


@functools.lru_cache(maxsize=None)
def tiny():
    """135 soups of 1..40, 64, 65, 255, 256 and 257 triangles, three seeds each: the root small-sort branches
    (n = 2, 3, 4..16), the root-is-leaf form (n = 1) and the first sizes past them."""
    return [tthip.Mesh.soup(1000 + 7 * n + s, n, 1.5, 0.35) for n in TINY_SIZES for s in range(3)]


@functools.lru_cache(maxsize=None)
def chain(n=600):
    """Triangle i at x = 1.05^i with extents 0.01 x: every SAH split peels a few triangles off the far end, so the
    BVH2 is far deeper than a soup's of the same size."""
    x = (np.float64(1.05) ** np.arange(n)).astype(np.float32)
    e = (x * np.float32(0.01)).astype(np.float32)
    pos = np.zeros((n, 3, 3), np.float32)
    pos[:, :, 0] = x[:, None]
    pos[:, 1, 0] += e
    pos[:, 2, 1] = e
    pos[:, 2, 2] = e
    return tthip.ArrayMesh(pos.reshape(-1, 3), np.arange(3 * n, dtype=np.int32))


def view_arrays(mesh):
    """name -> a copy of every array the mesh's tt_mesh_input names (None where it is null), for a Mesh or an
    ArrayMesh alike."""
    v = mesh.view()
    nv, n = v.n_vertices, v.n_indices // 3
    out = {}
    for name, ct, dt, count in (("positions", C.c_float, np.float32, 3 * nv), ("normals", C.c_float, np.float32, 3 * nv),
                                ("tangents", C.c_float, np.float32, 4 * nv), ("uvs", C.c_float, np.float32, 2 * nv),
                                ("indices", C.c_int32, np.int32, v.n_indices), ("matdat", C.c_int32, np.int32, n)):
        p = getattr(v, name)
        out[name] = np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), (count,)).astype(dt, copy=True) if p else None
    return out


_HOST = {}


def host_build(mesh, lossy_scale=None):
    """tthip.Blas(mesh), built once per mesh object and scale and left unchanged."""
    key = (id(mesh), tuple(lossy_scale) if lossy_scale is not None else None)
    if key not in _HOST:
        _HOST[key] = (mesh, tthip.Blas(mesh) if lossy_scale is None else tthip.Blas(mesh, lossy_scale=lossy_scale))
    return _HOST[key][1]


def bits(a):
    return np.array(list(a), np.float32).view(np.uint32).tolist()


def differences(obj, blas):
    """What differs between a device-built object and a host build: a list of reasons, empty when every byte of the
    nodes, the 88-byte triangles and the leaf order and every field of both info structs agree."""
    nodes, tris, leaf = obj.read()
    hn, ht = blas.arrays()
    out = []
    if nodes.tobytes() != hn.tobytes():
        out.append("CWBVH8 nodes")
    if tris.tobytes() != ht.tobytes():
        out.append("leaf-ordered triangles")
    if leaf is None or not np.array_equal(leaf, blas.leaf_order()):
        out.append("leaf order")
    bi, hi = obj.build_info, blas.info
    if (bi.n_nodes, bi.n_tris, bi.bvh2_depth) != (hi.n_nodes, hi.n_tris, hi.bvh2_depth):
        out.append(f"build info counts {(bi.n_nodes, bi.n_tris, bi.bvh2_depth)} vs {(hi.n_nodes, hi.n_tris, hi.bvh2_depth)}")
    if bits(bi.aabb_min) != bits(hi.aabb_min) or bits(bi.aabb_max) != bits(hi.aabb_max):
        out.append("aabb_untransformed")
    if len(ht) == len(tris) and bi.max_matdat != int(ht["MatDat"].max()):
        out.append("max_matdat")
    i = obj.info
    if (i.n_nodes, i.n_tris, i.root) != (hi.n_nodes, hi.n_tris, 0):
        out.append("object info")
    if i.bytes != hi.n_nodes * 80 + hi.n_tris * (88 + 48):
        out.append("object info bytes")
    return out


def assert_equals_host_build(obj, blas, what=""):
    d = differences(obj, blas)
    assert not d, f"{what}: differs from the host build in {d}"


def destroy(objects):
    for o in objects:
        o.destroy()
