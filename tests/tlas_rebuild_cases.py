"""Shared by tests/test_tlas_build_host.py and tests/test_gpu_tlas_rebuild.py: poses of test_gpu_parity's
refit_scene (one static parent, instances of six props), and a scene with a rebuilt TLAS put in place on the host."""
import dataclasses
import functools

import numpy as np

import tthip
from test_gpu_parity import refit_scene

W, H = 192, 108


@functools.lru_cache(maxsize=None)
def base_scene(seed, n_inst):
    """Shared between tests: do not write to it."""
    return refit_scene(seed, n_inst=n_inst)


def moved_pose(a, seed, scale=6.0, ties=True):
    """_MeshData and world boxes of scene `a` with every instance displaced by N(0, scale) per axis. ties: tie_boxes."""
    rng = np.random.default_rng(seed)
    md = a.meshdata.copy()
    boxes = np.ascontiguousarray(a.meta["mesh_aabbs"], np.float32).copy()
    for i in range(1, len(md)):
        d = rng.normal(0, scale, 3) * [1, 0.2, 1]
        w2l = md["W2L"][i].astype(np.float64).reshape(4, 4).T
        shift = np.eye(4)
        shift[:3, 3] = -d
        md["W2L"][i] = tthip.unity_colmajor(w2l @ shift)
        boxes[i, 0:3] += d.astype(np.float32)
        boxes[i, 3:6] += d.astype(np.float32)
    return md, tie_boxes(boxes) if ties else boxes


def tie_boxes(boxes):
    """Records 4, 10, 16, ... and the record three behind each both get the union of their two boxes: disjoint pairs
    of identical boxes (each still holds its mesh), which only the presort's tie order tells apart."""
    out = boxes.copy()
    for i in range(4, len(out), 6):
        out[i, :3] = out[i - 3, :3] = np.maximum(boxes[i, :3], boxes[i - 3, :3])
        out[i, 3:] = out[i - 3, 3:] = np.minimum(boxes[i, 3:], boxes[i - 3, 3:])
    return out


def instance_positions(seed, n_inst):
    """The positions refit_scene(seed, n_inst=n_inst) draws, by replaying its generator."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n_inst, 3))
    for i in range(n_inst):
        out[i] = rng.uniform(-40, 40, 3) * [1, 0.2, 1]
        rng.uniform(0, 360)
        rng.uniform(0.5, 2)
    return out


def permuted_pose(seed, n_inst, perm_seed):
    """The scene whose instances swapped places among themselves: instance i (its prop, rotation and scale kept)
    stands where instance perm[i] stood. Returns (meshdata, boxes) of that pose; the BLASes and the order of the
    records are those of base_scene(seed, n_inst)."""
    pos = instance_positions(seed, n_inst)
    perm = np.random.default_rng(perm_seed).permutation(n_inst)
    b = refit_scene(seed, offsets=pos[perm] - pos, n_inst=n_inst)
    a = base_scene(seed, n_inst)
    assert np.array_equal(a.meshdata["NodeOffset"], b.meshdata["NodeOffset"]) and np.array_equal(a.tris, b.tris)
    return b.meshdata, np.ascontiguousarray(b.meta["mesh_aabbs"], np.float32)


def with_tlas(a, nodes, tlas, meshdata):
    """Scene `a` with the TLAS (nodes, TLASBVH8Indices) in place of its own, as an installation leaves the arrays:
    the new nodes, zeros up to the old count, everything else untouched."""
    out = a.nodes.copy()
    out[:max(a.tlas_nodes, len(nodes))] = np.zeros(1, tthip.NODE_DTYPE)[0]
    out[:len(nodes)] = nodes
    return dataclasses.replace(a, nodes=out, tlas=np.ascontiguousarray(tlas, np.int32), meshdata=meshdata,
                               tlas_nodes=len(nodes))


def capacity(a):
    """The TLAS region of the reference's layout: 2 * n_mesh nodes in front of the first BLAS."""
    return 2 * len(a.meshdata)
