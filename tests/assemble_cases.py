"""Inputs shared by tests/test_assemble_host.py, tests/test_gpu_assemble.py and the form child: scene S of the
on-device assembly (3 parents, 2 instance parents, 3 instances) and the broken BLASes tt_object_validate must
refuse. Test infrastructure, no test lives here."""
import functools

import numpy as np

import tthip

# triangles per BLAS: the counts straddle a wave (63 / 65), the reference's 372-thread group (373) and the gather's
# 1,024-unit tile (4,097); odd prefix sums put 88-byte records at offsets that are 8- but not 16-byte aligned
PARENT_TRIS = (1, 65, 4097)
INSTANCE_PARENT_TRIS = (63, 373)
INSTANCES = ((0, (4.0, 0.5, -2.0)), (1, (-4.0, 0.0, 1.0)), (0, (0.5, 3.0, 2.5)))  # (instance parent, translation)
PARENT_POS = ((0.0, 0.0, 0.0), (2.5, 0.0, 0.0), (-1.0, -0.5, -1.0))


def _mesh(k: int, n_tris: int) -> "tthip.Mesh":
    return tthip.Mesh.soup(1000 + k, n_tris, 1.5, 0.35)


@functools.lru_cache(maxsize=None)
def meshes_and_blases():
    """(meshes, blases) in layout order: parents, then instance parents. Built once per process."""
    ms = [_mesh(k, n) for k, n in enumerate(PARENT_TRIS + INSTANCE_PARENT_TRIS)]
    return ms, [tthip.Blas(m) for m in ms]


def manager(parent_blases, instance_parent_blases) -> "tthip.AssetManager":
    am = tthip.AssetManager()
    for k, b in enumerate(parent_blases):
        am.add_parent(b, tthip.trs_matrix(PARENT_POS[k % len(PARENT_POS)], 20.0 * k), np.zeros(2, tthip.MAT_DTYPE))
    for b in instance_parent_blases:
        am.add_instance_parent(b, np.zeros(1, tthip.MAT_DTYPE))
    for ip, pos in INSTANCES:
        am.add_instance(ip, tthip.trs_matrix(pos, 35.0 * (ip + 1), 1.25))
    return am


@functools.lru_cache(maxsize=None)
def scene_s():
    """(AssetManager, its host build(): what tt_scene_upload takes)."""
    _, bl = meshes_and_blases()
    am = manager(bl[:len(PARENT_TRIS)], bl[len(PARENT_TRIS):])
    return am, am.build()


# ------------------------------------------------------------------ broken BLASes
def meta_of(nodes, ni: int, k: int) -> int:
    return int(nodes["meta"][ni][k >> 2] >> ((k & 3) * 8)) & 0xFF


def set_meta(nodes, ni: int, k: int, value: int):
    w = int(nodes["meta"][ni][k >> 2])
    sh = (k & 3) * 8
    nodes["meta"][ni][k >> 2] = (w & ~(0xFF << sh) & 0xFFFFFFFF) | ((value & 0xFF) << sh)


def children(nodes, ni: int):
    """[(k, 'inner', relative child index) | (k, 'leaf', first triangle, last triangle)] of node ni."""
    out = []
    imask = int(nodes["e_imask"][ni]) >> 24
    for k in range(8):
        m = meta_of(nodes, ni, k)
        low5, bits = m & 0x1F, (m >> 5) & 7
        if (m & 0x18) == 0x18:
            out.append((k, "inner", bin(imask & ((1 << (low5 - 24)) - 1)).count("1")))
        elif bits:
            base = int(nodes["base_tri"][ni]) + low5
            out.append((k, "leaf", base + (bits & -bits).bit_length() - 1, base + bits.bit_length() - 1))
    return out


def bad_objects(nodes, tris):
    """{name: (nodes, tris, root)}: one violation each of a BLAS with inner nodes, everything else left valid."""
    n_nodes, n_tris = len(nodes), len(tris)
    inner = [(ni, c) for ni in range(n_nodes) for c in children(nodes, ni) if c[1] == "inner"]
    leaf = [(ni, c) for ni in range(n_nodes) for c in children(nodes, ni) if c[1] == "leaf"]
    assert inner and leaf, "the BLAS needs inner and leaf children"
    out = {}
    # the last child of node 0 lands exactly on n_nodes (its siblings stay below)
    a = nodes.copy()
    rel = max(c[2] for ni, c in inner if ni == 0)
    a["base_child"][0] = n_nodes - rel
    out["child index == n_nodes"] = (a, tris, 0)
    # the node holding the last triangle, shifted by one
    a = nodes.copy()
    ni, c = max(leaf, key=lambda x: x[1][3])
    assert c[3] == n_tris - 1
    a["base_tri"][ni] += 1
    out["triangle index == n_tris"] = (a, tris, 0)
    a = nodes.copy()
    ni, c = inner[0]
    set_meta(a, ni, c[0], (meta_of(a, ni, c[0]) & 0x1F) | (2 << 5))
    out["inner meta with child bits 2"] = (a, tris, 0)
    a = nodes.copy()
    ni, c = leaf[0]
    set_meta(a, ni, c[0], (2 << 5) | 23)  # triangle slot 23 + 1 = bit 24
    out["leaf meta reaching bit 24"] = (a, tris, 0)
    out["root >= n_nodes"] = (nodes, tris, n_nodes)
    return out
