"""The scene, the part layouts and the expected values of tests/test_gpu_refit_many.py: one static soup plus
deforming meshes of 1, 7, 25, 300, 600 and 5,000 triangles (a BLAS of one node, one that just needs a second
level, meshes whose leaf pairs end inside a 256-thread block of the refit launch, one whose leaf pairs span
several blocks), each cut into parts of 1 triangle and of counts that are no multiple of 256. Expected values
come from the oracle's one-mesh refits and numpy alone, never from the library."""
import functools

import numpy as np

import oracle_ctypes as O
import tthip
from test_blas_refit import deform

SIZES = (1, 7, 25, 300, 600, 5000)
# source-triangle cuts per deforming mesh (record r = 1 + its position in SIZES)
CUTS = ([0, 1], [0, 3, 7], [0, 1, 25], [0, 299, 300], [0, 257, 600], [0, 1, 700, 5000])
RECORDS = tuple(range(1, 1 + len(SIZES)))


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case():
    """The scene as uploaded. Every mesh stands under a pure translation by small integers and halves, so the
    world box of a root box on the 1/64 grid is exact."""
    c = Case()
    c.meshes = [tthip.Mesh.soup(1, 120, 3.0, 0.3)] + [
        tthip.Mesh.soup(50 + n, n, 1.0, 0.4) if n < 25 else tthip.Mesh.prop(50 + n, n) for n in SIZES]
    c.blases = [tthip.Blas(m) for m in c.meshes]
    c.l2w = [np.eye(4)] + [tthip.trs_matrix((3.0 * k - 7.0, 0.0, 0.5)) for k in range(len(SIZES))]
    am = tthip.AssetManager()
    for b, m in zip(c.blases, c.l2w):
        am.add_parent(b, m, np.zeros(1, tthip.MAT_DTYPE))
    c.sc = am.build()
    c.arrays = [m.arrays() for m in c.meshes]
    c.leaf = [b.leaf_order() for b in c.blases]
    assert [b.n_tris for b in c.blases[1:]] == list(SIZES)
    assert c.blases[1].info.n_nodes == 1 and c.blases[2].info.n_nodes == 1 and c.blases[3].info.n_nodes > 1
    return c


def with_arrays(sc, nodes, tris):
    return tthip.Scene(nodes, tris, sc.tlas, sc.meshdata, sc.materials, tlas_nodes=sc.tlas_nodes)


def vertices(record, t, exact=False, seed=0):
    """The n_v x 10 float32 vertex buffer of mesh `record` at deformation t (position, normal, four unused floats).
    exact: positions on the 1/64 grid within +-8 and normals of components +-1/4 .. +-1 in quarters, none zero:
    every product and sum of a signed-permutation transform with a translation in quarters is exact (a zero
    position sum ends as +0 either way: the translation, never -0, is added last)."""
    pos, nrm, _ = case().arrays[record]
    p = deform(pos, t)
    if exact:
        rng = np.random.default_rng(1000 * record + seed)
        p = (np.rint(np.clip(p, -7.9, 7.9).astype(np.float64) * 64.0) / 64.0).astype(np.float32)
        nrm = (rng.integers(1, 5, nrm.shape) * rng.choice([-1.0, 1.0], nrm.shape) / 4.0).astype(np.float32)
    v = np.full((len(p), 10), 0.5, np.float32)
    v[:, 0:3], v[:, 3:6] = p, nrm
    return v


def general_matrix(k):
    return tthip.trs_matrix((0.2 + 0.1 * k, -0.1, 0.3 - 0.05 * k), 17.0 + 23.0 * k, 1.0 + 0.125 * (k % 3))


def exact_matrix(k):
    """A signed axis permutation with a translation in quarters: exact on the grid of vertices(exact=True)."""
    rng = np.random.default_rng(77 + k)
    m = np.zeros((4, 4))
    perm, sign = rng.permutation(3), rng.choice([-1.0, 1.0], 3)
    for r in range(3):
        m[r, perm[r]] = sign[r]
    m[:3, 3] = rng.integers(-16, 17, 3) / 4.0
    m[3, 3] = 1.0
    return m


class Layout:
    """One mesh's parts and the concatenated vertex buffer (stride 10) with shifted indices the oracle takes."""

    def __init__(self, record, V, cuts, strides=(10,), transforms=None, reverse=False):
        c = case()
        tri = c.arrays[record][2].reshape(-1, 3)
        self.record, self.cuts, self.leaf = record, cuts, c.leaf[record]
        self.n_tris = len(tri)
        self.transforms = [np.eye(4) if transforms is None else transforms[k] for k in range(len(cuts) - 1)]
        self.parts, self.rows = [], []
        vc, ic, off = [], [], 0
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            uniq, inv = np.unique(tri[a:b], return_inverse=True)
            local = np.ascontiguousarray(inv.reshape(-1), np.int32)
            stride = strides[k % len(strides)]
            self.parts.append(tthip.RefitPart(np.ascontiguousarray(V[uniq][:, :stride]), local, first_tri=a,
                                              transform=self.transforms[k]))
            self.rows.append(slice(off, off + len(uniq)))
            vc.append(V[uniq])
            ic.append(local + off)
            off += len(uniq)
        self.vcat, self.icat = np.ascontiguousarray(np.vstack(vc)), np.concatenate(ic).astype(np.int32)
        if reverse:
            self.parts.reverse()  # parts come in any order

    def item(self, local_to_world=None):
        return tthip.RefitItem(self.record, self.n_tris, self.leaf, self.parts, local_to_world)

    def pretransformed(self):
        """The concatenated buffer with every part's rows taken through its transform in float64 (exact for the
        exact cases), for an identity-transform refit."""
        v = self.vcat.copy()
        for rows, m in zip(self.rows, self.transforms):
            v[rows, 0:3] = (self.vcat[rows, 0:3].astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32)
            v[rows, 3:6] = (self.vcat[rows, 3:6].astype(np.float64) @ m[:3, :3].T).astype(np.float32)
        return v

    def corners64(self):
        """(n_tris, 3, 3) float64: every source triangle's (i0, i2, i1) corners under its part's transform."""
        v = self.vcat[:, 0:3].astype(np.float64)
        for rows, m in zip(self.rows, self.transforms):
            v[rows] = self.vcat[rows, 0:3].astype(np.float64) @ m[:3, :3].T + m[:3, 3]
        i = self.icat.reshape(-1, 3)
        return np.stack([v[i[:, 0]], v[i[:, 2]], v[i[:, 1]]], 1)


def oracle_chain(sc, refits):
    """The oracle's one-mesh refits made one after the other: refits = [(record, vertices, indices, leaf, transform)]."""
    nodes, tris = sc.nodes, sc.tris
    for record, v, idx, leaf, xf in refits:
        st, nodes, tris = O.blas_refit(with_arrays(sc, nodes, tris), record, v, idx, leaf, xf)
        assert st == 0
    return nodes, tris


def padded_root_box(corners32):
    """{BBMax, BBMin} over the triangles' boxes as Construct pads them (float32): (n, 3, 3) corners -> (6,)."""
    c = np.asarray(corners32, np.float32)
    mx, mn = c.max(1), c.min(1)
    flat = (mx - mn) < np.float32(0.000001)
    mx, mn = np.where(flat, mx + np.float32(0.000001), mx), np.where(flat, mn - np.float32(0.000001), mn)
    return np.concatenate([mx.max(0), mn.min(0)]).astype(np.float32)


def box_corners(box):
    b = np.asarray(box, np.float64)
    return np.array([[b[0 if c & 1 else 3], b[1 if c & 2 else 4], b[2 if c & 4 else 5]] for c in range(8)])


def world_box64(box, m):
    """{BBMax, BBMin} in float64 of the eight corners of a root box under the row-major matrix m."""
    w = box_corners(box) @ np.asarray(m, np.float64)[:3, :3].T + np.asarray(m, np.float64)[:3, 3]
    return np.concatenate([w.max(0), w.min(0)])


def world_box_bound(box, m):
    """Per output coordinate, 4 * 2^-24 * max over corners of (|m0 x| + |m1 y| + |m2 z| + |m3|): the rounding bound
    of the pinned three-fmaf chain and the add, in the layout of world_box64."""
    a = np.abs(box_corners(box))[:, None, :] * np.abs(np.asarray(m, np.float64)[:3, :3])[None]  # (8, 3 rows, 3 terms)
    mag = (a.sum(2) + np.abs(np.asarray(m, np.float64)[:3, 3])[None]).max(0)
    return np.concatenate([mag, mag]) * 4.0 * 2.0 ** -24
