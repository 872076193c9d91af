"""Inputs shared by tests/test_enclosure_host.py and tests/test_gpu_enclosure.py: the scenes whose TLAS is refit over
hand-made instance boxes at the quantiser's edges, the edge boxes themselves, and the small meshes of the build tests.
Test infrastructure, no test lives here. Every coordinate stays above -10000 except in far_box_case (the refit's
empty-slot sentinel)."""
import functools

import numpy as np

import tthip

EDGE_SIZES = (9, 70)  # instances: a root with leaves only is not enough, 70 gives a second and third TLAS level
SEED_40 = 71          # tlas_rebuild_cases.base_scene(SEED_40, 40): the 40-instance scene


@functools.lru_cache(maxsize=None)
def edge_scene(n):
    """n instances of a one-triangle BLAS on a loose spiral: a real, uploadable scene whose TLAS topology the refits
    keep while the boxes below it are replaced by edge_boxes. Shared: do not write to it."""
    am = tthip.AssetManager()
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    ip = am.add_instance_parent(tthip.Blas(tthip.Mesh.from_arrays(pos, np.array([0, 1, 2], np.int32))))
    for i in range(n):
        a = 0.7 * i
        am.add_instance(ip, tthip.trs_matrix((0.6 * i * np.cos(a), 0.3 * (i % 5), 0.6 * i * np.sin(a)), 10.0 * i, 1.0 + 0.1 * (i % 4)))
    return am.build()


def _f32(x):
    return np.float32(x)


def _ulps(x, d):
    x = _f32(x)
    for _ in range(abs(d)):
        x = np.nextafter(x, _f32(np.inf if d > 0 else -np.inf), dtype=np.float32)
    return x


def _fill(n, origin, extent, seed, span_box=False):
    """n float32 boxes {BBMax, BBMin} inside [origin, origin + extent] per axis (origin + extent must be a float32):
    box 0 touches the minimum corner, box 1 the maximum corner, so the union is exactly that range; span_box: box 2
    alone spans it."""
    rng = np.random.default_rng(seed)
    o = np.asarray(origin, np.float32)
    top = (o.astype(np.float64) + np.asarray(extent, np.float32).astype(np.float64)).astype(np.float32)
    assert np.array_equal(top.astype(np.float64), o.astype(np.float64) + np.asarray(extent, np.float32).astype(np.float64))
    assert np.array_equal((top - o).astype(np.float32), np.asarray(extent, np.float32)), "fl(max - min) is the extent"
    o64, t64 = o.astype(np.float64), top.astype(np.float64)
    lo = o64 + (t64 - o64) * rng.random((n, 3)) * 0.9
    hi = lo + (t64 - lo) * rng.random((n, 3)) * 0.5
    lo, hi = np.clip(lo.astype(np.float32), o, top), np.clip(hi.astype(np.float32), o, top)
    hi = np.maximum(hi, lo)
    lo[0], hi[1] = o, top
    if span_box:
        lo[2], hi[2] = o, top
    return np.ascontiguousarray(np.concatenate([hi, lo], 1), np.float32)


def edge_boxes(n):
    """[(name, (n, 6) float32 boxes)]: the quantiser's edges as the union extent of the root (and, by chance and by
    the flat and tiny cases, of deeper nodes). quantum = pow2_ceil(fl(extent * fl(1/255))), so extent = 255 * 2^k is
    where ceil(extent / quantum) would first reach 256."""
    out = []
    ks = (-10, 0, 7)
    for d in (-2, -1, 0, 1, 2):
        for rot in range(3):
            k3 = [ks[(rot + a) % 3] for a in range(3)]  # every (k, d) on every axis over the three rotations
            ext = np.array([_ulps(255.0 * 2.0 ** k, d) for k in k3], np.float32)
            org = np.array([-64.0 * 2.0 ** k for k in k3], np.float32)  # negative origins, max = 191 * 2^k +- ulps exact
            out.append((f"extent 255*2^{k3} {d:+d} ulp", _fill(n, org, ext, 100 + 10 * d + rot)))
    k3 = [0, 7, -10]
    ext = np.array([255.0 * 2.0 ** k for k in k3], np.float32)
    out.append(("one box spans the root", _fill(n, np.zeros(3, np.float32), ext, 7, span_box=True)))
    flat = _fill(n, np.float32([-3.0, 0.0, 1.0]), np.float32([8.0, 4.0, 2.0]), 8)
    flat[:, 1] = flat[:, 4] = np.float32(2.5)  # every box flat at the same y: a zero extent on every level
    out.append(("zero extent in y", flat))
    out.append(("extent 1e-30", _fill(n, np.zeros(3, np.float32), np.full(3, 1e-30, np.float32), 9)))
    out.append(("extent 1e6", _fill(n, np.full(3, -5000.0, np.float32), np.full(3, 1e6, np.float32), 10)))
    p = _f32(4096.37)
    out.append(("|P| >> extent", _fill(n, np.full(3, p, np.float32), np.full(3, _ulps(p, 2) - p, np.float32), 11)))
    out.append(("negative origins", _fill(n, np.float32([-9000.0, -0.375, -0.0009765625]),
                                             np.float32([16.0, 0.75, 0.001953125]), 12)))
    return out


def far_box_case(n):
    """Boxes of edge_scene(n)'s own layout with record 3 moved to x ~ -20000: NodeUpdate takes a child whose
    BBMax.x < -10000 for an empty slot (BVHRefitter.compute:287-290) and collapses it to the parent's minimum."""
    boxes = np.ascontiguousarray(edge_scene(n).meta["mesh_aabbs"], np.float32).copy()
    boxes[3, 0] -= np.float32(20000.0)
    boxes[3, 3] -= np.float32(20000.0)
    return boxes


# ------------------------------------------------------------------ meshes of the build tests
BUILD_TRIS = (1, 7, 25, 300, 5000)


def coplanar_mesh():
    """An 8 x 6 grid of quads in the plane y = 0.75: every triangle box is flat in y, the AABB.Validate padding path."""
    nx, nz = 8, 6
    xs, zs = np.meshgrid(np.arange(nx + 1, dtype=np.float32), np.arange(nz + 1, dtype=np.float32), indexing="ij")
    pos = np.stack([xs.ravel(), np.full(xs.size, 0.75, np.float32), zs.ravel()], 1)
    idx = []
    for i in range(nx):
        for j in range(nz):
            a, b, c, d = i * (nz + 1) + j, (i + 1) * (nz + 1) + j, i * (nz + 1) + j + 1, (i + 1) * (nz + 1) + j + 1
            idx += [a, b, c, c, b, d]
    return tthip.ArrayMesh(pos, np.array(idx, np.int32))


@functools.lru_cache(maxsize=None)
def build_meshes():
    """{name: mesh}: 1, 7, 25, 300 and 5,000 triangles (one node, a just-needed second level, several levels, several
    blocks of the build kernels) and the coplanar grid."""
    m = {f"soup_{n}": tthip.Mesh.soup(300 + n, n, 1.5, 0.35) if n < 300 else tthip.Mesh.prop(300 + n, n) for n in BUILD_TRIS}
    m["coplanar"] = coplanar_mesh()
    return m
