"""Seeded light scenes and ray sets for the light-BVH tests (host and GPU), built with the library's own host builders.

Scenes (whole scenes: TLAS, BLAS, _MeshData; emissive triangles carry the mesh-local material EMISSIVE):
  L1 "room"    a closed room with two emissive ceiling quads (4 light triangles; one quad has a blocker slab
               under it), a hanging cluster with 37 light triangles (odd, no power of two), and two instances of one
               6-light-triangle prop -- one rotated with scale 0.5 / 2 / 3, one mirrored -- sharing one light tree:
               4 light meshes;
  L2 "single"  a floor and one emissive triangle: both trees are one leaf;
  L3 "deep"    a floor under a jittered 32 x 16 grid of quads, 1,024 light triangles (depth >= 10).
Ray sets are real records: Generate + trace at bounce 0 over 64 x 64 pixels, the enqueue's bounce-1 rays traced, by
the CPU oracle here (the GPU tests produce the same records on the device and compare them first).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import oracle_ctypes as O
import tthip

EMISSIVE = 1
W = H = 64
FAR, NEAR = 1000.0, 0.3
FRAMES, MAX_BOUNCE = 3, 3


def _quad(p, ex, ey):
    p, ex, ey = (np.asarray(a, np.float64) for a in (p, ex, ey))
    return [p, p + ex, p + ex + ey, p, p + ex + ey, p + ey]


class _Soup:
    def __init__(self):
        self.v, self.m = [], []

    def quad(self, p, ex, ey, mat=0):
        self.v += _quad(p, ex, ey)
        self.m += [mat, mat]

    def tri(self, a, b, c, mat=0):
        self.v += [np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)]
        self.m.append(mat)

    def mesh(self):
        """Unshared vertices with their face's normal (a, b, c counter-clockwise seen from the normal's side)."""
        pos = np.asarray(self.v, np.float32)
        t = pos.astype(np.float64).reshape(-1, 3, 3)
        fn = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        fn /= np.linalg.norm(fn, axis=1, keepdims=True)
        return tthip.ArrayMesh(pos, np.arange(len(pos), dtype=np.int32), normals=np.repeat(fn, 3, 0).astype(np.float32),
                               matdat=np.asarray(self.m, np.int32))


def _room_mesh():
    s = _Soup()
    s.quad((-5, 0, -5), (0, 0, 10), (10, 0, 0))     # floor (normal +y)
    s.quad((-5, 6, -5), (10, 0, 0), (0, 0, 10))     # ceiling
    s.quad((-5, 0, -5), (10, 0, 0), (0, 6, 0))      # back
    s.quad((-5, 0, 5), (0, 6, 0), (10, 0, 0))       # front
    s.quad((-5, 0, -5), (0, 6, 0), (0, 0, 10))      # left
    s.quad((5, 0, -5), (0, 0, 10), (0, 6, 0))       # right
    s.quad((-3.5, 5.9, -3.0), (2.0, 0, 0), (0, 0, 1.5), EMISSIVE)   # panel A: open
    s.quad((1.5, 5.9, 1.0), (2.0, 0, 0), (0, 0, 1.5), EMISSIVE)     # panel B: a slab hangs under it
    s.quad((1.0, 5.5, 0.5), (3.0, 0, 0), (0, 0, 2.5))               # the slab, top ...
    s.quad((1.0, 5.45, 0.5), (0, 0, 2.5), (3.0, 0, 0))              # ... and bottom
    return s.mesh()


def _cluster_mesh(rng):
    s = _Soup()
    for k in range(60):
        c = rng.uniform((-1.0, -0.6, -1.0), (1.0, 0.6, 1.0))
        a, b = rng.normal(0, 0.18, 3), rng.normal(0, 0.18, 3)
        s.tri(c, c + a, c + b, EMISSIVE if k < 37 else 0)
    return s.mesh()


def _prop_mesh():
    s = _Soup()
    faces = [((-.5, -.5, -.5), (1, 0, 0), (0, 1, 0)), ((-.5, -.5, .5), (0, 1, 0), (1, 0, 0)),
             ((-.5, -.5, -.5), (0, 0, 1), (1, 0, 0)), ((-.5, .5, -.5), (1, 0, 0), (0, 0, 1)),
             ((-.5, -.5, -.5), (0, 1, 0), (0, 0, 1)), ((.5, -.5, -.5), (0, 0, 1), (0, 1, 0))]
    for k, (p, ex, ey) in enumerate(faces):
        s.quad(p, ex, ey, EMISSIVE if k < 3 else 0)  # three emissive faces: 6 light triangles
    return s.mesh()


def _trs(t, rot_deg=(0, 0, 0), scale=(1, 1, 1)):
    rx, ry, rz = np.deg2rad(rot_deg)
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = (Ry @ Rx @ Rz) @ np.diag(scale)
    m[:3, 3] = t
    return m


@dataclass
class Case:
    name: str
    scene: tthip.Scene
    lights: tthip.Lights
    parents: list            # [(LightTriData, normals)] as given to the assembly
    instances: list          # [(parent, mesh_index, local_to_world)]
    view: tuple              # (position, forward, vfov)


def _mesh_tri_range(scene, m):
    off = int(scene.meshdata["TriOffset"][m])
    later = [int(o) for o in scene.meshdata["TriOffset"] if o > off]
    return off, (min(later) if later else len(scene.tris))


def _assemble(name, am, l2w_of_mesh, view):
    """Lights of every mesh record with emissive triangles; records sharing a TriOffset share a parent."""
    scene = am.build()
    parents, parent_of_off, instances = [], {}, []
    for m in range(len(scene.meshdata)):
        off, end = _mesh_tri_range(scene, m)
        targets = np.nonzero(scene.tris["MatDat"][off:end] == EMISSIVE)[0].astype(np.uint32)
        if len(targets) == 0:
            continue
        if off not in parent_of_off:
            parent_of_off[off] = len(parents)
            parents.append(tthip.light_tris_from_mesh(scene.tris[off:end], targets))
        instances.append((parent_of_off[off], m, l2w_of_mesh[m]))
    lights = tthip.lights_assemble(parents, instances, scene.meshdata)
    return Case(name, scene, lights, parents, instances, view)


@lru_cache(maxsize=None)
def l1_room() -> Case:
    rng = np.random.default_rng(0x4C31)
    am = tthip.AssetManager()
    mats = np.zeros(2, tthip.MAT_DTYPE)
    cluster = _trs((-1.0, 3.2, 1.5), (0, 25, 0))
    am.add_parent(tthip.Blas(_room_mesh()), None, mats)
    am.add_parent(tthip.Blas(_cluster_mesh(rng)), cluster, mats)
    ip = am.add_instance_parent(tthip.Blas(_prop_mesh()), mats)
    skew = _trs((2.5, 1.5, -2.5), (20, 35, 10), (0.5, 2.0, 3.0))
    mirror = _trs((-3.0, 1.0, -1.0), (0, -30, 0), (-1.0, 1.0, 1.0))
    am.add_instance(ip, skew)
    am.add_instance(ip, mirror)
    return _assemble("L1", am, [np.eye(4), cluster, skew, mirror], ((0.0, 2.5, 4.6), (0.0, 0.05, -1.0), 75.0))


@lru_cache(maxsize=None)
def l2_single() -> Case:
    s = _Soup()
    s.quad((-4, 0, -4), (0, 0, 8), (8, 0, 0))
    s.tri((-1, 3, -1), (1, 3, -1), (0, 3, 1.2), EMISSIVE)  # faces down
    am = tthip.AssetManager()
    am.add_parent(tthip.Blas(s.mesh()), None, np.zeros(2, tthip.MAT_DTYPE))
    return _assemble("L2", am, [np.eye(4)], ((0.0, 1.5, 5.0), (0.0, -0.2, -1.0), 60.0))


@lru_cache(maxsize=None)
def l3_deep() -> Case:
    rng = np.random.default_rng(0x4C33)
    s = _Soup()
    s.quad((-8, 0, -4), (0, 0, 8), (16, 0, 0))
    gx, gz = np.meshgrid(np.arange(33), np.arange(17), indexing="ij")
    vx = -8 + 0.5 * gx + rng.uniform(-0.1, 0.1, gx.shape)
    vz = -4 + 0.5 * gz + rng.uniform(-0.1, 0.1, gz.shape)
    vy = 4 + rng.uniform(-0.15, 0.15, gx.shape)
    P = lambda i, j: (vx[i, j], vy[i, j], vz[i, j])
    for i in range(32):
        for j in range(16):
            s.tri(P(i, j), P(i + 1, j), P(i + 1, j + 1), EMISSIVE)  # normal -y
            s.tri(P(i, j), P(i + 1, j + 1), P(i, j + 1), EMISSIVE)
    am = tthip.AssetManager()
    am.add_parent(tthip.Blas(s.mesh()), None, np.zeros(2, tthip.MAT_DTYPE))
    return _assemble("L3", am, [np.eye(4)], ((0.0, 1.5, 6.0), (0.0, -0.1, -1.0), 70.0))


CASES = {"L1": l1_room, "L2": l2_single, "L3": l3_deep}


def camera(case: Case):
    pos, fwd, vfov = case.view
    return tthip.unity_camera(pos, fwd, (0, 1, 0), vfov, W, H, NEAR, FAR)


@lru_cache(maxsize=None)
def ray_sets(name: str):
    """{"b0": (rays, n, bounce), "b1": ..., "ragged": ...}: 2 W H RayData each, traced by the oracle. "ragged" has
    8,229 = 2 x 4,096 + 37 records on a 128 x 128 screen (bounce 0 twice with new pixel indices, then 37 misses)."""
    case = CASES[name]()
    c2w, ip = camera(case)
    rays = O.generate(c2w, ip, W, H, NEAR, FAR, jitter=1, frames=FRAMES, max_bounce=MAX_BOUNCE)
    assert O.trace(case.scene, rays, W * H, 0, FAR, W, H)[0] == 0
    b0 = rays.copy()
    n1 = O.enqueue_bounce(case.scene, rays, W * H, 0, FAR, W, H, frames=FRAMES, max_bounce=MAX_BOUNCE)
    assert O.trace(case.scene, rays, n1, 1, FAR, W, H)[0] == 0
    b1 = rays.copy()
    big = np.zeros(2 * 128 * 128, tthip.RAY_DTYPE)
    big[: W * H] = b0[: W * H]
    big[W * H: 2 * W * H] = b0[: W * H]
    big["PixelIndex"][W * H: 2 * W * H] += W * H
    big[2 * W * H: 2 * W * H + 37] = b0[:37]
    big["hits"][2 * W * H: 2 * W * H + 37] = (0, 0xFFFFFFFF, np.float32(FAR).view(np.uint32), 0)
    return {"b0": (b0, W * H, 0, W, H), "b1": (b1, n1, 1, W, H), "ragged": (big, 2 * W * H + 37, 0, 128, 128)}
