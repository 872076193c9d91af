"""Seeded poses for the light-BVH refit tests, over the scenes of tests/lights_cases.py (imported, not edited).

Per case three sets of light-mesh transforms (one LightBVHTransform per light mesh, SolidOffset = the LightNodeOffset of
its _MeshData record):
  "translated"  every instance's localToWorld under a seeded translation;
  "rotated"     under a seeded rotation about its own origin and a translation;
  "scaled"      with a seeded non-uniform scale (0.4 .. 2.5 per axis) applied in the mesh's space.
"across" (L1) moves the skewed prop to the far side of the room, for the chain into tt_emit_nee.
For L1's 37-triangle cluster and L3's 1,024-triangle grid a deformed vertex set: the mesh's own triangles as the
scene holds them (leaf order), unshared, displaced by a smooth seeded field -- applied with the oracle's blas_refit on
the host and tt_blas_refit on the device."""
from functools import lru_cache

import numpy as np

import lights_cases as LC
import oracle_ctypes as O
import tthip

POSES = ("translated", "rotated", "scaled")
DEFORMED = {"L1": 1, "L3": 0}  # the deforming _MeshData record
SEED = {"L1": 0x5231, "L2": 0x5232, "L3": 0x5233}


def instance_matrices(case):
    """The rest localToWorld of every light mesh, in _LightMeshes order (the assembly's instances)."""
    return [np.asarray(m, np.float64) for _, _, m in case.instances]


def solid_offsets(case):
    return [int(case.scene.meshdata["LightNodeOffset"][int(r)]) for r in case.lights.meshes["LockedMeshIndex"]]


def tree_records(case):
    """One _MeshData record per distinct light tree (the first that names it), in _LightMeshes order."""
    seen, out = set(), []
    for r in case.lights.meshes["LockedMeshIndex"]:
        off = int(case.scene.meshdata["LightNodeOffset"][int(r)])
        if off not in seen:
            seen.add(off)
            out.append(int(r))
    return out


@lru_cache(maxsize=None)
def pose_matrices(name: str, pose: str):
    case = LC.CASES[name]()
    rng = np.random.default_rng(SEED[name] + {"translated": 1, "rotated": 2, "scaled": 3, "across": 4}[pose])
    out = []
    for i, m in enumerate(instance_matrices(case)):
        if pose == "translated":
            d = LC._trs(rng.uniform(-1.5, 1.5, 3))
            out.append(d @ m)
        elif pose == "rotated":
            d = LC._trs(rng.uniform(-0.5, 0.5, 3), rng.uniform(-170, 170, 3))
            pivot = LC._trs(m[:3, 3])
            out.append(pivot @ d @ np.linalg.inv(pivot) @ m)
        elif pose == "scaled":
            s = np.eye(4)
            s[:3, :3] = np.diag(rng.uniform(0.4, 2.5, 3))
            out.append(m @ s)
        else:  # "across": the skewed prop (L1's third light mesh) to the other side of the room
            out.append(LC._trs((-5.0, 0.5, 5.5)) @ m if i == 2 else m)
    return out


def transforms(name: str, pose: str) -> np.ndarray:
    return tthip.light_transforms(pose_matrices(name, pose), solid_offsets(LC.CASES[name]()))


def with_tris(scene, tris, meshdata=None):
    import dataclasses

    return dataclasses.replace(scene, tris=tris, meshdata=scene.meshdata if meshdata is None else meshdata)


@lru_cache(maxsize=None)
def deformed(name: str):
    """(record, vertices [3 n, 6], indices [3 n], leaf_of_triangle [n], the scene after the oracle's refit)."""
    case = LC.CASES[name]()
    rec = DEFORMED[name]
    off, end = LC._mesh_tri_range(case.scene, rec)
    T = case.scene.tris[off:end]
    n = len(T)
    p0 = T["pos0"].astype(np.float64)
    # Construct reads vidx = (i0, i2, i1): posedge1 = v[i2] - v[i0], posedge2 = v[i1] - v[i0]
    v = np.stack([p0, p0 + T["posedge2"].astype(np.float64), p0 + T["posedge1"].astype(np.float64)], 1).reshape(-1, 3)
    rng = np.random.default_rng(SEED[name] + 9)
    k, ph = rng.uniform(0.8, 2.0, (3, 3)), rng.uniform(0, 6.28, 3)
    amp = 0.25 if name == "L1" else 0.2
    moved = v + amp * np.sin(v @ k.T + ph)
    V = np.zeros((3 * n, 6), np.float32)
    V[:, 0:3] = moved
    V[:, 4] = 1.0
    idx = np.arange(3 * n, dtype=np.int32)
    leaf = np.arange(n, dtype=np.int32)
    st, _, tris = O.blas_refit(case.scene, rec, V, idx, leaf)
    assert st == 0
    return rec, V, idx, leaf, with_tris(case.scene, tris)


PARTS = ("mesh", "tlas", "both")


def scenario(name: str, pose: str, part: str, deform: bool = False):
    """(the scene whose triangles the refit reads, the listed records, the transforms or None) of one refit call."""
    case = LC.CASES[name]()
    scene = deformed(name)[4] if deform else case.scene
    records = tree_records(case) if part in ("mesh", "both") else []
    return scene, records, (transforms(name, pose) if part in ("tlas", "both") else None)


@lru_cache(maxsize=None)
def host_refit(name: str, pose: str, part: str, deform: bool = False, conservative: bool = False):
    """tt_lights_refit_host over the case's uploaded lights: the refitted Lights (shared: do not write to it)."""
    case = LC.CASES[name]()
    scene, records, x = scenario(name, pose, part, deform)
    return tthip.lights_refit_host(case.lights, scene, records, x,
                                   tthip.TT_LIGHT_REFIT_CONSERVATIVE if conservative else 0)


@lru_cache(maxsize=None)
def varied_lights(name: str):
    """The case's lights with a seeded cosTheta_e code (8,000 .. 30,000) on every mesh-tree leaf: as built, all leaves
    share one code, and a union's min over equal codes says nothing. A refit keeps a leaf's cosTheta_oe."""
    case = LC.CASES[name]()
    rng = np.random.default_rng(SEED[name] + 17)
    nodes = case.lights.nodes.copy()
    leaf = (nodes["left"] < 0) & (np.arange(len(nodes)) >= 2 * len(case.lights.meshes))
    codes = rng.integers(8000, 30000, int(leaf.sum())).astype(np.uint32)
    nodes["cosTheta_oe"][leaf] = (nodes["cosTheta_oe"][leaf] & np.uint32(0xFFFF)) | (codes << np.uint32(16))
    return tthip.Lights(nodes, case.lights.tris.copy(), case.lights.meshes)


def overlapping_lights(name: str = "L1"):
    """Lights that tt_lights_validate accepts (it looks at each light mesh alone) and no refit can climb: a leaf of the
    largest mesh tree made an interior node whose children are two sibling leaves of the last tree."""
    case = LC.CASES[name]()
    md, nodes = case.scene.meshdata, case.lights.nodes.copy()
    offs = sorted(set(solid_offsets(case)))
    b = offs[-1]
    a = max(offs[:-1], key=lambda o: max(int(md["LightTriCount"][r]) for r in range(len(md)) if int(md["LightNodeOffset"][r]) == o))
    pair = next(b + int(nodes["left"][k]) for k in range(b, len(nodes))
                if nodes["left"][k] >= 0 and (nodes["left"][[b + nodes["left"][k], b + nodes["left"][k] + 1]] < 0).all())
    leaf = next(k for k in range(a + 2, offs[offs.index(a) + 1]) if nodes["left"][k] < 0)
    nodes["left"][leaf] = pair - a
    return tthip.Lights(nodes, case.lights.tris.copy(), case.lights.meshes)
