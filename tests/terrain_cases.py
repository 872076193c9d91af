"""The terrain test scene and its seeded ray sets, shared by tests/test_terrain_host.py (which asserts the
coverage conditions on the host reference's output) and tests/test_gpu_terrain.py (which compares the GPU with
that reference bit for bit).

Layout: a Cornell box ([-1, 1]^3) stands on terrain 0 (8 x 8 units, hills up to ~0.64 above its base at
y = -1.6, so the hill tops poke through the box floor at y = -1); terrain 1 (4 x 4 units, base y = -1.2) overlaps
terrain 0 in x in [2, 4] and continues to x = 6, beyond terrain 0's footprint. The 64 x 48 atlas holds terrain 0
on the 33 x 33 rectangle at texel (4, 3) and terrain 1 on the 17 x 17 rectangle at texel (44, 20); terrain 1's
left half is a plateau (constant height 0.5), which is where a ray skimming the surface spends all 2,000 steps.

The same scene, with the head of the ray sets, is compared with a float64 heightmap surface instead of the host
reference in tests/test_terrain_geometry_host.py and tests/test_gpu_terrain_geometry.py (tests/terrain_geometry.py,
tests/terrain_geometry_cases.py).
"""
import functools

import numpy as np

import tthip

ATLAS_W, ATLAS_H = 64, 48
FAR = 1000.0
G = np.float32(0.44721359549995793928)  # sin(atan(1/2))
RECT0 = (4, 3, 33, 33)    # x, y, w, h in texels
RECT1 = (44, 20, 17, 17)
PLATEAU = 0.5


def _rect_uv(rect):
    """HeightMap = (xy: atlas uv of the terrain's uv = 1 corner, zw: of its uv = 0 corner): texel centres of the
    rectangle's first and last texels, so the filter never reads outside the rectangle."""
    x, y, w, h = rect
    return ((x + w - 0.5) / ATLAS_W, (y + h - 0.5) / ATLAS_H, (x + 0.5) / ATLAS_W, (y + 0.5) / ATLAS_H)


@functools.lru_cache(maxsize=None)
def atlas() -> np.ndarray:
    a = np.zeros((ATLAS_H, ATLAS_W), np.float16)
    x, y, w, h = RECT0
    a[y:y + h, x:x + w] = tthip.synthetic_heightmap(0x7E44A1, w, h).view(np.float16)
    x, y, w, h = RECT1
    t1 = tthip.synthetic_heightmap(0x7E44A2, w, h).view(np.float16).copy()
    t1[:, : w // 2 + 1] = PLATEAU
    a[y:y + h, x:x + w] = t1
    out = a.view(np.uint16).copy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def terrains() -> np.ndarray:
    t = np.zeros(2, tthip.TERRAIN_DTYPE)
    t[0]["PositionOffset"] = (-4.0, -1.6, -4.0)
    t[0]["HeightScale"] = 0.35
    t[0]["TerrainDim"] = (8.0, 8.0)
    t[0]["HeightMap"] = _rect_uv(RECT0)
    t[1]["PositionOffset"] = (2.0, -1.2, -2.0)
    t[1]["HeightScale"] = 0.5
    t[1]["TerrainDim"] = (4.0, 4.0)
    t[1]["HeightMap"] = _rect_uv(RECT1)
    t["AlphaMap"] = (1.0, 1.0, 0.0, 0.0)
    t["MatOffset"] = (3, 4)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def scene():
    return tthip.single_object_scene(tthip.Mesh.cornell())


def miss_records(rays: np.ndarray, far: float = FAR):
    """hits = (0, 0, asuint(FarPlane), 0): what tt_generate_primary leaves (no triangle hit yet)."""
    rays["hits"][:] = 0
    rays["hits"][:, 2] = np.float32(far).view(np.uint32)


def _normalize(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


N_RANDOM = 4099          # not a multiple of 64
RW, RH = 80, 64          # the screen the randomized set's PixelIndex values live on (RW * RH >= N_RANDOM)
PLATEAU_Y = np.float32(-1.2) + np.float32(0.01) + np.float32(2.0 * 0.5 * PLATEAU)  # terrain 1's plateau surface


@functools.lru_cache(maxsize=None)
def random_rays() -> np.ndarray:
    """The randomized set: N_RANDOM rays (origin, direction, PixelIndex; records unset) in seven groups, each
    aimed at one of the paths the march can take."""
    rng = np.random.default_rng(0x7E44A3)
    o, d = [], []

    def add(origins, targets=None, dirs=None):
        origins = np.asarray(origins, np.float64)
        o.append(origins.astype(np.float32))
        d.append(_normalize(targets - origins) if dirs is None else _normalize(dirs))

    n = 1200  # from above onto terrain 0 outside the box footprint: plain hits
    tx = rng.uniform(-3.9, 3.9, (n, 3)) * (1, 0, 1) + (0, -1.4, 0)
    add(rng.uniform(-3, 3, (n, 3)) * (1, 0, 1) + (0, 1, 0) * rng.uniform(1.5, 5.0, (n, 1)), tx)
    n = 600   # into the Cornell box from its open front, down onto the floor: triangle hits cull the terrain
    fl = np.stack([rng.uniform(-0.9, 0.9, n), np.full(n, -1.0), rng.uniform(-0.9, 0.6, n)], 1)
    add(np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(0.0, 0.8, n), np.full(n, 3.4)], 1), fl)
    n = 500   # over terrain 0 (through its box, above its hills) onto the part of terrain 1 beyond it
    t1 = np.stack([rng.uniform(4.3, 5.9, n), np.full(n, -0.8), rng.uniform(-1.8, 1.8, n)], 1)
    add(np.stack([rng.uniform(-3.5, 1.5, n), rng.uniform(1.0, 3.0, n), rng.uniform(-3, 3, n)], 1), t1)
    n = 300   # from below the surface inside terrain 0's box, upwards: the bisection
    add(np.stack([rng.uniform(-3.8, 3.8, n), rng.uniform(-1.57, -1.45, n), rng.uniform(-3.8, 3.8, n)], 1),
        dirs=np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(0.3, 1.0, n), rng.uniform(-0.5, 0.5, n)], 1))
    n = 24    # skimming terrain 1's plateau 2.5e-4 .. 6e-4 above it: 2,000 steps and still going
    add(np.stack([rng.uniform(2.2, 3.6, n), PLATEAU_Y + rng.uniform(2.5e-4, 6e-4, n), np.full(n, -1.9)], 1),
        dirs=np.tile((0.0, 0.0, 1.0), (n, 1)))
    n = 500   # away from everything, and axis-aligned directions (zero components: infinite reciprocals)
    dirs = rng.uniform(-1, 1, (n, 3)) * (1, 0, 1) + (0, 1, 0) * rng.uniform(0.05, 1.0, (n, 1))
    axis = np.array([(1, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0)], np.float64)
    dirs[:120] = axis[rng.integers(0, 6, 120)]
    add(rng.uniform(-5, 7, (n, 3)) * (1, 0, 1) + (0, 1, 0) * rng.uniform(-1.0, 4.0, (n, 1)), dirs=dirs)
    n = N_RANDOM - sum(len(x) for x in o)  # the rest: anywhere to anywhere
    add(rng.uniform(-6, 8, (n, 3)) * (1, 0.5, 1) + (0, 1.0, 0), rng.uniform(-5, 7, (n, 3)) * (1, 0.3, 1) + (0, -1.0, 0))
    rays = np.zeros(N_RANDOM, tthip.RAY_DTYPE)
    order = rng.permutation(N_RANDOM)  # the groups interleaved, as a wavefront's rays are
    rays["origin"] = np.concatenate(o)[order]
    rays["direction"] = np.concatenate(d)[order]
    rays["PixelIndex"] = rng.permutation(RW * RH)[:N_RANDOM]
    rays["last_pdf"] = 1.0
    miss_records(rays)
    rays.setflags(write=False)
    return rays


N_SHADOW = 4096
SW, SH = 64, 64


@functools.lru_cache(maxsize=None)
def shadow_rays() -> np.ndarray:
    """4,096 NEE rays, one per pixel of a 64 x 64 screen: from points near the terrain surfaces and the box towards
    lights above and to the sides; t > 0, t < 0 and (one in eight) t == 0."""
    rng = np.random.default_rng(0x7E44A4)
    n = N_SHADOW
    s = np.zeros(n, tthip.SHADOW_DTYPE)
    org = np.stack([rng.uniform(-3.9, 5.9, n), rng.uniform(-1.5, 0.5, n), rng.uniform(-3.9, 3.9, n)], 1)
    light = np.stack([rng.uniform(-8, 10, n), rng.uniform(-1.4, 6.0, n), rng.uniform(-8, 8, n)], 1)
    dist = np.linalg.norm(light - org, axis=1)
    s["origin"] = org.astype(np.float32)
    s["direction"] = _normalize(light - org)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    t = (dist * sign).astype(np.float32)
    t[rng.random(n) < 0.125] = 0.0
    s["t"] = t
    s["illumination"] = rng.uniform(0.0, 4.0, (n, 3)).astype(np.float32)
    # LuminanceIncomming carries a packed RGBE colour (read as asuint under UseReSTIRGI)
    s["LuminanceIncomming"] = rng.integers(0x10101010, 0x7f7f7f7f, n, dtype=np.uint32).view(np.float32)
    s["PixelIndex"] = rng.permutation(SW * SH)
    s.setflags(write=False)
    return s
