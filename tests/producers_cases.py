"""The cameras, scenes, ray sets, comparisons and control mutants of the float64 producer pin, shared by
tests/test_producers_host.py (the oracle against tests/producers.py) and tests/test_gpu_producers.py (the kernels
against it). Nothing here calls the oracle or the engine: a test hands in a `side`, an object with

    generate(c2w, ip, W, H, near, far, jitter, frames, max_bounce) -> the 2 W H ray buffer
    trace(scene, buf, n, bounce, W, H)                               in place
    resolve(scene, buf, n, bounce, W, H) -> (n, 6) float32
    enqueue(scene, buf, n, bounce, W, H, frames, max_bounce, frame_pixels) -> survivor count, in place

Caps, conditions on the cases and not measurements of the code under test: at most MAX_OPEN = 0.5 % of a case's rays
may be marginal (the in-plane and pdf = 0 rays of the synthetic edge set are marginal by construction and are
asserted to be); the coverage counts of COVERAGE must be met by the model's own classification."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import producers as P
import tthip

FAR = 1000.0
NEAR = 0.05
MAX_OPEN = 0.005
U = P.U24
TILE = 4096
COVERAGE = {"helper z": 200, "x band": 200, "flipped": 200, "unflipped": 200, "mirrored": 100, "far": 100}


class Report:
    def __init__(self):
        self.bad = {}      # assertion -> indices of the rays (rows) that violate it
        self.worst = {}    # measured extremes, as fractions of their bounds where a bound exists
        self.counts = {}

    def add(self, what, idx):
        idx = np.asarray(idx)
        if len(idx):
            self.bad[what] = idx

    def ratio(self, what, err, tol):
        if len(err):
            self.worst[what] = max(self.worst.get(what, 0.0), float(np.max(err / tol)))

    def names(self):
        return set(self.bad)

    def check(self):
        assert not self.bad, {k: v[:8].tolist() for k, v in self.bad.items()} | {"worst": self.worst}
        return self

    def say(self, name):
        print(f"{name}: " + ", ".join(f"{k} {v:.3g}" for k, v in self.worst.items())
              + (" | " + ", ".join(f"{k} {v}" for k, v in self.counts.items()) if self.counts else ""))
        return self


# ------------------------------------------------------------------ cameras and Generate
CAMERAS = {
    "axis": P.Camera((0.0, 0.0, -5.0), (0, 0, 1), (0, 1, 0), 60.0),
    "oblique": P.Camera((1.5, 2.0, -6.0), (-0.3, -0.35, 1.0), (0.25, 1.0, -0.15), 60.0),
    "narrow": P.Camera((1.5, 2.0, -6.0), (-0.3, -0.35, 1.0), (0.25, 1.0, -0.15), 5.0),
    "wide": P.Camera((1.5, 2.0, -6.0), (0.4, -0.1, 1.0), (-0.3, 1.0, 0.2), 120.0),
    "shift": P.Camera((-2.0, 1.0, 7.0), (0.2, -0.2, -1.0), (0.1, 1.0, 0.3), 45.0, shift=(0.3, -0.2)),
}
SIZES = ((1, 1), (3, 2), (257, 3), (64, 65))
PARAMS = [(j, f, m) for j in (0, 1) for f in (0, 3, 0x7FFFFFFF) for m in (1, 5)]


def generate_cases():
    """(camera name, W, H, jitter, frames, max_bounce): every camera at every size, the twelve parameter sets dealt
    round so that each occurs, every camera and every size with jitter on and off."""
    out = []
    for ci, cn in enumerate(CAMERAS):
        for si, (w, h) in enumerate(SIZES):
            for k in (0, 7):
                out.append((cn, w, h) + PARAMS[(5 * ci + 3 * si + k) % len(PARAMS)])
    assert {c[3:] for c in out} == set(PARAMS)
    return out


def camera_matrices(cam: P.Camera, W, H):
    """(cameraToWorldMatrix, projectionMatrix.inverse) in float64 as Unity lays them out, the lens shift in
    P[0, 2], P[1, 2] (tthip.unity_camera has none)."""
    r, u, f = cam.basis()
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, u, -f, cam.position
    ft = 1.0 / np.tan(np.deg2rad(cam.vfov_deg) / 2.0)
    n, fa = cam.near, cam.far
    Pm = np.zeros((4, 4))
    Pm[0, 0], Pm[1, 1] = ft / (W / H), ft
    Pm[0, 2], Pm[1, 2] = cam.shift
    Pm[2, 2], Pm[2, 3] = (fa + n) / (n - fa), 2 * fa * n / (n - fa)
    Pm[3, 2] = -1.0
    return c2w, np.linalg.inv(Pm)


def rays_from_matrices(c2w, ip, W, H, near, far, jitter, frames, max_bounce, centre=0.5):
    """Generate through the matrices in float64, rounded to RayData: the cross-check of camera_matrices against the
    parametric model, and the source of the Generate mutants (a transposed c2w, dropped lens terms, centre = 0)."""
    n = W * H
    p = np.arange(n)
    jx = jy = np.zeros(n)
    if jitter:
        rx, ry = P.random2(0, p, frames, max_bounce, 0)
        jx, jy = rx.astype(np.float64) - centre, ry.astype(np.float64) - centre
    uvx, uvy = (p % W + jx) / W * 2 - 1, (p // W + jy) / H * 2 - 1
    d = np.stack([ip[k, 0] * uvx + ip[k, 1] * uvy + ip[k, 3] for k in range(3)], 1) @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(2 * n, tthip.RAY_DTYPE)
    rays["origin"][:n] = c2w[:3, 3] + near * d
    rays["direction"][:n] = d
    rays["PixelIndex"][:n] = p
    rays["hits"][:n, 2] = np.array([far], np.float32).view(np.uint32)[0]
    return rays


def compare_generate(cam, W, H, jitter, frames, max_bounce, rays) -> Report:
    r = Report()
    n = W * H
    e = P.generate(cam, W, H, jitter, frames, max_bounce)
    g = rays[:n]
    r.add("PixelIndex", np.nonzero(g["PixelIndex"] != np.arange(n))[0])
    r.add("last_pdf bits", np.nonzero(g["last_pdf"].view(np.uint32) != 0)[0])
    want = np.array([0, 0, np.array([cam.far], np.float32).view(np.uint32)[0], 0], np.uint32)
    r.add("hits", np.nonzero((g["hits"] != want).any(1))[0])
    d = g["direction"].astype(np.float64)
    ed = np.linalg.norm(d - e.direction, axis=1)
    r.add("direction", np.nonzero(~(ed <= e.tol_d))[0])
    eo = np.linalg.norm(g["origin"].astype(np.float64) - e.origin, axis=1)
    r.add("origin", np.nonzero(~(eo <= e.tol_o))[0])
    r.add("direction not a unit vector", np.nonzero(~(np.abs(np.linalg.norm(d, axis=1) - 1) <= 4 * U))[0])
    r.ratio("direction", ed, e.tol_d)
    r.ratio("origin", eo, e.tol_o)
    return r


def compare_jitter(cam, W, H, rays_by_frames) -> Report:
    """rays_by_frames: {frames: jittered rays}. jx + 0.5 and jy + 0.5 recovered from the directions against U(0, 1),
    and different offsets for different frames: two independent offsets lie within 1e-3 of each other on one axis
    with probability 2e-3, so more than 1 % of the pixels doing so on both axes is no accident."""
    r = Report()
    n = W * H
    js = {}
    for fr, rays in rays_by_frames.items():
        j = P.screen_jitter(cam, W, H, rays["direction"][:n]) + 0.5
        js[fr] = j
        for axis, name in ((0, "x"), (1, "y")):
            D = P.ks_statistic(np.clip(j[:, axis], 0, 1))
            r.ratio(f"jitter {name} KS", np.array([D]), P.ks_limit(n))
            if D > P.ks_limit(n):
                r.add(f"jitter {name} not uniform over the footprint", [fr])
    keys = list(js)
    for a, b in zip(keys, keys[1:]):
        same = (np.abs(js[a] - js[b]) < 1e-3).all(1).mean()
        if same > 0.01:
            r.add("same jitter in different frames", [a, b])
    return r


# ------------------------------------------------------------------ scenes
def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def trs(centre, R, scale):
    m = np.eye(4)
    m[:3, :3] = R @ np.diag(np.asarray(scale, np.float64))
    m[:3, 3] = centre
    return m


# (centre, R, scale): the identity, a skew-axis rotation with a non-uniform scale, a mirrored parent, a far copy
PARENTS = (
    ((0.0, 0.0, 0.0), np.eye(3), (1.0, 1.0, 1.0)),
    ((3.4, 0.3, 1.5), rotation((1, 2, 3), 40.0), (3.0, 1.0, 0.5)),
    ((-2.9, -0.2, 0.8), rotation((0.3, 1.0, -0.2), 65.0), (-1.5, 1.0, 1.0)),
    ((500.0, 500.5, 499.0), np.eye(3), (1.0, 1.0, 1.0)),
)
MIRRORED, FAR_PARENT = 2, 3


def icosphere(level=3):
    """A unit icosphere: 20 * 4^level triangles (1,280 at level 3), vertex normals equal to positions."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v), np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """"ellipsoid": the icosphere under the four PARENTS; "soup" / "instances": the brute-force pin's scenes.
    Shared between tests: do not write to it."""
    if name != "ellipsoid":
        import bruteforce_cases as BFC
        return BFC.scene(name)
    pos, idx = icosphere()
    am = tthip.AssetManager()
    blases = [tthip.Blas(tthip.ArrayMesh(pos, idx, normals=pos)) for _ in PARENTS]
    for b, (c, R, s) in zip(blases, PARENTS):
        am.add_parent(b, trs(c, R, s))
    sc = am.build()
    assert len(sc.meshdata) == len(PARENTS) and len(sc.tris) == len(PARENTS) * len(idx)
    return sc


TRACED = {  # name -> (scene, camera, W, H): 96 x 96 is two full 4,096-ray tiles and a ragged third
    "near": ("ellipsoid", P.Camera((0.4, 2.2, -8.5), (0.0, -0.22, 1.0), (0.2, 1.0, 0.1), 55.0), 96, 96),
    "far": ("ellipsoid", P.Camera((500.6, 501.4, 495.6), (-0.15, -0.22, 1.0), (-0.1, 1.0, 0.2), 40.0), 40, 40),
    "soup": ("soup", P.Camera((0.9, 1.3, -3.4), (-0.25, -0.36, 1.0), (0.2, 1.0, -0.1), 60.0), 96, 96),
    "instances": ("instances", P.Camera((2.0, 7.0, -14.0), (-0.12, -0.45, 1.0), (-0.15, 1.0, 0.1), 65.0), 96, 96),
}
TRACED_FRAMES, TRACED_MAXB = 3, 5


# ------------------------------------------------------------------ synthetic ray sets
def _tri_ranges(sc):
    off = sc.meshdata["TriOffset"].astype(np.int64)
    starts = sorted(set(off.tolist()))
    ends = dict(zip(starts, starts[1:] + [len(sc.tris)]))
    return off, np.array([ends[int(o)] for o in off])


def records(sc, n, seed, reach=(0.5, 3.0)):
    """n rays whose records name valid (mesh, triangle) pairs with random packed barycentrics, random unit directions
    and the origin t behind the point the record names, one pixel each (PixelIndex = a permutation's head is the
    caller's). Returns (rays, world point)."""
    rng = np.random.default_rng(seed)
    lo, hi = _tri_ranges(sc)
    mesh = rng.integers(0, len(lo), n)
    tri = lo[mesh] + (rng.random(n) * (hi - lo)[mesh]).astype(np.int64)
    a, b = rng.random(n), rng.random(n)
    a, b = np.where(a + b > 1, 1 - a, a), np.where(a + b > 1, 1 - b, b)
    cu, cv = np.rint(a * 65535).astype(np.uint32), np.rint(b * 65535).astype(np.uint32)
    cv = np.minimum(cv, 65535 - cu)
    d = P._unit(rng.normal(size=(n, 3)))
    t = rng.uniform(*reach, n)
    return make_rays(sc, mesh, tri, cu, cv, d, t)


def world_point(sc, mesh, tri, cu, cv):
    T = sc.tris[tri]
    obj = (T["pos0"].astype(np.float64) + (cu / 65535.0)[:, None] * T["posedge1"].astype(np.float64)
           + (cv / 65535.0)[:, None] * T["posedge2"].astype(np.float64))
    L = np.linalg.inv(P.w2l_rows(sc.meshdata))[mesh]
    return P._apply(L[:, :3, :3], obj) + L[:, :3, 3]


def make_rays(sc, mesh, tri, cu, cv, d, t):
    n = len(mesh)
    assert (np.asarray(tri) < len(sc.tris)).all() and (np.asarray(mesh) < len(sc.meshdata)).all()
    rays = np.zeros(n, tthip.RAY_DTYPE)
    p = world_point(sc, mesh, tri, cu, cv)
    d32 = np.asarray(d, np.float64).astype(np.float32)
    t32 = np.asarray(t, np.float64).astype(np.float32)
    rays["origin"] = p - d32.astype(np.float64) * t32.astype(np.float64)[:, None]
    rays["direction"] = d32
    rays["last_pdf"] = 1.0
    rays["hits"] = np.stack([np.asarray(mesh, np.uint32), np.asarray(tri, np.uint32), t32.view(np.uint32),
                             (np.asarray(cu, np.uint32) | (np.asarray(cv, np.uint32) << 16))], 1)
    return rays


def kill(rays, dead, seed=1):
    """Dead rays: t >= far (the far plane itself, or beyond) and triangle_id 0xFFFFFFFF (the miss record), mixed."""
    rng = np.random.default_rng(seed)
    dead = np.nonzero(dead)[0]
    how = rng.integers(0, 3, len(dead))
    far_bits = np.array([FAR, 2 * FAR], np.float32).view(np.uint32)
    rays["hits"][dead[how == 0], 2] = far_bits[0]
    rays["hits"][dead[how == 1], 2] = far_bits[1]
    rays["hits"][dead[how == 2], 1] = 0xFFFFFFFF
    return rays


@dataclasses.dataclass
class EnqueueCase:
    name: str
    scene: object            # a name scene() knows, or a tthip.Scene
    src: np.ndarray
    W: int
    H: int
    bounce: int = 0
    frames: int = TRACED_FRAMES
    max_bounce: int = TRACED_MAXB
    frame_pixels: int = 0
    order_only: bool = False
    by_construction: np.ndarray = None   # source rays that are marginal by construction (outside the cap)


COVER_W = COVER_H = 96


@functools.lru_cache(maxsize=None)
def coverage_case() -> EnqueueCase:
    """The ellipsoid scene's synthetic set: 40,000 candidate records, of which 400 whose smooth normal has |x| in
    (0.99, 1], 400 with |x| in [0.95, 0.99), and 6,000 as they come; then the edge records. One frame, one pixel each."""
    sc = scene("ellipsoid")
    cand = records(sc, 40000, 0x9A01)
    nm = P.restated_normals(sc.tris, sc.meshdata, cand["hits"][:, 0], cand["hits"][:, 1], cand["hits"][:, 3])
    ax = np.abs(nm.g[:, 0])
    pick = np.concatenate([np.nonzero(ax > 0.99)[0][:400], np.nonzero((ax >= 0.95) & (ax < 0.99))[0][:400],
                           np.arange(6000) + 30000])
    rays = cand[np.sort(pick)].copy()
    edge, by_con = edge_records(sc)
    rays = np.concatenate([rays, edge])
    n = len(rays)
    assert n <= COVER_W * COVER_H
    perm = np.random.default_rng(0x9A02).permutation(COVER_W * COVER_H)
    perm = np.concatenate([perm[perm != PDF0_PIXEL][:n - 1], [PDF0_PIXEL]])   # the last edge record is the pdf = 0 one
    rays["PixelIndex"] = perm
    assert by_con[-1] == 2
    assert len(np.unique(rays["PixelIndex"])) == n
    mark = np.zeros(n, bool)
    mark[n - len(edge):] = by_con > 0
    rays.setflags(write=False)
    return EnqueueCase("coverage", "ellipsoid", rays, COVER_W, COVER_H, frames=PDF0_FRAMES, by_construction=mark)


# random(1, PDF0_PIXEL) at frames PDF0_FRAMES, max_bounce 5, bounce 0 has rx = 2.07e-8: a = 2 rx - 1 is one float32
# step from -1, 1 - r^2 = 8.3e-8 is below the 24 u that float32 resolves there, and whether pdf comes out as 0 is the
# rounding's choice (the model: open). Found by a search of frames 0..2999 over the exact generator;
# tests/test_producers_host.py asserts the class.
PDF0_PIXEL, PDF0_FRAMES = 5620, 2751


def edge_records(sc):
    """(rays, by-construction class: 0 none, 1 direction in the triangle's plane, 2 pdf = 0). u + v = 1, u = 0, t
    tiny, in-plane directions, on every parent; each twice with the same record (two rays that share a normal)."""
    rng = np.random.default_rng(0x9A03)
    lo, hi = _tri_ranges(sc)
    mesh = np.repeat(np.arange(len(lo)), 24)
    n = len(mesh)
    tri = lo[mesh] + (rng.random(n) * (hi - lo)[mesh]).astype(np.int64)
    kind = np.arange(n) % 4
    cu = rng.integers(0, 65536, n).astype(np.uint32)
    cv = (rng.random(n) * (65535 - cu)).astype(np.uint32)
    cv = np.where(kind == 0, 65535 - cu, cv)            # u + v = 1
    cu = np.where(kind == 1, 0, cu)                     # u = 0
    d = P._unit(rng.normal(size=(n, 3)))
    t = np.where(kind == 2, 1e-6, rng.uniform(0.5, 2.0, n))   # t tiny
    T = sc.tris[tri]
    L = np.linalg.inv(P.w2l_rows(sc.meshdata))[mesh][:, :3, :3]
    inplane = P._unit(P._apply(L, T["posedge1"].astype(np.float64)) * rng.uniform(0.2, 1, (n, 1))
                      + P._apply(L, T["posedge2"].astype(np.float64)) * rng.uniform(0.2, 1, (n, 1)))
    d = np.where((kind == 3)[:, None], inplane, d)
    rays = make_rays(sc, mesh, tri, cu, cv, d, t)
    rays = np.concatenate([rays, rays, rays[:1]])       # every record twice; one more for the pdf = 0 pixel
    by_con = np.concatenate([kind == 3, kind == 3, [False]]).astype(np.int64)
    by_con[-1] = 2
    return rays, by_con


@functools.lru_cache(maxsize=None)
def resolve_case() -> EnqueueCase:
    """The coverage records at the odd bounce's offset, every fifth made a record the resolve writes six zeros for:
    a miss, t at or past the far plane, a triangle id past the scene's triangles, a mesh id past its records."""
    c = coverage_case()
    sc = scene(c.scene)
    rays = c.src.copy()
    bad = np.nonzero(np.arange(len(rays)) % 5 == 0)[0]
    kill(rays, np.isin(np.arange(len(rays)), bad[::2]))
    rest = bad[1::2]
    rays["hits"][rest[::2], 1] = len(sc.tris) + np.arange(len(rest[::2]), dtype=np.uint32) * 977
    rays["hits"][rest[1::2], 0] = len(sc.meshdata) + np.arange(len(rest[1::2]), dtype=np.uint32) % 3
    rays.setflags(write=False)
    return EnqueueCase("resolve", c.scene, rays, c.W, c.H, bounce=1)


PATTERN_N = 2 * TILE + 65        # two tiles, one wave and one lane
PATTERN_W, PATTERN_H = 128, 65
PATTERNS = ("all dead", "all live", "alternating", "one per wave", "last lane of a tile")


@functools.lru_cache(maxsize=None)
def pattern_case(name) -> EnqueueCase:
    sc = scene("ellipsoid")
    rays = records(sc, PATTERN_N, 0x9B00 + PATTERNS.index(name))
    i = np.arange(PATTERN_N)
    live = {"all dead": np.zeros(PATTERN_N, bool), "all live": np.ones(PATTERN_N, bool), "alternating": i % 2 == 1,
            "one per wave": i % 64 == (i // 64 * 7) % 64, "last lane of a tile": i % TILE == TILE - 1}[name]
    kill(rays, ~live)
    rays["PixelIndex"] = np.random.default_rng(0x9B10).permutation(PATTERN_W * PATTERN_H)[:PATTERN_N]
    rays.setflags(write=False)
    return EnqueueCase(name, "ellipsoid", rays, PATTERN_W, PATTERN_H, frames=0, max_bounce=1)


LOOKBACK_N = 65 * TILE + 1         # 266,241 rays: the 66th tile's look-back window slides once
LOOKBACK_W, LOOKBACK_H = 517, 515


@functools.lru_cache(maxsize=None)
def lookback_case() -> EnqueueCase:
    sc = scene("ellipsoid")
    rays = records(sc, LOOKBACK_N, 0x9C00)
    rng = np.random.default_rng(0x9C01)
    # tiles 1..64 alternate between sparse and dense, so the counts the window sums differ from tile to tile
    dead = rng.random(LOOKBACK_N) < np.where((np.arange(LOOKBACK_N) // TILE) % 2 == 0, 0.2, 0.8)
    kill(rays, dead)
    rays["PixelIndex"] = rng.permutation(LOOKBACK_W * LOOKBACK_H)[:LOOKBACK_N]
    rays.setflags(write=False)
    return EnqueueCase("look-back", "ellipsoid", rays, LOOKBACK_W, LOOKBACK_H, frames=0x7FFFFFFF, max_bounce=1,
                       order_only=True)


BATCH_W = BATCH_H = 48


@functools.lru_cache(maxsize=None)
def batched_case() -> EnqueueCase:
    """Two 48 x 48 frames as one 48 x 96 screen: frame j's rays carry PixelIndex + j W H, frame_pixels = W H."""
    sc = scene("ellipsoid")
    n = BATCH_W * BATCH_H
    rays = records(sc, 2 * n, 0x9D00)
    kill(rays, np.random.default_rng(0x9D01).random(2 * n) < 0.3)
    rng = np.random.default_rng(0x9D02)
    rays["PixelIndex"] = np.concatenate([rng.permutation(n), rng.permutation(n) + n])
    rays.setflags(write=False)
    return EnqueueCase("batched", "ellipsoid", rays, BATCH_W, 2 * BATCH_H, frames=0x7FFFFFFF, frame_pixels=n)


def scene_of(c: EnqueueCase):
    return scene(c.scene) if isinstance(c.scene, str) else c.scene


# ------------------------------------------------------------------ drivers
def frame_buffer(c: EnqueueCase):
    """The 2 W H buffer with the case's rays in the half its bounce reads; every other byte is 0xA5."""
    wh = c.W * c.H
    buf = np.zeros(2 * wh, tthip.RAY_DTYPE)
    buf.view(np.uint8)[:] = 0xA5
    off = wh if c.bounce % 2 == 1 else 0
    buf[off:off + len(c.src)] = c.src
    return buf, off, wh - off


def run_enqueue(side, c: EnqueueCase):
    """(count, the destination half's first `count` rows as written, Report of the buffer-level checks: the source
    half untouched, nothing written past the survivors)."""
    buf, off, dst = frame_buffer(c)
    before = buf.copy()
    n = len(c.src)
    count = side.enqueue(scene_of(c), buf, n, c.bounce, c.W, c.H, c.frames, c.max_bounce, c.frame_pixels)
    r = Report()
    wh = c.W * c.H
    if not np.array_equal(buf[off:off + wh].view(np.uint8), before[off:off + wh].view(np.uint8)):
        r.add("source half written", [0])
    count = int(count)
    tail = slice(dst + min(count, wh), dst + wh)
    if not np.array_equal(buf[tail].view(np.uint8), before[tail].view(np.uint8)):
        r.add("written past the survivors", [count])
    return count, buf[dst:dst + min(count, wh)].copy(), r


def traced_chain(side, name):
    """Generate, trace, resolve and enqueue at bounce 0, then trace, resolve and enqueue at bounce 1 (the odd bounce:
    the second half is the source, the first the destination). Yields (stage, Report)."""
    sname, cam, W, H = TRACED[name]
    sc = scene(sname)
    wh = W * H
    c2w, ip = camera_matrices(cam, W, H)
    buf = side.generate(c2w, ip, W, H, cam.near, cam.far, 1, TRACED_FRAMES, TRACED_MAXB)
    yield "generate", compare_generate(cam, W, H, 1, TRACED_FRAMES, TRACED_MAXB, buf)
    n = wh
    for b in (0, 1):
        off, dst = (wh, 0) if b else (0, wh)
        side.trace(sc, buf, n, b, W, H)
        src = buf[off:off + n].copy()
        yield f"resolve {b}", compare_resolve(sc, src, side.resolve(sc, buf, n, b, W, H), sname == "ellipsoid")
        count = side.enqueue(sc, buf, n, b, W, H, TRACED_FRAMES, TRACED_MAXB, 0)
        c = EnqueueCase(f"{name} {b}", sname, src, W, H, b, TRACED_FRAMES, TRACED_MAXB)
        rep = compare_bounce(c, count, buf[dst:dst + count].copy())
        if not np.array_equal(buf[off:off + n], src):
            rep.add("source half written", [0])
        yield f"bounce {b}", rep
        n = count


# ------------------------------------------------------------------ the normal resolve
def valid_records(sc, src):
    t = src["hits"][:, 2].copy().view(np.float32)
    return (t < np.float32(FAR)) & (src["hits"][:, 1] < len(sc.tris)) & (src["hits"][:, 0] < len(sc.meshdata))


def compare_resolve(sc, src, out6, ellipsoid=False) -> Report:
    """src: the launch's rays (the window); out6: the (n, 6) rows written."""
    r = Report()
    out6 = np.asarray(out6)
    ok = valid_records(sc, src)
    r.add("six zeros", np.nonzero(~ok & (out6.view(np.uint32) != 0).any(1))[0])
    w = np.nonzero(ok)[0]
    s = src[w]
    g32, us32 = out6[w, :3].astype(np.float64), out6[w, 3:].astype(np.float64)
    mesh, tri = s["hits"][:, 0].astype(np.int64), s["hits"][:, 1].astype(np.int64)
    nm = P.restated_normals(sc.tris, sc.meshdata, mesh, tri, s["hits"][:, 3])
    firm = ~nm.marginal
    eg, eu = np.linalg.norm(g32 - nm.g, axis=1), np.linalg.norm(us32 - nm.us, axis=1)
    well = nm.cond <= P.COND_MAX
    r.add("smooth normal", w[well & ~(eg <= nm.tol_g)])
    r.add("unsmoothed normal", w[firm & ~(eu <= nm.tol_us)])
    geo, _ = P.geometric_normal(sc.tris, sc.meshdata, mesh, tri, nm.g)
    ew = np.linalg.norm(us32 - geo, axis=1)
    r.add("unsmoothed normal against the world triangle", w[firm & ~(ew <= nm.tol_us)])
    for v, what in ((g32, "smooth"), (us32, "unsmoothed")):
        r.add(f"{what} normal not a unit vector", w[~(np.abs(np.linalg.norm(v, axis=1) - 1) <= 4 * U)])
    r.ratio("smooth normal", eg[well], nm.tol_g[well])
    r.ratio("unsmoothed normal", eu[firm], nm.tol_us[firm])
    r.ratio("unsmoothed normal against the world triangle", ew[firm], nm.tol_us[firm])
    r.worst["smooth normal, absolute"] = float(eg[well].max()) if well.any() else 0.0
    if ellipsoid:
        o, d = s["origin"].astype(np.float64), s["direction"].astype(np.float64)
        t = s["hits"][:, 2].copy().view(np.float32).astype(np.float64)
        p = o + d * t[:, None]
        for m, (c, R, sc_) in enumerate(PARENTS):
            k = mesh == m
            if not k.any():
                continue
            want = P.analytic_ellipsoid_normal(p[k], c, R, sc_)
            bound = P.analytic_ellipsoid_bound(sc.tris, tri[k], p[k], o[k], t[k], c, R, sc_)
            ea = np.linalg.norm(g32[k] - want, axis=1)
            r.add("smooth normal against the ellipsoid", w[k][~(ea <= bound)])
            r.ratio("smooth normal against the ellipsoid", ea, bound)
    r.counts.update(valid=int(ok.sum()), open=int((~firm).sum()))
    if ok.sum() and (~firm).sum() > MAX_OPEN * len(src):
        r.add("more than 0.5 % of the rays left open", [int((~firm).sum())])
    return r


# ------------------------------------------------------------------ the bounce
def compare_bounce(c: EnqueueCase, count, rows, model=None) -> Report:
    """count: what the enqueue returned; rows: the destination half's first `count` rays."""
    r = Report()
    sc, src = scene_of(c), c.src
    m = model if model is not None else P.bounce(sc.tris, sc.meshdata, src, FAR, c.bounce, c.frames, c.max_bounce,
                                                 c.frame_pixels, geometry=not c.order_only)
    opened = np.nonzero(m.open_pdf)[0]
    present = opened[np.isin(src["PixelIndex"][opened], rows["PixelIndex"])]
    expected = np.sort(np.concatenate([np.nonzero(m.firm)[0], present]))
    if count != len(expected) or len(rows) != count:
        r.add("survivor count", [count, len(expected)])
    k = min(len(rows), len(expected))
    e, got = expected[:k], rows[:k]
    pix_ok = got["PixelIndex"] == src["PixelIndex"][e]
    hits_ok = (got["hits"] == src["hits"][e]).all(1)
    if not pix_ok.all():
        same = len(rows) == len(expected) and np.array_equal(np.sort(rows["PixelIndex"]),
                                                             np.sort(src["PixelIndex"][expected]))
        r.add("source order" if same else "PixelIndex kept" if hits_ok[~pix_ok].all() else "survivor set",
              np.nonzero(~pix_ok)[0])
    r.add("hits not copied", np.nonzero(pix_ok & ~hits_ok)[0])
    r.counts.update(rays=len(src), survivors=len(expected))
    if c.order_only:
        return r
    ok = np.nonzero(pix_ok)[0]
    ci = np.searchsorted(m.idx, e[ok])
    g = got[ok]
    lb = m.lobe
    dd, pdf = g["direction"].astype(np.float64), g["last_pdf"].astype(np.float64)
    firm = ~m.marginal[ci]
    el = np.abs(np.linalg.norm(dd, axis=1) - 1)
    r.add("direction not a unit vector", ok[~(el <= 4 * U)])
    r.ratio("|direction| - 1", el, 4 * U)
    r.add("last_pdf not positive", ok[~(pdf > 0)])
    ep, tp = np.abs(pdf * np.pi - lb.om[ci, 1]), lb.tol_y[ci] + 3 * U
    r.add("last_pdf != omega_o.y / pi", ok[~lb.pdf_marginal[ci] & ~(ep <= tp)])
    r.ratio("last_pdf pi - omega_o.y", ep[~lb.pdf_marginal[ci]], tp[~lb.pdf_marginal[ci]])
    cosn = np.einsum("kj,kcj->kc", dd, m.norm[ci])
    cosn = np.where(m.norm_valid[ci], cosn, np.inf)
    e2 = np.abs(cosn - (pdf * np.pi)[:, None]).min(1)
    t2 = (P.K_FRAME + 3) * U + m.norm_slack[ci]
    r.add("direction . norm != last_pdf pi", ok[firm & ~(e2 <= t2)])
    r.ratio("direction . norm - last_pdf pi", e2[firm], t2[firm])
    e3 = np.abs(cosn - lb.om[ci, 1][:, None]).min(1)
    t3 = P.K_FRAME * U + lb.tol_y[ci] + m.norm_slack[ci]
    f3 = firm & ~lb.pdf_marginal[ci]
    r.add("direction . norm != disc sample", ok[f3 & ~(e3 <= t3)])
    r.ratio("direction . norm - disc sample", e3[f3], t3[f3])
    # two rays of one norm code: the angle between their directions is that between their omega_o
    single = f3 & ~m.norm_valid[ci][:, 1:].any(1) & ~lb.branch_marginal[ci]
    s = np.nonzero(single)[0]
    s = s[np.argsort(m.norm_code[ci][s], kind="stable")]
    a, b = s[:-1], s[1:]
    pair = m.norm_code[ci][a] == m.norm_code[ci][b]
    a, b = a[pair], b[pair]
    e4 = np.abs((dd[a] * dd[b]).sum(1) - (lb.om[ci[a]] * lb.om[ci[b]]).sum(1))
    t4 = (2 * P.K_FRAME + 28) * U + lb.tol_y[ci[a]] + lb.tol_y[ci[b]] + m.norm_slack[ci[a]] + m.norm_slack[ci[b]]
    r.add("angle between two rays of one normal", ok[a[~(e4 <= t4)]])
    r.ratio("pair angle", e4, t4)
    # the new origin against the world triangle's plane
    off = g["origin"].astype(np.float64) - m.pos[ci]
    dist = (off * m.n_side[ci]).sum(1)
    sure = ~m.marginal_flip[ci]
    e5, t5 = np.abs(dist - P.OFFSET), m.tol_origin[ci]
    r.add("origin offset", ok[sure & ~(e5 <= t5)])
    r.add("origin behind the surface", ok[sure & (t5 < P.OFFSET) & ~(dist > 0)])
    r.add("origin away from the hit point", ok[~(np.linalg.norm(off, axis=1) <= P.OFFSET + t5)])
    r.ratio("origin offset", e5[sure], t5[sure])
    ax = np.abs(m.norm[ci][:, 0, 0])
    n_open = int(m.marginal.sum())
    if c.by_construction is not None:
        n_open = int((m.marginal & ~c.by_construction[m.idx]).sum())
    r.counts.update({"pairs": int(len(a)), "helper z": int((firm & (ax > 0.99)).sum()),
                     "x band": int((firm & (ax >= 0.95) & (ax < 0.99)).sum()),
                     "flipped": int((firm & m.flipped[ci]).sum()), "unflipped": int((firm & ~m.flipped[ci]).sum()),
                     "mirrored": int((firm & (m.mesh[ci] == MIRRORED)).sum()) if c.scene == "ellipsoid" else 0,
                     "far": int((firm & (m.mesh[ci] == FAR_PARENT)).sum()) if c.scene == "ellipsoid" else 0,
                     "open": n_open, "two codes": int(m.norm_valid[:, 1:].any(1).sum())})
    if n_open > MAX_OPEN * len(src):
        r.add("more than 0.5 % of the rays left open", [n_open])
    return r


def compare_lobe(c: EnqueueCase, rows, model=None) -> Report:
    """cos^2(theta) against U(0, 1) and the azimuth about the model's frame against U, on one frame's survivors."""
    r = Report()
    sc = scene_of(c)
    m = model if model is not None else P.bounce(sc.tris, sc.meshdata, c.src, FAR, c.bounce, c.frames, c.max_bounce,
                                                 c.frame_pixels)
    pix = {int(p): i for i, p in enumerate(c.src["PixelIndex"][m.idx])}
    ci = np.array([pix.get(int(p), -1) for p in rows["PixelIndex"]])
    keep = (ci >= 0)
    keep[keep] &= ~m.marginal[ci[keep]]   # (a second candidate code moves norm by a grid step: nothing to a KS test)
    ci, dd = ci[keep], rows["direction"][keep].astype(np.float64)
    n = len(ci)
    r.counts["survivors"] = n
    if n < 4000:
        r.add("fewer than 4,000 survivors", [n])
        return r
    N = m.norm[ci][:, 0]
    cos2 = np.clip((dd * N).sum(1), 0, 1) ** 2
    T, B = P.tangent_frame(N)
    az = np.arctan2((dd * B).sum(1), (dd * T).sum(1)) / (2 * np.pi) + 0.5
    for x, what in ((cos2, "cosine lobe"), (az, "azimuth")):
        D = P.ks_statistic(x)
        r.ratio(f"{what} KS", np.array([D]), P.ks_limit(n))
        if D > P.ks_limit(n):
            r.add(f"{what} not distributed as the lobe", [n])
    return r


# ------------------------------------------------------------------ control mutants
def mutant_normals(sc, src, out6, form):
    """The rows a resolve through W2L untransposed ("W2L") or through L2W would write."""
    out = np.array(out6, np.float32)
    w = np.nonzero(valid_records(sc, src))[0]
    s = src[w]
    nm = P.restated_normals(sc.tris, sc.meshdata, s["hits"][:, 0], s["hits"][:, 1], s["hits"][:, 3], form=form)
    out[w, :3], out[w, 3:] = nm.g, nm.us
    return out


def bounce_mutants(c: EnqueueCase, count, rows):
    """name -> (count, rows, the failure that must be reported): numpy edits of a correct enqueue output."""
    sc = scene_of(c)
    m = P.bounce(sc.tris, sc.meshdata, c.src, FAR, c.bounce, c.frames, c.max_bounce, c.frame_pixels)
    assert len(rows) == len(m.idx) == count
    N = m.norm[:, 0]
    us, pos = m.n_side, m.pos   # (the unsmoothed normal ends on the side the ray came from)
    out = {}

    def edit(name, must, **fields):
        x = rows.copy()
        for k, v in fields.items():
            x[k] = v
        out[name] = (count, x, must)

    dd = rows["direction"].astype(np.float64)
    fl = m.flipped[:, None]
    edit("no back-face flip", "direction . norm != last_pdf pi",
         direction=np.where(fl, dd - 2 * (dd * N).sum(1)[:, None] * N, dd),
         origin=np.where(fl, pos - P.OFFSET * us, rows["origin"].astype(np.float64)))
    edit("origin offset along -us", "origin behind the surface", origin=pos - P.OFFSET * us)
    edit("origin offset 1e-3", "origin offset", origin=pos + 1e-3 * us)
    T, B = P.tangent_frame(N)
    om = m.lobe.om
    cu = om[:, 1] ** 2                       # a uniform hemisphere has cos(theta) ~ U(0, 1), as om.y^2 is
    su = np.sqrt(1 - cu * cu) / np.maximum(np.sqrt(1 - om[:, 1] ** 2), 1e-30)
    edit("direction from a uniform hemisphere", "direction . norm != last_pdf pi",
         direction=(om[:, 0] * su)[:, None] * T + cu[:, None] * N + (om[:, 2] * su)[:, None] * B)
    g = np.where(fl, -m.normals.g, m.normals.g)
    Tg, _ = P.tangent_frame(g)
    gr = np.cos(1e-3) * g + np.sin(1e-3) * Tg   # the unquantised normal turned by 1e-3 rad
    T2, B2 = P.tangent_frame(gr)
    edit("direction about the unquantised normal rotated by 1e-3 rad", "direction . norm != last_pdf pi",
         direction=om[:, :1] * T2 + om[:, 1:2] * gr + om[:, 2:] * B2)
    sw = rows.copy()
    i = count // 3
    sw[[i, i + 1]] = sw[[i + 1, i]]
    out["two survivors swapped"] = (count, sw, "source order")
    dr = rows.copy()
    dr[i:-1] = rows[i + 1:]
    out["one survivor dropped with the count unchanged"] = (count, dr, "survivor set")
    edit("hits not copied", "hits not copied", hits=np.zeros_like(rows["hits"]))
    if c.frame_pixels:
        edit("PixelIndex of the frame-local pixel", "PixelIndex kept", PixelIndex=rows["PixelIndex"] % c.frame_pixels)
    return out


def generate_mutants(cam, W, H, frames, max_bounce):
    """name -> (rays, the failure that must be reported); jitter on."""
    c2w, ip = camera_matrices(cam, W, H)
    rowmajor = c2w.copy()
    rowmajor[:3, :3] = c2w[:3, :3].T
    noshift = ip.copy()
    noshift[:2, 3] = 0
    a = (W, H, cam.near, cam.far, 1, frames, max_bounce)
    return {"c2w read row-major": (rays_from_matrices(rowmajor, ip, *a), "direction"),
            "lens-shift terms dropped": (rays_from_matrices(c2w, noshift, *a), "direction"),
            "jitter r in place of r - 0.5": (rays_from_matrices(c2w, ip, *a, centre=0.0), "direction")}
