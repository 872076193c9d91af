"""The heightmap surface as geometry, in numpy and float64: what a terrain march must answer for a ray, derived
from the surface the reference's shaders describe and from nothing else. No call into tthip's host reference
(host/tt_terrain.cpp), the kernels or the oracle is made here; tests/test_terrain_geometry_host.py compares that
host reference with this module and tests/test_gpu_terrain_geometry.py the kernels.

The surface (IntersectionKernels.compute:604-618, CommonData.cginc:922-938): GetDist measures
g * (|y| - 0.01 - h) with h = 2 HeightScale Heightmap.SampleLevel(sampler_trilinear_clamp, uv', 0).x,
uv = min(local xz / TerrainDim, 1) and uv' = uv * (HeightMap.xy - HeightMap.zw) + HeightMap.zw, so in world space
the surface is y = PositionOffset.y + 0.01 + 2 HeightScale B(u', v') with B the D3D bilinear filter with clamp
addressing: texel i has its centre at i + 0.5.

The march is a sphere trace with steps g * gap, g = sin(atan(1/2)) = 1 / sqrt(5) (:511), gap = y - surface. Along
a unit direction the gap changes by at most sqrt(1 + slope^2) per unit length, sqrt(5) at slope 2, so a step
never passes a surface whose slope is below 2 and what the march answers is a geometric fact outside small bands:
it accepts a sample whose gap is below 1e-4 / g = 2.2361e-4 (:657, :550), it starts 1e-4 (:649) or 1e-3 (:531)
past the box entry, it gives up after 2,000 steps. Rays inside those bands are classed ambiguous and asserted
nothing about; max_slope() is what a caller asserts to be below 2 first."""
import numpy as np

G = 1.0 / np.sqrt(5.0)
ACCEPT = 1e-4 / G                                   # 2.2361e-4: the gap below which a sample is accepted
DT = 5e-4                                           # spacing of the gap samples along a ray
BELOW = -2e-4                                       # a sample this far under the surface: the ray is in the ground
SAFE = ACCEPT + 1.5e-4 + 0.5 * DT * np.sqrt(5.0)    # acceptance + margin + the change between two samples, slope < 2
START_BELOW, START_BAND = -3e-4, 4e-4
EDGE = 1e-5
LIMIT_BAND = 2e-3
STEPS_FILTER = 1500                                 # the bound is 2,000 (TT_TERRAIN_MAX_STEPS)
MUST_MISS, MUST_HIT, STARTS_BELOW, AMBIGUOUS = 0, 1, 2, 3
CLEAR, OCCLUDED = 0, 1                              # shadow classes (AMBIGUOUS as above)
_STRIDE = 32                                        # coarse samples are every 32nd sample
_REFINE = SAFE + 1.2 * 0.5 * _STRIDE * DT * np.sqrt(5.0)


# ------------------------------------------------------------------ the surface
def decode_atlas(atlas) -> np.ndarray:
    """binary16 bits (uint16) or float16 [h, w] -> float64."""
    a = np.asarray(atlas)
    return (a.view(np.float16) if a.dtype == np.uint16 else a).astype(np.float64)


def bilinear_clamp(A, au, av, half_texel=0.5):
    """SampleLevel(sampler_*_linear_clamp, (au, av), 0) of the single-channel texture A [h, w] as D3D defines it:
    the sample point in texel units is uv * size - 0.5, the four texels around it are weighted by the fractions and
    their indices clamped to the texture."""
    h, w = A.shape
    x, y = au * w - half_texel, av * h - half_texel
    xf, yf = np.floor(x), np.floor(y)
    wx, wy = x - xf, y - yf
    x0 = np.clip(xf, 0, w - 1).astype(np.intp)
    x1 = np.clip(xf + 1, 0, w - 1).astype(np.intp)
    y0 = np.clip(yf, 0, h - 1).astype(np.intp)
    y1 = np.clip(yf + 1, 0, h - 1).astype(np.intp)
    top = A[y0, x0] + (A[y0, x1] - A[y0, x0]) * wx
    bot = A[y1, x0] + (A[y1, x1] - A[y1, x0]) * wx
    return top + (bot - top) * wy


def surface(T, atlas, x, z):
    """World-space height of terrain T (one TERRAIN_DTYPE record) at world x, z; atlas as decode_atlas gives it."""
    P = np.asarray(T["PositionOffset"], np.float64)
    dim_x, dim_z = (float(v) for v in T["TerrainDim"])
    hm = np.asarray(T["HeightMap"], np.float64)
    u = np.minimum((np.asarray(x, np.float64) - P[0]) / dim_x, 1.0)
    v = np.minimum((np.asarray(z, np.float64) - P[2]) / dim_z, 1.0)
    b = bilinear_clamp(atlas, u * (hm[0] - hm[2]) + hm[2], v * (hm[1] - hm[3]) + hm[3])
    return P[1] + 0.01 + 2.0 * float(T["HeightScale"]) * b


def max_slope(T, atlas, surf=surface, per_texel=8):
    """The largest gradient magnitude of the surface over the footprint. The grid has per_texel points per texel
    and its lines include the texel centres when the rectangle's corners are texel centres; inside one cell of
    the filter the height is bilinear, its x slope constant along x and its z slope along z, so one-sided
    differences between neighbouring grid points are slopes the surface really has, and the magnitude at a
    grid point is taken over the four quadrants around it."""
    h, w = atlas.shape
    hm = np.asarray(T["HeightMap"], np.float64)
    P = np.asarray(T["PositionOffset"], np.float64)
    dim_x, dim_z = (float(v) for v in T["TerrainDim"])
    nx = int(np.ceil(abs(hm[0] - hm[2]) * w * per_texel)) + 1
    nz = int(np.ceil(abs(hm[1] - hm[3]) * h * per_texel)) + 1
    xs, zs = P[0] + np.linspace(0.0, dim_x, nx), P[2] + np.linspace(0.0, dim_z, nz)
    Y = surf(T, atlas, xs[None, :], zs[:, None])
    sx = np.abs(np.diff(Y, axis=1)) / (dim_x / (nx - 1))
    sz = np.abs(np.diff(Y, axis=0)) / (dim_z / (nz - 1))
    mx = np.maximum(np.pad(sx, ((0, 0), (1, 0))), np.pad(sx, ((0, 0), (0, 1))))
    mz = np.maximum(np.pad(sz, ((1, 0), (0, 0))), np.pad(sz, ((0, 1), (0, 0))))
    return float(np.sqrt(mx * mx + mz * mz).max())


def secant_normal(T, atlas, pos, surf=surface):
    """GetHeightmapNormal (CommonData.cginc:931-937): the cross product of the unit secants over +0.25 in x and
    over +0.25 in z; (0, -1, 0) on flat ground."""
    p = np.atleast_2d(np.asarray(pos, np.float64))
    c = surf(T, atlas, p[:, 0], p[:, 2])
    sx = surf(T, atlas, p[:, 0] + 0.25, p[:, 2]) - c
    sz = surf(T, atlas, p[:, 0], p[:, 2] + 0.25) - c
    zero = np.zeros_like(c)
    a = _unit(np.stack([zero + 0.25, sx, zero], 1))
    b = _unit(np.stack([zero, sz, zero + 0.25], 1))
    return _unit(np.cross(a, b))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------ the march interval
def _slab(o, d, mn, mx):
    """rayBoxIntersection (:513-521) without its two clamps: (entry, exit) per ray. min / max ignore a NaN, as
    HLSL's do (0 * inf where an axis-aligned ray starts on a face)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        a, b = (mn - o) * inv, (mx - o) * inv
    lo, hi = np.fmin(a, b), np.fmax(a, b)
    return np.fmax.reduce(lo, axis=1), np.fmin.reduce(hi, axis=1)


def _interval(T, o, d, lim, shrink, shift):
    """(t0, t1, first sample, end of the samples) per ray. The box is P + shrink .. P + (dimX, dimX, dimZ) - shrink
    (its y extent is dimX: the reference's choice), with corners as float32 holds them; t0 = max(entry, 0.025),
    t1 = min(exit, lim). Samples run from t0 + shift while the local position is inside (0, dim) in x and z and
    (0, 1000) in y and while the distance marched is below lim: that distance is measured from the first sample
    (:653 CurDist < bestHit.t, :535 Dist < MaxDist), so the march reaches t0 + lim, not lim."""
    P = np.asarray(T["PositionOffset"], np.float32)
    dim_x, dim_z = (np.float32(v) for v in T["TerrainDim"])
    ext = np.array([dim_x, dim_x, dim_z], np.float32)
    mn = (P + np.float32(shrink)).astype(np.float64)
    mx = ((P + ext) - np.float32(shrink)).astype(np.float64)
    entry, exit_ = _slab(o, d, mn, mx)
    t0, t1 = np.maximum(entry, 0.025), np.minimum(exit_, lim)
    P64 = P.astype(np.float64)
    _, leave = _slab(o, d, P64, P64 + np.array([float(dim_x), 1000.0, float(dim_z)]))
    s0 = t0 + shift
    return t0, t1, s0, np.minimum(leave, s0 + lim)


class _Gap:
    """gap(t) = y - surface along the rays o + d t."""

    def __init__(self, T, atlas, o, d, surf):
        self.T, self.A, self.o, self.d, self.surf = T, atlas, o, d, surf

    def __call__(self, idx, t):
        p = self.o[idx] + self.d[idx] * t[:, None]
        return p[:, 1] - self.surf(self.T, self.A, p[:, 0], p[:, 2])


def _segments(counts):
    """(ray index, sample index within the ray) of sum(counts) samples, ray by ray."""
    ray = np.repeat(np.arange(len(counts)), counts)
    start = np.cumsum(counts) - counts
    return ray, np.arange(len(ray)) - np.repeat(start, counts)


def _scan(gap, rows, s0, end):
    """The gap sampled at s0 + k DT < end for the rays `rows`: per ray the smallest sampled gap, the index of the
    first sample below BELOW and of the first sample at or below zero (-1: none).

    Every sample is accounted for, though not every one is evaluated: every 32nd is, and the 31 between two of
    those only where one of the two lies below SAFE + 1.2 * 16 DT sqrt(5). Under the slope bound the gap changes
    by at most 16 DT sqrt(5) from the nearer of the two, so a sample left out lies above SAFE and is neither the
    minimum that decides a must-miss nor below zero. Nothing after the first coarse sample below BELOW is needed."""
    n = len(rows)
    count = np.maximum(np.ceil((end - s0) / DT).astype(np.int64), 1)
    big = np.iinfo(np.int64).max
    g_min, first_below, first_neg = np.full(n, np.inf), np.full(n, big), np.full(n, big)

    def reduce_into(ray, k, g):
        np.minimum.at(g_min, ray, g)
        np.minimum.at(first_below, ray, np.where(g < BELOW, k, big))
        np.minimum.at(first_neg, ray, np.where(g <= 0.0, k, big))

    nc = (count - 1) // _STRIDE + 2                     # k = 0, 32, 64, ... and the last sample
    ray, j = _segments(nc)
    k = np.minimum(j * _STRIDE, count[ray] - 1)
    g = gap(rows[ray], s0[ray] + k * DT)
    reduce_into(ray, k, g)
    stop = first_below.copy()                           # the first coarse sample in the ground, if any
    # blocks [k_j, k_j+1] to refine: an end below _REFINE, and the block not after `stop`
    nxt = np.r_[ray[1:] == ray[:-1], False]
    lo_k, hi_k = k[nxt], k[np.r_[False, nxt[:-1]]]
    near = np.minimum(g[nxt], g[np.r_[False, nxt[:-1]]]) < _REFINE
    near &= (lo_k < stop[ray[nxt]]) & (hi_k - lo_k > 1)
    b_ray, b_lo, b_n = ray[nxt][near], lo_k[near] + 1, (hi_k - lo_k - 1)[near]
    for c0 in range(0, len(b_ray), 4096):               # in chunks: a few million samples at a time
        sl = slice(c0, c0 + 4096)
        seg, off = _segments(b_n[sl])
        r, kk = b_ray[sl][seg], b_lo[sl][seg] + off
        reduce_into(r, kk, gap(rows[r], s0[r] + kk * DT))
    return g_min, np.where(first_below == big, -1, first_below), np.where(first_neg == big, -1, first_neg)


def _bisect(gap, rows, lo, hi):
    """The zero of the gap between lo (gap > 0) and hi (gap <= 0)."""
    for _ in range(48):
        mid = 0.5 * (lo + hi)
        above = gap(rows, mid) > 0.0
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    return 0.5 * (lo + hi)


def _trace_steps(gap, rows, s0, end, cap=STEPS_FILTER):
    """Steps a float64 sphere trace takes from s0 until it accepts a sample or passes `end`, capped. A conditioning
    filter only: it never supplies an answer."""
    steps = np.zeros(len(rows), np.int64)
    t = s0.copy()
    live = np.arange(len(rows))
    for _ in range(cap):
        if not len(live):
            break
        g = gap(rows[live], t[live])
        steps[live] += 1
        go = (g >= ACCEPT)
        t[live] = t[live] + G * np.maximum(g, 0.0)
        live = live[go & (t[live] < end[live])]
    return steps


# ------------------------------------------------------------------ classification
def _rays64(o, d):
    return np.atleast_2d(np.asarray(o, np.float32)).astype(np.float64), \
        np.atleast_2d(np.asarray(d, np.float32)).astype(np.float64)


def classify_closest(T, atlas, o, d, lim, surf=surface):
    """What tt_trace_heightmap must do with each ray on terrain T, whose record holds t = lim on arrival (the far
    plane for a miss): (class, t0, t_cross), class one of MUST_MISS (the record stays), MUST_HIT (a terrain record;
    t_cross is the float64 first crossing), STARTS_BELOW (a terrain record with t = t0) and AMBIGUOUS. The first
    class that applies wins; the ambiguity tests come after the others."""
    o, d = _rays64(o, d)
    n = len(o)
    lim = np.broadcast_to(np.asarray(lim, np.float64), (n,)).copy()
    t0, t1, s0, end = _interval(T, o, d, lim, 0.001, 1e-4)
    cls = np.full(n, MUST_MISS)
    t_cross = np.full(n, np.nan)
    gap = _Gap(T, atlas, o, d, surf)
    rows = np.nonzero(t0 <= t1)[0]                      # the others fail the box test (:646): no march
    if len(rows):
        g0 = gap(rows, s0[rows])
        below = g0 < START_BELOW
        cls[rows[below]] = STARTS_BELOW
        m = rows[~below]
        g_min, k_below, k_neg = _scan(gap, m, s0[m], end[m])
        hit = k_below >= 0
        cls[m[hit]] = MUST_HIT
        cls[m[~hit & ~(g_min > SAFE)]] = AMBIGUOUS      # grazing: neither in the ground nor safely above it
        cls[rows[~below][(g0[~below] <= START_BAND)]] = AMBIGUOUS
        h = m[hit]
        sure = h[k_neg[hit] >= 1]                       # (k = 0 at or below zero is in the start band: ambiguous)
        if len(sure):
            k = k_neg[hit][k_neg[hit] >= 1]
            t_cross[sure] = _bisect(gap, sure, s0[sure] + (k - 1) * DT, s0[sure] + k * DT)
            slow = _trace_steps(gap, sure, s0[sure], t_cross[sure] + 1e-3) >= STEPS_FILTER
            cls[sure[slow]] = AMBIGUOUS
        # the limit: the crossing within LIMIT_BAND of where the march stops
        near_lim = (cls == MUST_HIT) & (np.abs((t_cross - t0) - lim) < LIMIT_BAND)
        cls[near_lim] = AMBIGUOUS
    cls[np.abs(t0 - t1) < EDGE] = AMBIGUOUS             # the box edge
    return cls, t0, t_cross


def classify_shadow(terrains, atlas, o, d, t, surf=surface):
    """What tt_trace_shadow_heightmap must find for each NEE ray: CLEAR, OCCLUDED or AMBIGUOUS; a ray with t == 0
    is not marched (:570) and comes back CLEAR. Against the closest-hit form (:525-556): the box is not shrunk, the
    first sample lies 1e-3 past t0, the limit is |t|. The reference takes the terrains in order and stops at the
    first that occludes; for the answer the order does not matter: a ray is OCCLUDED when it is on any terrain,
    otherwise AMBIGUOUS when it is on any.

    The loop of :535 tests `> 0` on the previous sample, so one sample may lie past the faces at 0; the step to it
    is at most g * gap, which under the slope bound ends no further than g * (the gap at the exit) past the exit.
    A CLEAR ray is safe over that stretch too (the surface formula continues past the footprint)."""
    o, d = _rays64(o, d)
    n = len(o)
    reach = np.abs(np.asarray(t, np.float64))
    out = np.full(n, CLEAR)
    any_occ, any_amb = np.zeros(n, bool), np.zeros(n, bool)
    for T in terrains:
        t0, t1, s0, end = _interval(T, o, d, reach, 0.0, 1e-3)
        gap = _Gap(T, atlas, o, d, surf)
        marched = (reach != 0) & (t0 <= t1)
        any_amb |= (reach != 0) & (np.abs(t0 - t1) < EDGE)
        rows = np.nonzero(marched & (end > s0))[0]
        any_amb |= marched & ~(end > s0) & (end > s0 - LIMIT_BAND)
        if not len(rows):
            continue
        at_exit = np.maximum(gap(rows, end[rows]), 0.0)
        lag = np.where(end[rows] < s0[rows] + reach[rows], G * at_exit + 1e-3, 0.0)
        g_min, k_below, _ = _scan(gap, rows, s0[rows], end[rows] + lag)
        in_ground = (k_below >= 0) & (s0[rows] + k_below * DT < end[rows] - LIMIT_BAND)
        slow = np.zeros(len(rows), bool)
        if in_ground.any():
            r = rows[in_ground]
            slow[in_ground] = _trace_steps(gap, r, s0[r], s0[r] + k_below[in_ground] * DT) >= STEPS_FILTER
        occ = in_ground & ~slow
        any_occ[rows[occ]] = True
        any_amb[rows[~occ & ~(g_min > SAFE)]] = True
    out[any_amb] = AMBIGUOUS
    out[any_occ] = OCCLUDED
    return out
