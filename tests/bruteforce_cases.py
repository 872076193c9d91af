"""Scenes, ray sets and comparisons of the brute-force matrix (test infrastructure), shared by
test_oracle_bruteforce.py (the oracle against bruteforce.py) and test_gpu_bruteforce.py (the kernels
against bruteforce.py). Nothing here calls the oracle or the engine: a test hands in what its side wrote.

Caps of every case, conditions on the case and not measurements of the code under test: at most 5 % of the
rays may be unrobust, and at least 100 robust hits (occluded rays) and 15 robust misses (visible rays) must
remain. A case that misses a cap gets another seed or ray box, never another cap.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import bruteforce as BF
import tthip

FAR = 1000.0
MAX_UNROBUST = 0.05
MIN_HITS, MIN_MISSES = 100, 15
FLAGS = (0, tthip.TT_TRACE_IGNORE_GLASS, tthip.TT_TRACE_IGNORE_BACKFACING,
         tthip.TT_TRACE_IGNORE_GLASS | tthip.TT_TRACE_IGNORE_BACKFACING)
N_MAT = 8
SCENES = ("soup", "instances", "cornell", "ground")
LEAF_SCENES = ("soup", "cornell", "ground")


# ------------------------------------------------------------------ materials and scenes
def closest_materials():
    """Two glass and two Invisible materials among eight."""
    m = np.zeros(N_MAT, tthip.MAT_DTYPE)
    m["specTrans"][[1, 2]] = 1.0
    m["Tag"][[3, 4]] = 1 << tthip.FLAG_INVISIBLE
    return m


def glass_materials():
    """Two glass materials and no Invisible one: a scene whose bounce-0 launches need no material check."""
    m = closest_materials()
    m["Tag"] = 0
    return m


def shadow_materials():
    """One untextured glass, one ShadowCaster and one IsBackground material among eight."""
    m = np.zeros(N_MAT, tthip.MAT_DTYPE)
    m["specTrans"][1] = 1.0
    m["surfaceColor"][1] = (0.9, 0.8, 0.7)
    m["AlbedoTex"][1] = (0, 0)
    m["Tag"][5] = 1 << tthip.TT_FLAG_SHADOW_CASTER
    m["Tag"][6] = 1 << tthip.TT_FLAG_IS_BACKGROUND
    return m


def instanced_scene(moved=False):
    """One parent and twelve instances of three props (thirteen mesh records). moved: six of the twelve
    instances at another place, the same BLASes and the same order of records."""
    rng = np.random.default_rng(11)
    am = tthip.AssetManager()
    mats = closest_materials()
    am.add_parent(tthip.Blas(tthip.Mesh.soup(5, 800, 6.0, 0.6)), tthip.trs_matrix((0, 0, 0)), mats)
    props = [am.add_instance_parent(tthip.Blas(tthip.Mesh.prop(100 + k, int(rng.integers(60, 400)))), mats)
             for k in range(3)]
    shift = np.random.default_rng(12).uniform(-2.0, 2.0, (12, 3)) * [1, 0.3, 1]
    for i in range(12):
        pos = rng.uniform(-8, 8, 3) * [1, 0.2, 1]
        if moved and i % 2 == 0:
            pos = pos + shift[i]
        am.add_instance(props[i % 3], tthip.trs_matrix(pos, float(rng.uniform(0, 360)), float(rng.uniform(0.4, 1.5))))
    return am.build()


@functools.lru_cache(maxsize=None)
def _base_scene(name):
    if name == "soup":
        sc = tthip.single_object_scene(tthip.Mesh.soup(1, 3000, 2.0, 0.2), n_materials=N_MAT)
    elif name == "cornell":
        sc = tthip.single_object_scene(tthip.Mesh.cornell(), n_materials=N_MAT)
    elif name == "ground":
        sc = tthip.single_object_scene(tthip.Mesh.ground(-4, 4, -4, 4, 16, 16), n_materials=N_MAT)
    else:
        sc = instanced_scene()
    paint_materials(sc)
    return sc


def paint_materials(sc, seed=5):
    """MatDat drawn from 0..8 per triangle: the eight materials, and one index past the table of the last
    mesh record (it reads a zero material). About 30 % of the triangles get a material that one of the filters
    acts on under either table."""
    p = [0.2, 0.08, 0.07, 0.08, 0.07, 0.1, 0.1, 0.2, 0.1]
    sc.tris["MatDat"] = np.random.default_rng(seed).choice(N_MAT + 1, len(sc.tris), p=p)


@functools.lru_cache(maxsize=None)
def scene(name, kind="closest"):
    """kind 'closest', 'glass' or 'shadow': the same geometry under one of the material tables. Shared between
    tests: do not write to it."""
    sc = _base_scene(name)
    table = {"closest": closest_materials, "glass": glass_materials, "shadow": shadow_materials}[kind]()
    mats = np.concatenate([table] * (len(sc.materials) // N_MAT))
    atlas = np.ones((1, 1, 4), np.float16) if kind == "shadow" else None
    return dataclasses.replace(sc, materials=mats, texture_atlas=atlas)


@functools.lru_cache(maxsize=None)
def geometry(name, kind="closest"):
    return BF.Geometry.from_scene(scene(name, kind))


# ------------------------------------------------------------------ ray sets
def _box(g, grow):
    lo, hi = g.bounds()
    pad = grow * (hi - lo).max()
    return lo - pad, hi + pad


def surface_points(g, rng, n):
    """n world-space points, each uniform on a triangle drawn uniformly from all instance triangles."""
    counts = np.array([hi - lo for lo, hi in g.ranges])
    m = rng.choice(len(counts), n, p=counts / counts.sum())
    tri = np.array([lo for lo, _ in g.ranges])[m] + (rng.random(n) * counts[m]).astype(np.int64)
    a, b = rng.random(n), rng.random(n)
    a, b = np.where(a + b > 1, 1 - a, a), np.where(a + b > 1, 1 - b, b)
    obj = g.p0[tri] + a[:, None] * g.e1[tri] + b[:, None] * g.e2[tri]
    l2w = np.linalg.inv(g.w2l)[m]
    return np.einsum("nij,nj->ni", l2w[:, :3, :3], obj) + l2w[:, :3, 3]


def random_rays(g, seed, n, grow=0.25, reach=2.0):
    """Random origins and unit directions. The first half of the origins is uniform in the bounds grown by
    `grow` of the largest extent; the second half lies U(0, reach) behind a random point of the surface, against
    the ray's direction, so that sparse scenes are hit often enough for the caps whatever the launch flags."""
    rng = np.random.default_rng(seed)
    lo, hi = _box(g, grow)
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = n // 2
    o[k:] = surface_points(g, rng, n - k) - d[k:] * rng.uniform(0.0, reach, (n - k, 1))
    return o.astype(np.float32), d.astype(np.float32)


def axis_rays(g, seed, n, grow=0.1):
    """One component +-1, the other two +0 or -0; the origin outside the bounds on that axis by U(0.5, 2). On
    the other two axes the first half is uniform over the bounds grown a little (some rays pass beside the
    geometry), the second half takes the coordinates of a random point of the surface, moved by up to 0.05 (and at most a
    quarter of the bounds' extent on that axis) so that the ray does not lie in the plane of an upright wall it was
    drawn from."""
    rng = np.random.default_rng(seed)
    lo, hi = g.bounds()
    blo, bhi = _box(g, grow)
    o = rng.uniform(blo, bhi, (n, 3))
    k = n // 2
    o[k:] = surface_points(g, rng, n - k) + rng.uniform(-1.0, 1.0, (n - k, 3)) * np.minimum(0.05, (hi - lo) / 4)
    d = np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0)
    axis = rng.integers(0, 3, n)
    sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    ar = np.arange(n)
    d[ar, axis] = sign
    off = rng.uniform(0.5, 2.0, n)
    o[ar, axis] = np.where(sign > 0, lo[axis] - off, hi[axis] + off)
    return o.astype(np.float32), d.astype(np.float32)


def axis_shadow_buffer(g, o, d, seed):
    """Shadow rays over axis_rays: |t| is U(0.05, 1.2) of the way from the origin to the far side of the bounds
    (some rays end in front of the geometry, some inside it, some behind it), 75 % positive."""
    rng = np.random.default_rng(seed)
    lo, hi = g.bounds()
    far_side = np.where(d > 0, hi[None, :], lo[None, :])
    across = np.abs(np.where(np.abs(d) == 1, far_side - o, 0.0)).max(1)
    r = shadow_buffer(o, d, seed)
    r["t"] = across * rng.uniform(0.05, 1.2, len(o)) * np.where(rng.random(len(o)) < 0.75, 1.0, -1.0)
    return r


def ray_buffer(o, d):
    """RayData ping-pong buffer of 2 n with the n rays in both halves (bounce 1 reads the second), one ray per
    pixel of an n x 1 frame."""
    n = len(o)
    r = np.zeros(2 * n, tthip.RAY_DTYPE)
    for h in (slice(0, n), slice(n, 2 * n)):
        r["origin"][h], r["direction"][h], r["PixelIndex"][h] = o, d, np.arange(n)
    return r


def shadow_buffer(o, d, seed):
    """ShadowRayData with t = +-U(0.05, 3), 75 % positive, random illumination, one ray per pixel."""
    rng = np.random.default_rng(seed)
    n = len(o)
    r = np.zeros(n, tthip.SHADOW_DTYPE)
    r["origin"], r["direction"] = o, d
    r["t"] = rng.uniform(0.05, 3.0, n) * np.where(rng.random(n) < 0.75, 1.0, -1.0)
    r["illumination"] = rng.random((n, 3))
    r["PixelIndex"] = np.arange(n)
    return r


NEE_W, NEE_H = 40, 24


def nee_camera(g):
    """A camera in front of the scene's bounds looking at their centre, and a light above them."""
    lo, hi = g.bounds()
    c, ext = (lo + hi) / 2, (hi - lo).max()
    eye = c + np.array([0.1, 0.3, 0.7]) * ext
    light = c + np.array([0.3, 0.3, 0.2]) * ext
    c2w, ip = tthip.unity_camera(tuple(eye), tuple(c - eye), (0, 1, 0), 60.0, NEE_W, NEE_H, 0.05, FAR)
    return c2w, ip, light


def nee_shadow_rays(traced, light, seed, limit=600):
    """handbuilt.nee_rays_from_hits of a traced NEE_W x NEE_H frame, at most `limit` of them."""
    import handbuilt as hb

    sr = hb.nee_rays_from_hits(traced, NEE_W * NEE_H, light, seed, FAR)
    if len(sr) > limit:
        sr = sr[np.sort(np.random.default_rng(seed).choice(len(sr), limit, replace=False))].copy()
    return sr


# ------------------------------------------------------------------ closest-hit comparison
@dataclasses.dataclass
class Report:
    mismatches: int
    failures: list
    text: str
    tint: tuple = None  # compare_any_hit with a tint model: (largest row ratio, largest Direct ratio, rays resolved with O)

    def check(self):
        print(self.text)
        assert not self.failures, "; ".join(self.failures) + " | " + self.text


def _caps(robust, positive, what_pos, what_neg, caps):
    n = len(robust)
    fails = []
    unrobust = int((~robust).sum())
    n_pos, n_neg = int((robust & positive).sum()), int((robust & ~positive).sum())
    if caps:
        if unrobust > MAX_UNROBUST * n:
            fails.append(f"{unrobust} of {n} rays unrobust (cap {MAX_UNROBUST:.0%})")
        if n_pos < MIN_HITS:
            fails.append(f"only {n_pos} robust {what_pos} (cap {MIN_HITS})")
        if n_neg < MIN_MISSES:
            fails.append(f"only {n_neg} robust {what_neg} (cap {MIN_MISSES})")
    text = f"robust share {1 - unrobust / max(n, 1):.4f}, robust {what_pos} {n_pos}, robust {what_neg} {n_neg}"
    return fails, text


def compare_closest(ref: BF.Closest, hits, caps=True) -> Report:
    """Hit records (n x 4 uint32, as a trace left them) against the reference.
    Robust rays: a miss carries the miss record (hits[1] == 0xFFFFFFFF), a hit the reference's (mesh,
    triangle). Every hit on the reference's triangle, robust or not: |t32 - t64| <= K 2^-24 cond_t |t64| and
    each 16-bit uv code c has |c / 65535 - u64| <= 1 / 65535 + K 2^-24 cond_u (K = bruteforce.K_ROUNDINGS)."""
    hits = np.ascontiguousarray(hits)
    missed = hits[:, 1] == 0xFFFFFFFF
    on_tri = ref.hit & ~missed & (hits[:, 0].astype(np.int64) == ref.mesh) & (hits[:, 1].astype(np.int64) == ref.tri)
    same = np.where(ref.hit, on_tri, missed)
    bad = np.nonzero(ref.robust & ~same)[0]
    fails, text = _caps(ref.robust, ref.hit, "hits", "misses", caps)
    if len(bad):
        i = int(bad[0])
        fails.append(f"{len(bad)} robust rays differ, first ray {i}: reference "
                     + (f"(mesh {ref.mesh[i]}, triangle {ref.tri[i]}, t {ref.t[i]:.9g}, u {ref.u[i]:.6g}, v {ref.v[i]:.6g})"
                        if ref.hit[i] else "a miss")
                     + f", record {[hex(int(x)) for x in hits[i]]} (t {hits[i, 2:3].view(np.float32)[0]:.9g})")
    k = BF.K_ROUNDINGS * BF.U24
    t32 = hits[:, 2].copy().view(np.float32).astype(np.float64)
    cu, cv = (hits[:, 3] & 0xFFFF) / 65535.0, (hits[:, 3] >> 16) / 65535.0
    w = np.nonzero(on_tri)[0]
    rt = np.abs(t32[w] - ref.t[w]) / (k * ref.cond_t[w] * np.abs(ref.t[w]))
    ru = np.abs(cu[w] - ref.u[w]) / (1 / 65535.0 + k * ref.cond_u[w])
    rv = np.abs(cv[w] - ref.v[w]) / (1 / 65535.0 + k * ref.cond_v[w])
    t_max = float(rt.max()) if len(w) else 0.0
    uv_max = float(max(ru.max(), rv.max())) if len(w) else 0.0
    if t_max > 1:
        i = int(w[np.argmax(rt)])
        fails.append(f"t of ray {i} off by {t_max:.3g} of its bound (t32 {t32[i]:.9g}, t64 {ref.t[i]:.9g}, cond_t "
                     f"{ref.cond_t[i]:.3g})")
    if uv_max > 1:
        fails.append(f"a uv code off by {uv_max:.3g} of its bound")
    text += f", largest t ratio {t_max:.3g}, largest uv ratio {uv_max:.3g} over {len(w)} hits"
    return Report(len(bad), fails, text)


def reference_closest(g, rays, n, flags, bounce, **kw):
    return BF.closest(g, rays["origin"][:n], rays["direction"][:n], FAR, flags, bounce, **kw)


# ------------------------------------------------------------------ any-hit comparison
DIRECT0, NEE0, VIS0 = 0.5, 9.0, 7.0


def shadow_outputs(n, n_pixels):
    """(visibility, GlobalColors, NEEPosA) as a shadow call takes them, filled with the marker values that
    compare_any_hit knows as untouched."""
    vis = np.full((n, 4), VIS0, np.float32)
    col = np.zeros(n_pixels, tthip.COL_DTYPE)
    col["Direct"] = DIRECT0
    nee = np.full((n_pixels, 4), NEE0, np.float32)
    return vis, col, nee


def reference_any_hit(g, srays, visibility_check=False, **kw):
    return BF.any_hit(g, srays["origin"], srays["direction"], srays["t"], visibility_check, **kw)


def compare_any_hit(ref: BF.AnyHit, before, after, vis, col, nee, bounce, visibility_check=False, status=None,
                    caps=True, tint=None, tint_check=None) -> Report:
    """What an any-hit call left (`after`: the rays in place, vis / col / nee from shadow_outputs) against the
    reference, on robust rays; `before` are the rays as handed in, one per pixel. status: the oracle's
    counts.status, or None.

    Default mode: an occluded ray has t == 0 and a zero visibility row, a visible one keeps its t bitwise and
    has visibility.w == 1; the row is exactly (1, 1, 1, 1) where no glass triangle can have tinted (tint values
    themselves are not checked). At bounce 0, Direct[pixel] == float32(0.5 + illumination) for visible rays
    with t >= 0 and an all-ones row (one correctly rounded add), and stays untouched for occluded and negative-t
    rays. NEEPosA[pixel] = (o + d |t|, 0) for visible rays at bounce 0 to within 4 * 2^-24 * M, M the largest
    coordinate magnitude of the segment's end points o and p: fl(o + fl(d |t|)) is off by at most
    2^-24 (|d |t|| + |p|) <= 2^-24 (|o| + 2 |p|) <= 3 * 2^-24 * M per component, plus one for slack; it stays
    untouched for occluded rays and at bounce 1.
    Visibility-check mode: rows are (1, 1, 1, 1) or (0, 0, 0, 0) and nothing else is written.

    tint, tint_check (a materials.Tint and materials.tint_check, handed in by the caller; the default mode only):
    the visibility rows of robustly visible rays must also satisfy the subset rule of tint_check, and at bounce 0 the Direct of a visible ray with t >= 0 whose
    row is not all ones lies within two roundings (the product and the sum, all terms positive) of 0.5 +
    illumination * row, row the float32 row that was written: |Direct - x| <= 2 * 2^-24 * x. The report's
    `tint` holds (largest row ratio, largest Direct ratio, rays with O non-empty the rule resolves)."""
    n = len(before)
    r = ref.robust
    pix = before["PixelIndex"].astype(np.int64)
    zero_row, one_row = (vis == 0).all(1), (vis == 1).all(1)
    t_in, t_out = before["t"], after["t"]
    fails, text = _caps(r, ref.occluded, "occluded", "visible", caps)
    occ, see = r & ref.occluded, r & ~ref.occluded
    extra = None

    def need(cond, where, what):
        bad = np.nonzero(where & ~cond)[0]
        if len(bad):
            fails.append(f"{len(bad)} rays: {what}, first ray {int(bad[0])}")
        return len(bad)

    if visibility_check:
        mism = need(zero_row, occ, "occluded but the visibility row is not zero")
        mism += need(one_row, see, "visible but the visibility row is not ones")
        raw = [np.ascontiguousarray(x).view(np.uint8).reshape(n, -1) for x in (before, after)]
        need((raw[0] == raw[1]).all(1), np.ones(n, bool), "the visibility check wrote to a ray")
        if not ((col["Direct"] == np.float32(DIRECT0)).all() and (nee == np.float32(NEE0)).all()):
            fails.append("the visibility check wrote GlobalColors or NEEPosA")
    else:
        mism = need(zero_row & (t_out == 0), occ, "occluded but t != 0 or the visibility row is not zero")
        mism += need((t_out.view(np.uint32) == t_in.view(np.uint32)) & (vis[:, 3] == 1), see,
                     "visible but t changed or visibility.w != 1")
        need(one_row, see & ref.glass_clear, "visible past no glass but the visibility row is not ones")
        direct, il = col["Direct"][pix], before["illumination"]
        lit = see & (t_in >= 0) & one_row if bounce == 0 else np.zeros(n, bool)
        need((direct == (np.float32(DIRECT0) + il)).all(1), lit, "Direct != float32(0.5 + illumination)")
        need((direct == np.float32(DIRECT0)).all(1), occ | (r & (t_in < 0)) if bounce == 0 else np.ones(n, bool),
             "Direct was written")
        o, d = before["origin"].astype(np.float64), before["direction"].astype(np.float64)
        p = o + d * np.abs(t_in.astype(np.float64))[:, None]
        scale = np.maximum(np.abs(o).max(1), np.abs(p).max(1))
        got = nee[pix].astype(np.float64)
        if bounce == 0:
            need((np.abs(got[:, :3] - p).max(1) <= 4 * BF.U24 * scale) & (got[:, 3] == 0), see, "NEEPosA is off")
            need((got == NEE0).all(1), occ, "NEEPosA of an occluded ray was written")
        else:
            need((got == NEE0).all(1), np.ones(n, bool), "NEEPosA was written at bounce 1")
        if tint is not None:
            bad, row_ratio, resolved, _ = tint_check(tint, vis[:, :3], see)
            mism += len(bad)
            if bad:
                fails.append(f"{len(bad)} robust visible rays: the visibility row is no product of the tints the ray "
                             f"must and may cross, first ray {bad[0]} (row {vis[bad[0], :3]}, |R| {tint.r_n[bad[0]]}, "
                             f"|O| {len(tint.o_tints[bad[0]])})")
            x = DIRECT0 + il.astype(np.float64) * vis[:, :3].astype(np.float64)
            tinted = see & (t_in >= 0) & ~one_row if bounce == 0 else np.zeros(n, bool)
            dr = (np.abs(direct.astype(np.float64) - x) / (2 * BF.U24 * x)).max(1)
            direct_ratio = float(dr[tinted].max()) if tinted.any() else 0.0
            mism += need(dr <= 1, tinted, "Direct is not within two roundings of 0.5 + illumination * row")
            extra = (row_ratio, direct_ratio, resolved)
            text += (f", largest tint ratio {row_ratio:.3g}, largest Direct ratio {direct_ratio:.3g} over "
                     f"{int(tinted.sum())} tinted rays, {resolved} rays resolved with O non-empty")
    if status is not None:
        mism += need(status == 4, occ, "occluded but counts.status != 4")
        mism += need(status == 0, see, "visible but counts.status != 0")
    text += f", {int((see & ~ref.glass_clear).sum())} visible rays may cross glass"
    return Report(mism, fails, text, extra)


# ------------------------------------------------------------------ refits
def head(ref, k):
    """The first k rays of a reference result."""
    return type(ref)(*[getattr(ref, f.name)[:k] for f in dataclasses.fields(ref)])


@functools.lru_cache(maxsize=None)
def refit_soup():
    """(scene, positions, indices, leaf order) of the soup as one parent whose mesh and BLAS are at hand."""
    mesh = tthip.Mesh.soup(1, 3000, 2.0, 0.2)
    blas = tthip.Blas(mesh)
    am = tthip.AssetManager()
    am.add_parent(blas, None, closest_materials())
    sc = am.build()
    paint_materials(sc)
    pos, _, idx = mesh.arrays()
    return sc, pos, idx, blas.leaf_order()


def deformed_vertices(pos):
    """The vertices under a smooth displacement of at most 0.1, as the float32 array a refit is handed."""
    p = pos.astype(np.float64)
    k = 0.1 / np.sqrt(3.0)
    disp = np.stack([np.sin(1.3 * p[:, 1] + 0.2), np.sin(1.1 * p[:, 2] + 1.0), np.sin(0.9 * p[:, 0] + 2.0)], 1) * k
    return (p + disp).astype(np.float32)


def vertex_buffer(pos):
    """Interleaved position + normal vertex buffer (the normals play no part in tracing)."""
    v = np.zeros((len(pos), 6), np.float32)
    v[:, 0:3] = pos
    v[:, 4] = 1.0
    return v


def deformed_geometry(sc, mesh_index, vertices, indices, leaf):
    """The scene's geometry with mesh record mesh_index rebuilt in float64 from a vertex array, as RefitMesh
    lays a triangle out: pos0 = v[i0], posedge1 = v[i2] - v[i0], posedge2 = v[i1] - v[i0], at its leaf position."""
    v = np.asarray(vertices, np.float64)
    i = np.asarray(indices).reshape(-1, 3)
    at = int(sc.meshdata["TriOffset"][mesh_index]) + np.asarray(leaf, np.int64)
    p0, e1, e2 = (sc.tris[f].astype(np.float64) for f in ("pos0", "posedge1", "posedge2"))
    p0[at], e1[at], e2[at] = v[i[:, 0]], v[i[:, 2]] - v[i[:, 0]], v[i[:, 1]] - v[i[:, 0]]
    return BF.Geometry.from_scene(sc, p0, e1, e2)


def world_boxes(g):
    """Per mesh record {BBMax, BBMin} of its triangles in world space, computed in float64 and rounded outward
    to float32 (the input of a TLAS refit)."""
    out = np.zeros((len(g.ranges), 6), np.float32)
    for m in range(len(g.ranges)):
        w = g.world_corners(m)
        hi, lo = w.max(0), w.min(0)
        h32, l32 = hi.astype(np.float32), lo.astype(np.float32)
        out[m, :3] = np.where(h32 < hi, np.nextafter(h32, np.float32(np.inf)), h32)
        out[m, 3:] = np.where(l32 > lo, np.nextafter(l32, np.float32(-np.inf)), l32)
    return out


@functools.lru_cache(maxsize=None)
def moved_instances():
    """(scene as uploaded, mesh records after six instances moved, geometry after the move, boxes after it)."""
    a = dataclasses.replace(scene("instances"))
    b = instanced_scene(moved=True)
    assert np.array_equal(a.meshdata["TriOffset"], b.meshdata["TriOffset"])
    assert np.array_equal(a.meshdata["NodeOffset"], b.meshdata["NodeOffset"])
    assert (a.meshdata["W2L"] != b.meshdata["W2L"]).any(1).sum() == 6
    g = BF.Geometry.from_scene(a, meshdata=b.meshdata)
    return a, b.meshdata, g, world_boxes(g)
