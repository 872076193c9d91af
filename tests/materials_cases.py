"""Scenes, atlases, ray sets, comparisons and controls of the texture-space pin (test infrastructure), shared
by test_materials_host.py (the oracle against materials.py) and test_gpu_materials.py (the kernels against
materials.py). Nothing here calls the oracle or the engine: a test hands in what its side wrote.

Caps of every case, conditions on the case and not measurements of the code under test: the geometric caps of
bruteforce_cases (at most 5 % unrobust rays, at least 100 robust positives and 15 robust negatives), and the
material margins may make at most 2 % of a case's rays unrobust that would be robust without them. A case that
misses a cap gets another input, never another cap. COVERAGE holds the floors a scene family's cases must reach
together, counted on the model's classes.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import bruteforce as BF
import bruteforce_cases as C
import materials as M
import producers_cases as PC
import tthip

FAR = C.FAR
N_RAYS = 600
N_BIG = 4096
MAX_MATERIAL_MARGINAL = 0.02
ALPHA_W, ALPHA_H = 64, 32
TEX_W, TEX_H = 40, 24
ATLASES = ("noise", "checker", "ramps", "marker")
AFFINE = ("parts", "soup")
FAMILIES = {"affine": AFFINE, "random": ("rsoup",)}
COVERAGE = {"cutout hits": 100, "alpha-rejected first": 100, "visible by rejection": 50, "tinted": 100,
            "tinted twice": 30, "resolved with O": 20, "each kind": 20}
EQUAL = np.float32(128) / np.float32(255)


# ------------------------------------------------------------------ atlases
@functools.lru_cache(maxsize=None)
def alpha_atlas(kind):
    """uint8 [32, 64]. noise; a 0 / 255 checkerboard of 4-texel squares; a horizontal ramp in the left half and
    a vertical one in the right; a marker: 128 everywhere except distinct values in the four corners and along row
    0 and column 0, and a block of 127 (rows 18..27, columns 44..59) for the materials whose cutoff is 128 / 255."""
    y, x = np.mgrid[0:ALPHA_H, 0:ALPHA_W]
    if kind == "noise":
        # white noise under two 3 x 3 box blurs, stretched back over 0 .. 255: neighbouring texels differ by about
        # a tenth of the range, which keeps the linear sampler's margin (its slope times the UV's uncertainty) small
        a = np.random.default_rng(71).uniform(0.0, 1.0, (ALPHA_H, ALPHA_W))
        for _ in range(2):
            a = sum(np.roll(np.roll(a, i, 0), j, 1) for i in (-1, 0, 1) for j in (-1, 0, 1)) / 9.0
        a = np.clip(np.rint(127.5 + (a - a.mean()) / a.std() * 60.0), 0, 255)
    elif kind == "checker":
        a = 255 * (((x // 4) + (y // 4)) % 2)
    elif kind == "ramps":
        a = np.where(x < ALPHA_W // 2, x * 255 // (ALPHA_W // 2 - 1), y * 255 // (ALPHA_H - 1))
    else:
        a = np.full((ALPHA_H, ALPHA_W), 128)
        a[0, :] = 1 + np.arange(ALPHA_W)
        a[:, 0] = 200 + np.arange(ALPHA_H)
        a[0, 0], a[0, -1], a[-1, 0], a[-1, -1] = 10, 20, 30, 40
        a[18:28, 44:60] = 127
    return np.ascontiguousarray(a, np.uint8)


@functools.lru_cache(maxsize=None)
def texture_atlas():
    """float16 [24, 40, 4], texels in (0, 4)."""
    return np.random.default_rng(72).uniform(0.0, 4.0, (TEX_H, TEX_W, 4)).astype(np.float16)


# ------------------------------------------------------------------ materials
def _pack(x, y):
    return int(x) | (int(y) << 15)


def _rect(lo, hi, w, h):
    """[TexDim2.x, TexDim2.y] of the rectangle whose corner at wrapped uv = 0 is texel `lo` and at 1 texel `hi`
    (AlignUV: .x packs the corner at 1, .y the corner at 0)."""
    return [_pack(hi[0] * 16384 // w, hi[1] * 16384 // h), _pack(lo[0] * 16384 // w, lo[1] * 16384 // h)]


# alpha rectangles, in texels of the 64 x 32 atlas
RECTS = {
    "interior": _rect((10, 6), (40, 22), ALPHA_W, ALPHA_H),           # corners low to high
    "interior reversed": _rect((40, 22), (10, 6), ALPHA_W, ALPHA_H),  # corners high to low
    "low edges": _rect((0, 0), (24, 12), ALPHA_W, ALPHA_H),           # touches column 0 and row 0
    "high edges": _rect((64, 32), (36, 14), ALPHA_W, ALPHA_H),        # touches the last column and row, reversed
    "one texel": _rect((20, 4), (21, 28), ALPHA_W, ALPHA_H),
    "none": [0, 0],                                                  # AlignUV returns -1: texel (0, 0)
    "in 127": _rect((45, 19), (58, 26), ALPHA_W, ALPHA_H),
}
ROTATED = ("interior", "interior reversed", "low edges", "high edges", "one texel")
# AlbedoTexScale: negative scales and offsets among them; about 0.6 in size, so that BaseUv's uncertainty times the
# scale, the rectangle and the atlas width stays a small part of a texel (the 0 / 255 checkerboard's margin grows with it)
SCALES = ((0.8, 0.4, 0.25, -0.4), (-0.5, 0.7, 0.3, 0.2), (0.55, -0.7, -0.35, 0.6), (0.6, 0.6, 0.0, 0.0),
          (0.35, 0.85, -0.15, -0.7))
N_MAT = 16
GLASS_CUTOUT = 13
# MatDat 0 .. 16 (16 is past a parent's table: the next parent's material 0, or zeros past the last)
MATDAT_P = (0.178, 0.07, 0.07, 0.07, 0.07, 0.07, 0.07, 0.04, 0.05, 0.012, 0.03, 0.07, 0.05, 0.06, 0.04, 0.03, 0.02)


def material_table(parent, equal_only=False):
    """(materials, rectangle kind per material or None, cutoff kind per material or None) of one parent: opaque
    (0, 15), Cutout (1 .. 10), textured glass (11), untextured glass (12), glass + Cutout (13), Invisible (14).
    The rectangles of materials 1 .. 5 rotate with the parent's index, so a wrong MaterialOffset picks a wrong
    rectangle. equal_only: every Cutout material gets the interior rectangle and the cutoff 128 / 255."""
    m = np.zeros(N_MAT, tthip.MAT_DTYPE)
    rects, cuts = [None] * N_MAT, [None] * N_MAT
    mids = (0.45, 0.3, 0.6, 0.5, 0.55, 0.4)

    def cutout(i, rect, cutoff, kind):
        m[i]["MatType"] = tthip.MAT_CUTOUT_INDEX
        m[i]["AlphaTex"] = RECTS[rect]
        m[i]["AlphaCutoff"] = cutoff
        m[i]["AlbedoTexScale"] = SCALES[(i + parent) % len(SCALES)]
        rects[i], cuts[i] = rect, kind

    for i in range(1, 6):
        cutout(i, ROTATED[(i - 1 + parent) % 5], mids[i - 1], "inside")
    cutout(6, "none", mids[5], "inside")
    cutout(7, "interior", 0.0, "zero")
    cutout(8, "interior", 1.5, "above one")
    cutout(9, "interior", EQUAL, "equal")
    cutout(10, "in 127", EQUAL, "equal over 127")
    for i in (11, 12, 13):
        m[i]["specTrans"] = 1.0
        m[i]["surfaceColor"] = ((0.9, 0.8, 0.7), (0.5, 0.95, 0.6), (0.75, 0.4, 1.0))[i - 11]
        m[i]["AlbedoTexScale"] = SCALES[(i + parent) % len(SCALES)]
    m[11]["AlbedoTex"] = _rect((4, 3), (33, 20), TEX_W, TEX_H)
    m[12]["AlbedoTex"] = [0, 0]
    m[13]["AlbedoTex"] = _rect((40, 24), (8, 2), TEX_W, TEX_H)
    cutout(GLASS_CUTOUT, "low edges", 0.5, "inside")
    m[14]["Tag"] = 1 << tthip.FLAG_INVISIBLE
    if equal_only:
        for i in list(range(1, 11)) + [GLASS_CUTOUT]:
            cutout(i, "interior", EQUAL, "equal")
    return m, rects, cuts


# ------------------------------------------------------------------ scenes
def _affine(scale, c):
    """A 2 x 3 map with no zero entry."""
    return np.array([[0.37, 0.21, -0.29], [-0.23, 0.31, 0.33]]) * scale, np.asarray(c, np.float64)


def _ground():
    """A 16 x 16 grid over [-4, 4]^2 at y = 0 (512 triangles) and an opaque floor one unit below (2 triangles)."""
    k = np.linspace(-4.0, 4.0, 17)
    x, z = np.meshgrid(k, k, indexing="ij")
    pos = np.stack([x.ravel(), np.zeros(x.size), z.ravel()], 1)
    i, j = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    a, b, c, d = (i * 17 + j).ravel(), ((i + 1) * 17 + j).ravel(), ((i + 1) * 17 + j + 1).ravel(), (i * 17 + j + 1).ravel()
    idx = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    floor = np.array([[-5, -1, -5], [5, -1, -5], [5, -1, 5], [-5, -1, 5]], np.float64)
    idx = np.concatenate([idx, len(pos) + np.array([[0, 1, 2], [0, 2, 3]])])
    return np.concatenate([pos, floor]), idx.astype(np.int32), 2


@dataclasses.dataclass
class Part:
    pos: np.ndarray      # float32 vertices
    idx: np.ndarray      # int32 (n, 3)
    matdat: np.ndarray
    l2w: np.ndarray
    affine: tuple        # (A, c), or None for random per-corner UVs
    uvs: np.ndarray

    def mesh(self):
        return tthip.ArrayMesh(self.pos, self.idx, uvs=self.uvs, matdat=self.matdat)


def _part(pos, idx, l2w, affine, seed, opaque_tail=0):
    pos = np.asarray(pos, np.float32)
    rng = np.random.default_rng(seed)
    drawn = len(idx)  # (a flat index array draws three values per triangle; the first of every mesh's run are used)
    idx = np.asarray(idx, np.int32).reshape(-1, 3)
    md = rng.choice(N_MAT + 1, drawn, p=MATDAT_P)[:len(idx)]
    if opaque_tail:
        md[-opaque_tail:] = 0
    uvs = (pos.astype(np.float64) @ affine[0].T + affine[1]).astype(np.float32)
    return Part(pos, idx, md.astype(np.int32), np.asarray(l2w, np.float64), affine, uvs)


@functools.lru_cache(maxsize=None)
def parts(name):
    """The meshes of an affine-UV scene, UVs running over about -3 .. 3.
    "parts": the ground grid over its floor under an identity parent, an icosphere under a rotated parent with a
    non-uniform scale, another under a mirrored parent. "soup": a 3,000-triangle soup under a mirrored parent."""
    if name == "parts":
        gp, gi, tail = _ground()
        sp, si = PC.icosphere(2)
        return (_part(gp, gi, np.eye(4), _affine(1.6, (0.15, -0.2)), 81, opaque_tail=tail),
                _part(sp * 1.4, si, PC.trs((0.6, 1.2, 0.4), PC.rotation((1, 2, 3), 40.0), (1.5, 1.0, 0.6)),
                      _affine(3.4, (-0.3, 0.45)), 82),
                _part(sp * 1.2, si, PC.trs((-2.1, 1.0, -1.2), PC.rotation((0.3, 1.0, -0.2), 65.0), (-1.3, 1.0, 1.0)),
                      _affine(-3.9, (0.2, 0.1)), 83))
    assert name == "soup"
    pos, _, idx = tthip.Mesh.soup(1, 3000, 2.0, 0.2).arrays()
    return (_part(pos, idx, PC.trs((0.2, -0.1, 0.3), PC.rotation((0.2, 1.0, 0.1), 25.0), (-1.0, 1.0, 1.0)),
                  _affine(2.2, (0.1, -0.35)), 84),)


def assemble(name, blases, add="add_parent"):
    """The AssetManager of a scene over its parts' BLASes (or device-built objects with add='add_parent_object'),
    one material table per parent."""
    am = tthip.AssetManager()
    for k, (p, b) in enumerate(zip(parts(name), blases)):
        getattr(am, add)(b, p.l2w, material_table(k)[0])
    return am


def check_order(sc, name):
    """The mesh records stand in the order of the parts, each at its own MaterialOffset."""
    ps = parts(name)
    assert len(sc.meshdata) == len(ps)
    for k, p in enumerate(ps):
        w2l = sc.meshdata["W2L"][k].reshape(4, 4).T
        assert np.allclose(w2l, np.linalg.inv(p.l2w), atol=1e-5) and sc.meshdata["MaterialOffset"][k] == k * N_MAT


@functools.lru_cache(maxsize=None)
def _host_scene(name):
    if name == "rsoup":
        rng = np.random.default_rng(85)
        sc = tthip.single_object_scene(tthip.Mesh.soup(2, 3000, 2.0, 0.2), n_materials=N_MAT)
        n = len(sc.tris)
        for f in ("tex0", "texedge1", "texedge2"):
            sc.tris[f] = rng.uniform(-1.5, 1.5, (n, 2))
        sc.tris["MatDat"] = rng.choice(N_MAT + 1, n, p=MATDAT_P)
        sc.materials = material_table(0)[0]
        return sc
    sc = assemble(name, [tthip.Blas(p.mesh()) for p in parts(name)]).build()
    check_order(sc, name)
    return sc


def with_atlases(sc, atlas, **kw):
    return dataclasses.replace(sc, alpha_atlas=alpha_atlas(atlas), texture_atlas=texture_atlas(), **kw)


@functools.lru_cache(maxsize=None)
def scene(name, atlas="noise", equal_only=False):
    """The host-built scene under one of the alpha atlases. Shared between tests: do not write to it."""
    sc = _host_scene(name)
    kw = {}
    if equal_only:
        kw["materials"] = np.concatenate([material_table(k, True)[0] for k in range(len(sc.materials) // N_MAT)])
    return with_atlases(sc, atlas, **kw)


def affine_of(name):
    return None if name == "rsoup" else [p.affine for p in parts(name)]


@functools.lru_cache(maxsize=None)
def model(name, atlas="noise", variant=None, uv="record", equal_only=False):
    return M.Model(scene(name, atlas, equal_only), uv=uv, affine=affine_of(name), variant=variant)


def kinds(name):
    """(rectangle kind, cutoff kind) per material index of the scene's concatenated table."""
    n = 1 if name == "rsoup" else len(parts(name))
    r, c = [], []
    for k in range(n):
        _, rk, ck = material_table(k)
        r, c = r + rk, c + ck
    return r, c


# ------------------------------------------------------------------ ray sets
CLOSEST_SETS = ("random", "axis", "big")
SHADOW_SETS = ("random", "axis", "nee", "enclosing", "big")
_SEED = {"parts": 300, "soup": 310, "rsoup": 320}


def _geometry(name):
    return model(name).g


@functools.lru_cache(maxsize=None)
def closest_rays(name, ray_set):
    g = _geometry(name)
    seed = _SEED[name] + CLOSEST_SETS.index(ray_set)
    if ray_set == "axis":
        o, d = C.axis_rays(g, seed, N_RAYS)
    else:
        o, d = C.random_rays(g, seed, N_BIG if ray_set == "big" else N_RAYS)
    return C.ray_buffer(o, d)


def enclosing_rays(g, seed, n):
    """Segments that start and end outside the scene's bounds: through a point of the bounds grown by a quarter,
    from 1.05 of the grown box's diagonal before it to as far behind it."""
    rng = np.random.default_rng(seed)
    lo, hi = C._box(g, 0.25)
    p = rng.uniform(lo, hi, (n, 3))
    k = n // 2
    p[k:] = C.surface_points(g, rng, n - k)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    R = 1.05 * np.linalg.norm(hi - lo)
    o = (p - d * R).astype(np.float32)
    r = C.shadow_buffer(o, d.astype(np.float32), seed)
    r["t"] = np.float32(2 * R) * np.sign(r["t"])
    return r


def is_enclosing(g, r):
    lo, hi = g.bounds()
    o = r["origin"].astype(np.float64)
    e = o + r["direction"].astype(np.float64) * np.abs(r["t"].astype(np.float64))[:, None]
    return (((o < lo) | (o > hi)).any(1) & ((e < lo) | (e > hi)).any(1)).all()


def shadow_rays(name, ray_set, traced=None):
    """(rays, width, height). The NEE set is made from `traced`, the NEE_W x NEE_H frame of nee_frame() as the
    caller's side traced it."""
    g = _geometry(name)
    seed = _SEED[name] + 5 + SHADOW_SETS.index(ray_set)
    if ray_set == "nee":
        return C.nee_shadow_rays(traced, C.nee_camera(g)[2], seed), C.NEE_W, C.NEE_H
    if ray_set == "axis":
        o, d = C.axis_rays(g, seed, N_RAYS)
        return C.axis_shadow_buffer(g, o, d, seed), N_RAYS, 1
    if ray_set == "enclosing":
        r = enclosing_rays(g, seed, N_RAYS)
        assert is_enclosing(g, r)
        return r, N_RAYS, 1
    n = N_BIG if ray_set == "big" else N_RAYS
    o, d = C.random_rays(g, seed, n)
    return C.shadow_buffer(o, d, seed), n, 1


# ------------------------------------------------------------------ references and comparisons
@functools.lru_cache(maxsize=None)
def closest_reference(name, atlas, ray_set, flags, bounce, variant=None, uv="record"):
    """(model's closest hits, rays the material margins alone make unrobust)."""
    rays = closest_rays(name, ray_set)
    n = len(rays) // 2
    mdl = model(name, atlas, variant, uv)
    ref = mdl.closest(rays["origin"][:n], rays["direction"][:n], FAR, flags, bounce)
    added = 0
    if variant is None:
        sure = mdl.closest(rays["origin"][:n], rays["direction"][:n], FAR, flags, bounce, sure=True)
        added = int((sure.robust & ~ref.robust).sum())
    return ref, added


def _material_cap(rep, added, n):
    rep.text += f", material margins add {added} unrobust rays ({added / n:.4f})"
    if added > MAX_MATERIAL_MARGINAL * n:
        rep.failures.append(f"material margins make {added} of {n} rays unrobust (cap {MAX_MATERIAL_MARGINAL:.0%})")
    return rep


def compare_closest(name, atlas, ray_set, flags, bounce, hits, variant=None, uv="record", caps=True):
    ref, added = closest_reference(name, atlas, ray_set, flags, bounce, variant, uv)
    rep = C.compare_closest(ref, hits, caps=caps)
    return _material_cap(rep, added, len(hits)) if variant is None else rep


def any_hit_reference(mdl, before, visibility_check=False, count_added=True):
    """(bruteforce.AnyHit, materials.Tint or None, rays the material margins alone make unrobust)."""
    o, d, t = before["origin"], before["direction"], before["t"]
    ref, tint = mdl.any_hit(o, d, t, visibility_check)
    added = 0
    if count_added and mdl.variant is None:
        sure, _ = mdl.any_hit(o, d, t, visibility_check, sure=True)
        added = int((sure.robust & ~ref.robust).sum())
    return ref, tint, added


def compare_any_hit(mdl, before, out, bounce, visibility_check=False, reference=None, caps=True):
    """out: (after, vis, col, nee, status or None) as the caller's side left them."""
    ref, tint, added = reference or any_hit_reference(mdl, before, visibility_check)
    after, vis, col, nee, status = out
    rep = C.compare_any_hit(ref, before, after, vis, col, nee, bounce, visibility_check, status, caps=caps, tint=tint,
                            tint_check=M.tint_check)
    return _material_cap(rep, added, len(before)) if mdl.variant is None else rep


def check_uv(mdl, ref, rays):
    """Record UV against surface UV on every robust hit of an affine scene: (largest ratio to db, hits checked)."""
    w = np.nonzero(ref.hit & ref.robust)[0]
    o, d = rays["origin"][w].astype(np.float64), rays["direction"][w].astype(np.float64)
    t, u, v, _, cu, cv = BF.hit_details(mdl.g, o, d, ref.mesh[w], ref.tri[w])
    mdl.stats = M.Stats(np.zeros(mdl.n_mat + 1, np.int64))
    mdl.check_uv(ref.mesh[w], ref.tri[w], o, d, t, u, v, cu, cv)
    st = mdl.stats
    assert not st.uv_bad, f"record UV and surface UV differ by {st.uv_ratio:.3g} of db, triangles {st.uv_bad}"
    return st.uv_ratio, st.uv_checked


# ------------------------------------------------------------------ coverage
class Coverage:
    """The floors of COVERAGE, gathered over a scene family's cases."""

    def __init__(self, family):
        self.family = family
        self.n = {k: 0 for k in COVERAGE if k != "each kind"}
        self.rect, self.cut = {}, {}
        self.wrap = {"negative": 0, "positive": 0}

    def _kinds(self, name, stats, atlas):
        """The cutoff 128 / 255 is an exact equality under the marker atlas alone, and counts there alone."""
        r, c = kinds(name)
        for i, k in enumerate(stats.mat_hits[:len(r)]):
            if r[i] is not None and c[i].startswith("equal") == (atlas == "marker"):
                self.rect[r[i]] = self.rect.get(r[i], 0) + int(k)
                self.cut[c[i]] = self.cut.get(c[i], 0) + int(k)
        self.wrap["negative"] += stats.wrap_neg
        self.wrap["positive"] += stats.wrap_pos

    def closest(self, name, atlas, ray_set, flags, bounce):
        ref, _ = closest_reference(name, atlas, ray_set, flags, bounce)
        mdl = model(name, atlas)
        rays = closest_rays(name, ray_set)
        n = len(rays) // 2
        win = ref.hit & ref.robust
        mi = mdl._mat(ref.mesh[win], ref.tri[win])
        self.n["cutout hits"] += int(((mi >= 0) & (mdl.mat_type[np.maximum(mi, 0)] == M.CUTOUT)).sum())
        opaque = BF.closest(mdl.g, rays["origin"][:n], rays["direction"][:n], FAR, flags, bounce)
        both = ref.robust & opaque.robust & opaque.hit
        self.n["alpha-rejected first"] += int((both & ((ref.tri != opaque.tri) | (ref.mesh != opaque.mesh))).sum())
        self._kinds(name, ref.stats, atlas)

    def any_hit(self, name, mdl, before, ref, tint, resolved, atlas):
        opaque = BF.any_hit(mdl.g, before["origin"], before["direction"], before["t"])
        see = ref.robust & ~ref.occluded
        self.n["visible by rejection"] += int((see & opaque.robust & opaque.occluded).sum())
        ok = see & ~tint.unrobust
        self.n["tinted"] += int((ok & (tint.r_n >= 1)).sum())
        self.n["tinted twice"] += int((ok & (tint.r_n >= 2)).sum())
        self.n["resolved with O"] += resolved
        self._kinds(name, ref.stats, atlas)

    def text(self):
        return f"{self.family}: {self.n}, rectangles {self.rect}, cutoffs {self.cut}, wrap {self.wrap}"

    def check(self):
        print(self.text())
        short = [f"{k} {v} < {COVERAGE[k]}" for k, v in self.n.items() if v < COVERAGE[k]]
        for what, have, want in (("rectangle", self.rect, tuple(RECTS)),
                                 ("cutoff", self.cut, ("inside", "zero", "above one", "equal", "equal over 127")),
                                 ("wrap", self.wrap, ("negative", "positive"))):
            short += [f"{what} '{k}' {have.get(k, 0)} < {COVERAGE['each kind']}" for k in want
                      if have.get(k, 0) < COVERAGE["each kind"]]
        assert not short, "; ".join(short) + " | " + self.text()


# ------------------------------------------------------------------ numpy edits of a correct output
def scaled_row(vis, tint, ref):
    """A copy of the visibility rows with the row of one robustly visible tinted ray scaled by 1 + 2^-20."""
    i = int(np.nonzero(ref.robust & ~ref.occluded & ~tint.unrobust & (tint.r_n >= 1))[0][0])
    out = vis.copy()
    out[i, :3] *= np.float32(1 + 2.0 ** -20)
    return out


def floor_triangle(sc):
    """A triangle of the opaque floor under the ground grid (y = -1), as the scene's triangle array numbers it."""
    return int(np.nonzero((sc.tris["pos0"][:, 1] == -1) & (sc.tris["posedge1"][:, 1] == 0) & (sc.tris["posedge2"][:, 1] == 0))[0][0])


def moved_record(hits, ref, floor_tri):
    """A copy of the hit records with one robust hit's triangle id moved to the opaque floor."""
    i = int(np.nonzero(ref.robust & ref.hit & (ref.tri != floor_tri))[0][0])
    out = hits.copy()
    out[i, 1] = floor_tri
    return out


# ------------------------------------------------------------------ the matrix, for either side
SCENES = AFFINE + ("rsoup",)
# the NEE set needs something between a surface and the light, as in the brute-force matrix: the two soups
SHADOW_CASES = [(n, s) for n in SCENES for s in ("random", "axis", "nee", "enclosing") if s != "nee" or n != "parts"]
CONTROL_MIN = 20
TEXTURE_CONTROLS = ("swap_samplers", "transpose_atlas", "flip_rows", "swap_corners", "clamp_wrap", "drop_offset",
                    "swap_texedges", "no_half_texel", "albedo_for_alpha")


class Side:
    """What a test file's side (the oracle, the kernels) wrote for a case, each launch made once. A subclass gives
    trace(scene, rays, n, flags, bounce) -> hit records of that half, shadow(scene, before, W, H, bounce,
    visibility_check) -> (after, vis, col, nee, status or None) and nee_frame(scene, c2w, ip) -> the traced frame."""

    def __init__(self):
        self._c, self._s, self._r, self._ref = {}, {}, {}, {}

    def closest(self, name, atlas, ray_set, flags, bounce, equal_only=False):
        key = (name, atlas, ray_set, flags, bounce, equal_only)
        if key not in self._c:
            rays = closest_rays(name, ray_set)
            self._c[key] = self.trace(scene(name, atlas, equal_only), rays, len(rays) // 2, flags, bounce)
        return self._c[key]

    def shadow_rays(self, name, ray_set):
        """The NEE set comes from a frame the side generates and traces itself (under the noise atlas)."""
        key = (name, ray_set)
        if key not in self._r:
            traced = None
            if ray_set == "nee":
                c2w, ip, _ = C.nee_camera(model(name).g)
                traced = self.nee_frame(scene(name), c2w, ip)
            self._r[key] = shadow_rays(name, ray_set, traced)
        return self._r[key]

    def any_hit(self, name, atlas, ray_set, bounce, visibility_check, equal_only=False):
        key = (name, atlas, ray_set, bounce, visibility_check, equal_only)
        if key not in self._s:
            before, W, H = self.shadow_rays(name, ray_set)
            self._s[key] = self.shadow(scene(name, atlas, equal_only), before, W, H, bounce, visibility_check)
        return self._s[key]

    def reference(self, name, atlas, ray_set, visibility_check):
        key = (name, atlas, ray_set, visibility_check)
        if key not in self._ref:
            self._ref[key] = any_hit_reference(model(name, atlas), self.shadow_rays(name, ray_set)[0], visibility_check)
        return self._ref[key]


def closest_case(side, name, atlas, ray_set, flags, bounce, uv="record"):
    return compare_closest(name, atlas, ray_set, flags, bounce, side.closest(name, atlas, ray_set, flags, bounce), uv=uv)


def any_hit_case(side, name, atlas, ray_set, bounce, visibility_check):
    reference = side.reference(name, atlas, ray_set, visibility_check)
    if ray_set == "enclosing" and not visibility_check:
        # O has two kinds of member: a glass pair that is robust in u, v and in its texel and lies outside the t range
        # (o_range counts these), and a pair that is marginal in u, v, t, its texel or its alpha test. A segment that
        # begins and ends outside the bounds rules out the first kind by construction, which is what is asserted;
        # marginal pairs occur on any ray set, stay in O and are resolved by the subset rule.
        assert reference[1].o_range.sum() == 0, "a segment that encloses the scene has a glass pair outside its t range"
    return compare_any_hit(model(name, atlas), side.shadow_rays(name, ray_set)[0],
                           side.any_hit(name, atlas, ray_set, bounce, visibility_check), bounce, visibility_check, reference)


def uv_case(side, name):
    """On every robust hit of an affine-UV scene the record's UV is A p + c of the hit point, within the smaller of
    the two sources' db; and the whole comparison holds with the surface UV in the record UV's place."""
    worst, n = 0.0, 0
    for ray_set in CLOSEST_SETS:
        ref, _ = closest_reference(name, "noise", ray_set, 0, 1)
        rays = closest_rays(name, ray_set)
        ratio, k = check_uv(model(name), ref, rays[:len(rays) // 2])
        worst, n = max(worst, ratio), n + k
    print(f"{name}: largest record-versus-surface UV ratio to db {worst:.3g} over {n} robust hits")
    assert n >= 1000
    for flags, bounce in ((0, 1), (C.FLAGS[3], 0)):
        closest_case(side, name, "noise", "random", flags, bounce, uv="surface").check()


def coverage_case(side, family):
    """The floors of COVERAGE over the family's cases, on the model's classes; the exact-equality cutoff counts
    under the marker atlas alone, where the texels it meets are 128 and 127."""
    cov = Coverage(family)
    ratios = [0.0, 0.0]
    for name in FAMILIES[family]:
        for ray_set in CLOSEST_SETS:
            cov.closest(name, "noise", ray_set, 0, 1)
        for atlas, sets in (("noise", [s for n, s in SHADOW_CASES if n == name] + ["big"]), ("marker", ["random", "big"])):
            for ray_set in sets:
                ref, tint, _ = reference = side.reference(name, atlas, ray_set, False)
                before = side.shadow_rays(name, ray_set)[0]
                rep = compare_any_hit(model(name, atlas), before, side.any_hit(name, atlas, ray_set, 0, False), 0, False,
                                      reference, caps=False)
                assert not rep.failures, rep.failures
                ratios = [max(a, b) for a, b in zip(ratios, rep.tint[:2])]
                cov.any_hit(name, model(name, atlas), before, ref, tint, rep.tint[2], atlas)
    print(f"{family}: largest tint ratio {ratios[0]:.3g}, largest Direct ratio {ratios[1]:.3g}")
    cov.check()


def control_mismatches(side, variant, name, atlas, closest_sets, shadow_sets, equal_only=False):
    """Robust mismatches of a deliberately wrong model against the side's outputs, and the failure texts."""
    mdl = model(name, atlas, variant, "record", equal_only)
    total, texts = 0, []
    for ray_set in closest_sets:
        rays = closest_rays(name, ray_set)
        n = len(rays) // 2
        ref = mdl.closest(rays["origin"][:n], rays["direction"][:n], FAR, 0, 1)
        rep = C.compare_closest(ref, side.closest(name, atlas, ray_set, 0, 1, equal_only), caps=False)
        total, texts = total + rep.mismatches, texts + rep.failures
    for ray_set in shadow_sets:
        before = side.shadow_rays(name, ray_set)[0]
        rep = compare_any_hit(mdl, before, side.any_hit(name, atlas, ray_set, 0, False, equal_only), 0, False,
                              any_hit_reference(mdl, before, False, count_added=False), caps=False)
        total, texts = total + rep.mismatches, texts + rep.failures
    print(variant, total, texts)
    return total, texts


def control_texture_space(side, variant):
    total, texts = control_mismatches(side, variant, "soup", "noise", ("random", "axis"), ("random", "nee"))
    assert total >= CONTROL_MIN and texts, (variant, total)


def control_tints(side):
    """The tint without (+ 2) / 3; the tint applied only inside the t range, which cannot differ on segments that
    enclose the scene (no glass pair lies outside their t range) and does on the NEE set, whose rows need members of
    O; a Cutout rejection that does not cancel the tint of glass + Cutout."""
    rows = lambda texts: any("visibility row" in t for t in texts)
    total, texts = control_mismatches(side, "tint_no_2_3", "soup", "noise", (), ("random", "nee"))
    assert total >= CONTROL_MIN and rows(texts), (total, texts)
    total, texts = control_mismatches(side, "tint_in_range_only", "soup", "noise", (), ("enclosing",))
    assert total == 0 and not texts, (total, texts)
    total, texts = control_mismatches(side, "tint_in_range_only", "soup", "noise", (), ("nee",))
    assert total >= CONTROL_MIN and rows(texts), (total, texts)
    total, texts = control_mismatches(side, "cutout_keeps_tint", "soup", "noise", (), ("big",))
    assert total >= CONTROL_MIN and rows(texts), (total, texts)


def control_equality(side):
    """Every Cutout material with the cutoff 128 / 255 over texels of 128: `<` keeps the surface (the point sampler's
    equality is exact and robust), `<=` rejects it."""
    total, texts = control_mismatches(side, None, "rsoup", "marker", (), ("random",), equal_only=True)
    assert total == 0 and not texts, (total, texts)
    total, texts = control_mismatches(side, "le_cutoff", "rsoup", "marker", (), ("random",), equal_only=True)
    assert total >= CONTROL_MIN and texts, (total, texts)


def control_numpy_edits(side):
    """One visibility row scaled by 1 + 2^-20; one hit record's triangle id moved to the opaque floor."""
    name = "parts"
    before = side.shadow_rays(name, "big")[0]
    ref, tint, _ = reference = side.reference(name, "noise", "big", False)
    after, vis, col, nee, status = side.any_hit(name, "noise", "big", 0, False)
    rep = compare_any_hit(model(name), before, (after, scaled_row(vis, tint, ref), col, nee, status), 0, False, reference)
    assert rep.mismatches >= 1 and any("visibility row" in t for t in rep.failures), rep.failures
    hits = side.closest(name, "noise", "random", 0, 1)
    cref, _ = closest_reference(name, "noise", "random", 0, 1)
    rep = compare_closest(name, "noise", "random", 0, 1, moved_record(hits, cref, floor_triangle(scene(name))))
    assert rep.mismatches == 1 and any("robust rays differ" in t for t in rep.failures), rep.failures
