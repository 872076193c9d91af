"""The scenes, seeded ray sets, expectations and comparisons of the float64 terrain pin, shared by
tests/test_terrain_geometry_host.py (the host reference against tests/terrain_geometry.py) and
tests/test_gpu_terrain_geometry.py (the kernels against it). Nothing here calls the host reference, the kernels or
the oracle: a caller traces and hands in what was written.

Scene A is the scene of tests/terrain_cases.py with the head of its randomized set on miss records. Scene B is
one oblong terrain (3 x 6 units, a 17 x 33 rectangle off the origin of a 40 x 48 atlas): a TerrainDim x / y mix-up
or a rectangle mapped with u and v exchanged changes its surface, which they do not on scene A's square terrains."""
import functools

import numpy as np

import terrain_cases as TC
import terrain_geometry as TG
import tthip

FAR = TC.FAR
TID = tthip.TT_TERRAIN_MESH_ID
N_A, N_B, N_SHADOW = 1500, 1200, 1500
N_SHORT = 65              # one full wave and one lane of the next
MARKER = 0x00C0FFEE       # triangle id (and packed uv) of the finite-limit variant's synthetic records
SLOPE_BOUND = 1.95
MISS, HIT, BELOW, AMB = TG.MUST_MISS, TG.MUST_HIT, TG.STARTS_BELOW, TG.AMBIGUOUS
UV_PACKED_TOL = 1.0 / 65535.0 + 4e-7   # tests/test_terrain_host.py's plane test
UV_FLOAT_TOL = 4e-6
GAP_LO, GAP_HI = -2.4e-4, 4.6e-4
NORMAL_TOL = 1e-5


class Case:
    def __init__(self, name, terrains, atlas_bits, rays, w, h):
        self.name, self.terrains, self.atlas_bits, self.rays, self.W, self.H = name, terrains, atlas_bits, rays, w, h
        self.atlas = TG.decode_atlas(atlas_bits)
        self.n = len(rays)
        for a in (terrains, atlas_bits, rays, self.atlas):
            a.setflags(write=False)

    def window(self, bounce):
        return self.W * self.H if bounce % 2 == 1 else 0

    def frame(self, bounce, rays=None):
        """The 2 W H ray buffer with the set in the half bounce reads; every other byte is 0xA5."""
        rays = self.rays if rays is None else rays
        buf = np.zeros(2 * self.W * self.H, tthip.RAY_DTYPE)
        buf.view(np.uint8)[:] = 0xA5
        off = self.window(bounce)
        buf[off:off + len(rays)] = rays
        return buf, off

    def info(self):
        return np.full((self.W * self.H, 4), 0x51515151, np.uint32)


@functools.lru_cache(maxsize=None)
def scene_a() -> Case:
    rays = TC.random_rays()[:N_A].copy()
    TC.miss_records(rays)
    return Case("A", TC.terrains().copy(), TC.atlas().copy(), rays, TC.RW, TC.RH)


B_ATLAS_W, B_ATLAS_H = 40, 48
B_RECT = (9, 5, 17, 33)
B_SEED = 0x7E44C1


@functools.lru_cache(maxsize=None)
def scene_b() -> Case:
    x, y, w, h = B_RECT
    a = np.zeros((B_ATLAS_H, B_ATLAS_W), np.uint16)
    a[y:y + h, x:x + w] = tthip.synthetic_heightmap(B_SEED, w, h)
    t = np.zeros(1, tthip.TERRAIN_DTYPE)
    t[0]["PositionOffset"] = (-1.5, -0.5, -3.0)
    t[0]["HeightScale"] = 0.2
    t[0]["TerrainDim"] = (3.0, 6.0)
    t[0]["HeightMap"] = ((x + w - 0.5) / B_ATLAS_W, (y + h - 0.5) / B_ATLAS_H, (x + 0.5) / B_ATLAS_W,
                         (y + 0.5) / B_ATLAS_H)  # texel centres, as terrain_cases._rect_uv computes them
    t["AlphaMap"] = (1.0, 1.0, 0.0, 0.0)
    rng = np.random.default_rng(0x7E44C2)
    o, d = [], []

    def add(origins, targets=None, dirs=None):
        origins = np.asarray(origins, np.float64)
        dirs = targets - origins if dirs is None else np.asarray(dirs, np.float64)
        o.append(origins.astype(np.float32))
        d.append((dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32))

    def box(n, lo, hi):
        return rng.uniform(lo, hi, (n, 3))

    # 600 from above onto the footprint
    add(box(600, (-1.3, 0.3, -2.8), (1.3, 3.5, 2.8)), box(600, (-1.45, -0.3, -2.95), (1.45, -0.3, 2.95)))
    # 200 from below the surface (which lies in y = -0.49 .. -0.09) upwards
    add(box(200, (-1.4, -0.497, -2.9), (1.4, -0.47, 2.9)), dirs=box(200, (-0.5, 0.3, -0.5), (0.5, 1.0, 0.5)))
    # 200 axis-aligned (zero components: infinite reciprocals), 200 anywhere to anywhere
    axis = np.array([(1, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0)], np.float64)
    add(box(200, (-2.5, -0.3, -4.0), (2.5, 2.0, 4.0)), dirs=axis[rng.integers(0, 6, 200)])
    add(box(200, (-4.0, -0.3, -5.0), (4.0, 3.0, 5.0)), box(200, (-4.0, -0.5, -5.0), (4.0, 1.0, 5.0)))
    w_, h_ = 40, 32
    rays = np.zeros(N_B, tthip.RAY_DTYPE)
    order = rng.permutation(N_B)
    rays["origin"] = np.concatenate(o)[order]
    rays["direction"] = np.concatenate(d)[order]
    rays["PixelIndex"] = rng.permutation(w_ * h_)[:N_B]
    rays["last_pdf"] = 1.0
    TC.miss_records(rays)
    return Case("B", t, a, rays, w_, h_)


def case(name) -> Case:
    return scene_a() if name == "A" else scene_b()


# ------------------------------------------------------------------ expectations
class Expect:
    """Per ray: kind (MISS: the record `keep` stays; HIT / BELOW: a record of `terrain`; AMB: nothing is asserted),
    t0 and t_cross on that terrain."""

    def __init__(self, kind, terrain, t0, t_cross, keep):
        self.kind, self.terrain, self.t0, self.t_cross, self.keep = kind, terrain, t0, t_cross, keep

    def head(self, n):
        return Expect(self.kind[:n], self.terrain[:n], self.t0[:n], self.t_cross[:n], self.keep[:n])

    def shares(self):
        return {k: float((self.kind == v).mean()) for k, v in
                (("miss", MISS), ("hit", HIT), ("below", BELOW), ("ambiguous", AMB))}


def _classify(c: Case, terrain, rays, lim, surf):
    return TG.classify_closest(c.terrains[terrain], c.atlas, rays["origin"], rays["direction"], lim, surf=surf)


@functools.lru_cache(maxsize=None)
def _far_classes(name, terrain):
    c = case(name)
    return _classify(c, terrain, c.rays, FAR, TG.surface)


def expect_one(name, terrain=0, surf=None) -> Expect:
    """The set on miss records against one terrain, uploaded alone (so its index is 0)."""
    c = case(name)
    kind, t0, tc = _far_classes(name, terrain) if surf is None else _classify(c, terrain, c.rays, FAR, surf)
    return Expect(kind, np.zeros(c.n, np.uint32), t0, tc, c.rays["hits"].copy())


def expect_two(after0) -> Expect:
    """Scene A against both terrains, given the records terrain 0 alone leaves (after0, the set's window): terrain
    1 is marched with the limit terrain 0 reported, t_0. It takes the record where it is crossed more than 2e-3
    before that limit runs out (t_cross_1 - t0_1 < t_0 - 2e-3) and leaves terrain 0's record, bit for bit, where
    it is crossed more than 2e-3 after (or not at all)."""
    c = scene_a()
    k0, _, _ = _far_classes("A", 0)
    hit0 = after0["hits"][:, 0] == TID
    lim1 = np.where(hit0, after0["hits"][:, 2].view(np.float32).astype(np.float64), FAR)
    k1, t01, tc1 = _classify(c, 1, c.rays, lim1, TG.surface)
    kind = k1.copy()
    kind[k0 == AMB] = AMB
    return Expect(kind, np.ones(c.n, np.uint32), t01, tc1, after0["hits"].copy())


def two_terrain_sides(e2: Expect, after0):
    """(rays terrain 0 hit and terrain 1 takes, rays terrain 0 hit and keeps though terrain 1 lies on their line)."""
    k1_far, _, _ = _far_classes("A", 1)
    hit0 = after0["hits"][:, 0] == TID
    front = hit0 & ((e2.kind == HIT) | (e2.kind == BELOW))
    behind = hit0 & (e2.kind == MISS) & ((k1_far == HIT) | (k1_far == BELOW))
    return int(front.sum()), int(behind.sum())


@functools.lru_cache(maxsize=None)
def finite_variant():
    """Scene A's set against terrain 0 alone with a synthetic triangle record on every must-hit ray:
    (rays, Expect, rays expected to hit, rays expected to keep their record)."""
    c = scene_a()
    kind, t0, tc = _far_classes("A", 0)
    rng = np.random.default_rng(0x7E44C3)
    f = rng.choice([0.5, 0.9, 1.1, 2.0], c.n)
    mh = kind == HIT
    lim = np.where(mh, t0 + f * (tc - t0), FAR).astype(np.float32)
    rays = c.rays.copy()
    rays["hits"][mh] = np.stack([np.zeros(mh.sum(), np.uint32), np.full(mh.sum(), MARKER, np.uint32),
                                 lim[mh].view(np.uint32), np.full(mh.sum(), MARKER, np.uint32)], 1)
    rays.setflags(write=False)
    lim64 = lim.astype(np.float64)
    k, t0f, tcf = _classify(c, 0, rays, lim64, TG.surface)
    e = Expect(k, np.zeros(c.n, np.uint32), t0f, tcf, rays["hits"].copy())
    reach = tc - t0  # the distance marched to the crossing (:653 compares it with the record's t)
    rule_hit, rule_keep = mh & (reach < lim64 - 2e-3), mh & (reach > lim64 + 2e-3)
    return rays, e, rule_hit, rule_keep


@functools.lru_cache(maxsize=None)
def shadow_set():
    s = TC.shadow_rays()[:N_SHADOW].copy()
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def shadow_classes(surf=None):
    c, s = scene_a(), shadow_set()
    return TG.classify_shadow(c.terrains, c.atlas, s["origin"], s["direction"], s["t"], surf=surf or TG.surface)


# ------------------------------------------------------------------ comparisons
class Report:
    def __init__(self):
        self.bad = {}        # assertion -> indices of the rays that violate it
        self.worst = {}      # measured extremes

    def add(self, what, idx):
        if len(idx):
            self.bad[what] = np.asarray(idx)

    def count(self, what):
        return len(self.bad.get(what, ()))

    def check(self):
        assert not self.bad, {k: v[:8].tolist() for k, v in self.bad.items()} | {"worst": self.worst}
        return self


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def compare_closest(c: Case, e: Expect, before, after, info, bounce, terrains=None, surf=None) -> Report:
    """before / after: the launch's rays (the window, not the buffer) as handed in and as written. info: the
    W H x 4 texture after the launch (or None), 0x51515151 before it. terrains: the records that were uploaded
    (their index in the upload is what a record names); surf: the surface the expectation was classed with."""
    terrains = c.terrains if terrains is None else terrains
    surf = TG.surface if surf is None else surf
    r = Report()
    n = len(before)
    rec = after["hits"]
    for f in ("origin", "direction", "PixelIndex", "last_pdf"):
        r.add("ray fields written", np.nonzero((after[f].view(np.uint32) != before[f].view(np.uint32)).reshape(n, -1)
                                               .any(axis=1))[0])
    hitk = (e.kind == HIT) | (e.kind == BELOW)
    is_ter = rec[:, 0] == TID
    r.add("record", np.nonzero(hitk & ~(is_ter & (rec[:, 1] == e.terrain)))[0])
    r.add("miss", np.nonzero((e.kind == MISS) & (rec != e.keep).any(axis=1))[0])
    ok = np.nonzero(hitk & is_ter & (rec[:, 1] == e.terrain))[0]
    t = rec[:, 2].view(np.float32).astype(np.float64)
    o, d = before["origin"].astype(np.float64), before["direction"].astype(np.float64)
    mh = ok[e.kind[ok] == HIT]
    over = t[mh] - e.t_cross[mh]
    r.add("t past the crossing", mh[over > 1e-5])
    gap = np.full(n, np.nan)
    for ti in np.unique(e.terrain[mh]):
        m = mh[e.terrain[mh] == ti]
        p = o[m] + d[m] * t[m, None]
        gap[m] = p[:, 1] - surf(terrains[ti], c.atlas, p[:, 0], p[:, 2])
    r.add("gap", mh[(gap[mh] < GAP_LO) | (gap[mh] > GAP_HI)])
    sb = ok[e.kind[ok] == BELOW]
    r.add("t of a ray that starts below", sb[np.abs(t[sb] - e.t0[sb]) > 2 * _ulp32(e.t0[sb])])
    # uv: the local x / dimX, z / dimZ of the sample, 1e-4 past the reported point
    uv = np.full((n, 2), np.nan)
    for ti in np.unique(e.terrain[ok]):
        m = ok[e.terrain[ok] == ti]
        T = terrains[ti]
        p = o[m] + d[m] * (t[m, None] + 1e-4)
        uv[m, 0] = np.minimum((p[:, 0] - float(T["PositionOffset"][0])) / float(T["TerrainDim"][0]), 1.0)
        uv[m, 1] = np.minimum((p[:, 2] - float(T["PositionOffset"][2])) / float(T["TerrainDim"][1]), 1.0)
    packed = np.stack([rec[:, 3] & 0xFFFF, rec[:, 3] >> 16], 1).astype(np.float64) / 65535.0
    err_p = np.abs(packed[ok] - uv[ok]).max(axis=1) if len(ok) else np.zeros(0)
    r.add("packed uv", ok[err_p > UV_PACKED_TOL])
    if info is not None:
        pix = before["PixelIndex"]
        rows = info[pix[ok]]
        if bounce == 0:
            r.add("info ids", ok[(rows[:, 0] != TID) | (rows[:, 1] != e.terrain[ok])])
            err_f = np.abs(rows[:, 2:].copy().view(np.float32).astype(np.float64) - uv[ok]).max(axis=1)
            r.add("info uv", ok[~(err_f <= UV_FLOAT_TOL)])
            r.worst["info uv"] = float(err_f.max()) if len(ok) else 0.0
        untouched = np.nonzero((e.kind == MISS) & ~(e.keep[:, 0] == TID))[0]
        r.add("info of a miss written", untouched[(info[pix[untouched]] != 0x51515151).any(axis=1)])
    r.worst.update({"t - t_cross": float(over.max()) if len(mh) else 0.0,
                    "gap": (float(np.nanmin(gap[mh])), float(np.nanmax(gap[mh]))) if len(mh) else (0.0, 0.0),
                    "packed uv": float(err_p.max()) if len(ok) else 0.0})
    return r


def compare_shadow(classes, live, occluded) -> Report:
    r = Report()
    r.add("occluded", np.nonzero((classes == TG.OCCLUDED) & (occluded != 1))[0])
    r.add("clear", np.nonzero((classes == TG.CLEAR) & live & (occluded != 0))[0])
    r.add("not marched", np.nonzero(~live & (occluded != 0))[0])
    return r


def hit_points(c: Case, before, after, count=400):
    """Up to `count` terrain records spread over the launch: (ray indices, float64 hit points o + d t)."""
    ter = np.nonzero(after["hits"][:, 0] == TID)[0]
    ter = ter[:: max(1, len(ter) // count)][:count]
    t = after["hits"][ter, 2].view(np.float32).astype(np.float64)
    pos = before["origin"][ter].astype(np.float64) + before["direction"][ter].astype(np.float64) * t[:, None]
    return ter, pos


def normals64(c: Case, after, ter, pos, terrains=None):
    terrains = c.terrains if terrains is None else terrains
    out = np.zeros((len(ter), 3))
    ids = after["hits"][ter, 1]
    for ti in np.unique(ids):
        m = ids == ti
        out[m] = TG.secant_normal(terrains[ti], c.atlas, pos[m])
    return out


def compare_normals(want, got) -> Report:
    r = Report()
    err = np.abs(np.asarray(got, np.float64) - want).max(axis=1)
    r.add("normal", np.nonzero(~(err <= NORMAL_TOL))[0])
    r.worst["normal"] = float(err.max())
    return r


def compare_bounce(c: Case, traced, rows) -> Report:
    """traced: the launch's rays with their terrain records; rows: the enqueue's surviving terrain rows (any order;
    PixelIndex names the source ray). The numbers are those of tests/test_enqueue.py and
    tests/test_terrain_bounce_host.py: the origin 1e-4 along the flipped normal from the hit point (within 2e-4
    of it, on the side the ray came from), a unit direction within 1e-5, and direction . normal = last_pdf * pi
    within 1e-4 (the sampled frame's axis is the normal after a 16:16 octahedral round trip)."""
    r = Report()
    src = {int(p): i for i, p in enumerate(traced["PixelIndex"])}
    idx = np.array([src[int(p)] for p in rows["PixelIndex"]], np.int64)
    r.add("row of a ray without a terrain record", np.nonzero(traced["hits"][idx, 0] != TID)[0])
    r.add("hits not copied", np.nonzero((rows["hits"] != traced["hits"][idx]).any(axis=1))[0])
    t = traced["hits"][idx, 2].view(np.float32).astype(np.float64)
    d_in = traced["direction"][idx].astype(np.float64)
    pos = traced["origin"][idx].astype(np.float64) + d_in * t[:, None]
    nn = normals64(c, traced, idx, pos)
    side = np.einsum("ij,ij->i", d_in, nn)
    nn = np.where(side[:, None] > 0, -nn, nn)
    firm = np.abs(side) > 1e-4  # (a ray along the tangent plane: the flip may go either way)
    off = rows["origin"].astype(np.float64) - pos
    dist = np.linalg.norm(off, axis=1)
    r.add("origin away from the hit point", np.nonzero(dist > 2e-4)[0])
    r.add("origin behind the surface", np.nonzero(firm & ~(np.einsum("ij,ij->i", off, nn) > 0))[0])
    dd = rows["direction"].astype(np.float64)
    r.add("direction not a unit vector", np.nonzero(np.abs(np.linalg.norm(dd, axis=1) - 1.0) > 1e-5)[0])
    cos = np.einsum("ij,ij->i", dd, nn) - rows["last_pdf"].astype(np.float64) * np.pi
    r.add("direction . normal", np.nonzero(firm & (np.abs(cos) > 1e-4))[0])
    r.worst.update({"origin distance": float(dist.max()), "direction . normal": float(np.abs(cos[firm]).max()),
                    "rows": len(rows), "flipped": int((side > 0).sum())})
    return r
