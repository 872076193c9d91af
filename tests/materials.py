"""Float64 texture-space model of the Cutout alpha test and the stained-glass shadow tint (test
infrastructure: numpy only, no GPU, no oracle).

Of a ``tthip.Scene`` it reads the triangle records (positions, ``tex0``, ``texedge1``, ``texedge2``,
``MatDat``), the mesh records, the materials (``MatType``, ``AlphaCutoff``, ``AlphaTex``, ``AlbedoTex``,
``AlbedoTexScale``, ``specTrans``, ``surfaceColor``, ``Tag``) and the two atlases; never the nodes, the TLAS,
the oracle or the per-material records the engine derives. It is written from the reference's text:
AlignUV (CommonData.cginc:569-591, Rotation 0, IsAlbedo false), the closest hit's alpha test with the linear
sampler (IntersectionKernels.compute:35-40), the shadow path with the point sampler (CommonData.cginc:611-629:
the material is read before the t range is tested, a Cutout rejection also cancels the tint of a glass + Cutout
surface, a glass surface inside the triangle tints whatever its t) and the filter definition of
truetrace_hip.h (point = texel clamp(floor(uv * size)); linear = taps at floor(uv * size - 0.5) and + 1,
clamped, lerp in x then y). A texel is ``np.float32(k) / np.float32(255)``, one correctly rounded float32
quotient; half texels convert exactly; everything else is float64. It plugs into ``bruteforce.closest`` /
``bruteforce.any_hit`` through their material hook.

Two UV sources, named by the caller (``Model(uv=...)``):

* "record": tex0 (1 - u - v) + texedge1 u + texedge2 v from the record, u, v the float64 ones;
* "surface": for a mesh whose vertex UVs are an affine function of object position, uv_k = A p_k + c, the UV
  at the hit is A (o_obj + t d_obj) + c: no tex* field, no corner order, no leaf order. After a refit it is
  A (the same barycentric combination of the rest corners) + c, the rest corners rebuilt from the vertex array.

Uncertainty, each a count of float32 roundings times the magnitudes they act on (U = 2^-24, K =
bruteforce.K_ROUNDINGS, cond_u / cond_v of bruteforce.hit_details):

* du = K U cond_u, dv = K U cond_v: the bound compare_closest holds the kernels' u, v to.
* BaseUv, per component: w = 1 - u - v costs two roundings of magnitudes <= 1 beside du + dv, the three
  products one each and the two sums one each of magnitudes <= |t0| + |t1| + |t2|:
  db = (|t0| + |t1|) du + (|t0| + |t2|) dv + 8 U (|t0| + |t1| + |t2|). The surface source has no record to
  read magnitudes from; with m the largest |A p + c| over the triangle's corners (no order needed) it uses
  db = 2 m (du + dv) + 24 U m, which is no smaller.
* x = b * scale.xy + scale.zw: dx = |s| db + 2 U (|b s| + |o|) (a product and a sum).
* the wrap: fmodf is exact, 1 - f is one rounding of a magnitude <= 1: df = dx + U.
* U_atlas = f (D.xy - D.zw) + D.zw: the rectangle's corners are 15-bit integers over 2^14 and their difference is
  exact; a product and a sum: dU = |D.x - D.z| df + U (|f (D.x - D.z)| + |U_atlas|). In texels, X = U_atlas W
  is one more rounding: dX = W dU + U |X|, and the linear sampler's - 0.5 another, U max(|X|, 0.5).

A (ray, triangle) pair is material-marginal when an integer, 0 included, lies in [x - dx, x + dx] (the wrap's
discontinuity and the sign branch); or, point sampler, the texels whose cells meet [X +- dX] x [Y +- dY] after
the clamp are not all on the same side of the cutoff (texture atlas: not all the same texel value; more than
two cells per axis count as marginal outright); or, linear sampler, |alpha64 - cutoff| <= Gx dX + Gy dY + 12 U,
Gx / Gy the largest difference between horizontally / vertically adjacent taps over the cells of the clamped
3 x 3 cell neighbourhood of the footprint that [X +- dX] x [Y +- dY] meets (the bilinear surface is continuous
and bilinear per cell, so its slopes there are differences of adjacent taps; dX >= 1 counts as marginal
outright; 12 U: one rounding per texel quotient, two weights, four products, two sums and the second lerp's
four, all of magnitude <= 1). alpha == cutoff exactly is robust for the point sampler (`<` is strict: kept) and always marginal for
the linear one.

Tints. For a shadow ray in the default mode, R = the glass pairs robustly inside in u, v with EPS < t <
t_end (1 - EPS), a robust texel pick and, for glass + Cutout, a robust alpha accept: their leaf box holds a
point of the segment, so the traversal reaches them. O = the glass pairs inside or marginal in u, v that are not
in R and not robustly alpha-rejected: the reference tints by them exactly when its traversal reaches their leaf.
A robustly visible ray's visibility row must satisfy, per channel, |row - P| <= ((1 + U)^(4 n + 1) - 1) P for P
= prod(R + S), some S in O, n = |R + S| (each tint three roundings, each product one). Rays with |O| > 4, or
with an O member whose tint is itself uncertain, count as unrobust. Where R + O is empty the row is exactly ones.
"""
from __future__ import annotations

import dataclasses
import itertools
from dataclasses import dataclass, field

import numpy as np

import bruteforce as BF
import tthip

U24 = BF.U24
EPS = BF.EPS
CUTOUT = tthip.MAT_CUTOUT_INDEX
MAX_O = 4

# deliberately wrong variants (the controls of materials_cases.py)
VARIANTS = ("swap_samplers", "transpose_atlas", "flip_rows", "swap_corners", "clamp_wrap", "drop_offset",
            "swap_texedges", "no_half_texel", "albedo_for_alpha", "tint_no_2_3", "tint_in_range_only",
            "cutout_keeps_tint", "le_cutoff")


@dataclass
class Tint:
    """The tint classes of a shadow launch, per ray."""
    r_prod: np.ndarray    # (n, 3) product of the tints of R
    r_n: np.ndarray       # |R|
    o_tints: list         # per ray: list of (3,) tints of O
    unrobust: np.ndarray  # |O| > MAX_O, or an O member with an uncertain tint
    o_range: np.ndarray   # O members that are there for their t alone (robust in u, v and texel)


@dataclass
class Stats:
    """What the robust alpha tests of a launch touched: per material index, and the wrap's two signs."""
    mat_hits: np.ndarray
    wrap_neg: int = 0
    wrap_pos: int = 0
    marginal_pairs: int = 0
    uv_ratio: float = 0.0   # largest |record UV - surface UV| / db
    uv_checked: int = 0
    uv_bad: list = field(default_factory=list)


class Model:
    """The material path of one scene: `closest` and `any_hit` are bruteforce's with the alpha test hooked in."""

    def __init__(self, sc, tris=None, geometry=None, uv="record", affine=None, rest=None, variant=None):
        """tris: the triangle records (default the scene's; a device-assembled scene's are read back).
        geometry: a bruteforce.Geometry (default: of those records). affine: per mesh record (A, c) or None.
        rest: (p0, e1, e2) float64 rest positions in record order, for the surface UV after a refit."""
        assert variant is None or variant in VARIANTS
        self.variant = variant
        tris = sc.tris if tris is None else tris
        self.g = geometry if geometry is not None else BF.Geometry.from_scene(dataclasses.replace(sc, tris=tris))
        self.t0, self.t1, self.t2 = (tris[f].astype(np.float64) for f in ("tex0", "texedge1", "texedge2"))
        if variant == "swap_texedges":
            self.t1, self.t2 = self.t2, self.t1
        m = sc.materials
        self.n_mat = len(m)
        self.mat_type = m["MatType"].astype(np.int64)
        self.cutoff = m["AlphaCutoff"].astype(np.float32).astype(np.float64)
        self.alpha_tex = m["AlphaTex"].astype(np.int64)
        self.albedo_tex = m["AlbedoTex"].astype(np.int64)
        self.scale = m["AlbedoTexScale"].astype(np.float32).astype(np.float64)
        self.glass = m["specTrans"].astype(np.float32) == np.float32(1.0)
        self.color = m["surfaceColor"].astype(np.float32).astype(np.float64)
        self.tag = m["Tag"].astype(np.int64)
        a = sc.alpha_atlas
        self.alpha = None
        if a is not None:
            a = np.ascontiguousarray(a, np.uint8)
            self.alpha_h, self.alpha_w = a.shape
            self.alpha = (a.reshape(-1).astype(np.float32) / np.float32(255)).astype(np.float64)
        t = sc.texture_atlas
        self.tex = None
        if t is not None:
            t = np.ascontiguousarray(t, np.float16)
            self.tex_h, self.tex_w = t.shape[:2]
            self.tex = t.reshape(-1, 4)[:, :3].astype(np.float64)
        self.uv = uv
        if affine is not None:  # a mesh record without an affine map (None) reads zeros and is never asked
            self.A = np.stack([np.zeros((2, 3)) if a is None else np.asarray(a[0], np.float64) for a in affine])
            self.c = np.stack([np.zeros(2) if a is None else np.asarray(a[1], np.float64) for a in affine])
        self.rest = None if rest is None else tuple(np.asarray(x, np.float64) for x in rest)
        self.sure = False  # True: a marginal alpha test counts as passed (to count what the margins add)
        self.stats = Stats(np.zeros(self.n_mat + 1, np.int64))
        self.skip = (1 << tthip.TT_FLAG_IS_BACKGROUND) | (1 << tthip.TT_FLAG_SHADOW_CASTER)

    # ------------------------------------------------------------------ materials of a block
    def _mat(self, m, tri):
        """(material index or -1 past the table) per triangle index under mesh record m."""
        mi = self.g.mat_offset[m] + self.g.matdat[tri]
        return np.where((mi >= 0) & (mi < self.n_mat), mi, -1)

    # ------------------------------------------------------------------ BaseUv and its bound
    def base_uv(self, m, tri, o, d, t, u, v, cu, cv, source=None):
        """(b, db), (n, 2) each, of ray i against triangle tri[i] of mesh record m[i] (o, d world space)."""
        source = source or self.uv
        du, dv = (BF.K_ROUNDINGS * U24 * cu)[:, None], (BF.K_ROUNDINGS * U24 * cv)[:, None]
        if source == "record":
            t0, t1, t2 = self.t0[tri], self.t1[tri], self.t2[tri]
            b = t0 * (1 - u - v)[:, None] + t1 * u[:, None] + t2 * v[:, None]
            a0, a1, a2 = np.abs(t0), np.abs(t1), np.abs(t2)
            return b, (a0 + a1) * du + (a0 + a2) * dv + 8 * U24 * (a0 + a1 + a2)
        g = self.g
        A, c = self.A[m], self.c[m]
        if self.rest is None:
            W = g.w2l[m]
            oo = np.einsum("nij,nj->ni", W[:, :3, :3], o) + W[:, :3, 3]
            dd = np.einsum("nij,nj->ni", W[:, :3, :3], d)
            p = oo + t[:, None] * dd
            P0, E1, E2 = g.p0[tri], g.e1[tri], g.e2[tri]
        else:
            P0, E1, E2 = (x[tri] for x in self.rest)
            p = P0 + u[:, None] * E1 + v[:, None] * E2
        b = np.einsum("nij,nj->ni", A, p) + c
        corners = np.stack([P0, P0 + E1, P0 + E2], 1)
        mag = np.abs(np.einsum("nij,nkj->nki", A, corners) + c[:, None, :]).max(1)
        return b, 2 * mag * (du + dv) + 24 * U24 * mag

    # ------------------------------------------------------------------ AlignUV
    def align(self, b, db, mi, tex):
        """AlignUV of BaseUv b +- db under material mi's AlbedoTexScale and the rectangle tex (n, 2 ints).
        Returns (UV, dUV, marginal at the wrap, x before the wrap)."""
        s = self.scale[mi]
        off = np.zeros_like(s[:, 2:]) if self.variant == "drop_offset" else s[:, 2:]
        x = b * s[:, :2] + off
        dx = np.abs(s[:, :2]) * db + 2 * U24 * (np.abs(b * s[:, :2]) + np.abs(off))
        wrapm = (np.ceil(x - dx) <= np.floor(x + dx)).any(1)
        if self.variant == "clamp_wrap":
            f = np.clip(x, 0.0, 1.0)
        else:
            f = np.where(x < 0, 1.0 - np.fmod(np.abs(x), 1.0), np.fmod(np.abs(x), 1.0))
        df = dx + U24
        tx, ty = tex[:, 0], tex[:, 1]
        hi = np.stack([(tx & 0x7FFF) / 16384.0, (tx >> 15) / 16384.0], 1)  # TexDim.xy
        lo = np.stack([(ty & 0x7FFF) / 16384.0, (ty >> 15) / 16384.0], 1)  # TexDim.zw
        if self.variant == "swap_corners":
            hi, lo = lo, hi
        uv = f * (hi - lo) + lo
        duv = np.abs(hi - lo) * df + U24 * (np.abs(f * (hi - lo)) + np.abs(uv))
        none = tx <= 0  # AlignUV returns -1: both samplers clamp to texel (0, 0)
        uv = np.where(none[:, None], -1.0, uv)
        duv = np.where(none[:, None], 0.0, duv)
        wrapm &= ~none
        if self.variant == "flip_rows":
            uv = np.stack([uv[:, 0], 1.0 - uv[:, 1]], 1)
        return uv, duv, wrapm, np.where(none[:, None], np.nan, x)

    # ------------------------------------------------------------------ samplers
    def _fetch(self, flat, w, h, x, y):
        x, y = x.astype(np.int64), y.astype(np.int64)
        return flat[x * h + y] if self.variant == "transpose_atlas" else flat[y * w + x]

    def point(self, flat, w, h, uv, duv):
        """Point-clamp candidates: (values (n, 4, ...) at the corner cells of the uncertainty box, too wide)."""
        X, Y = uv[:, 0] * w, uv[:, 1] * h
        dX, dY = w * duv[:, 0] + U24 * np.abs(X), h * duv[:, 1] + U24 * np.abs(Y)
        xl, xh = np.clip(np.floor(X - dX), 0, w - 1), np.clip(np.floor(X + dX), 0, w - 1)
        yl, yh = np.clip(np.floor(Y - dY), 0, h - 1), np.clip(np.floor(Y + dY), 0, h - 1)
        wide = (xh - xl > 1) | (yh - yl > 1)
        vals = np.stack([self._fetch(flat, w, h, a, b) for a in (xl, xh) for b in (yl, yh)], 1)
        return vals, wide

    def linear(self, flat, w, h, uv, duv):
        """Bilinear-clamp value in float64 and its uncertainty."""
        half = 0.0 if self.variant == "no_half_texel" else 0.5
        X0, Y0 = uv[:, 0] * w, uv[:, 1] * h
        X, Y = X0 - half, Y0 - half
        dX = w * duv[:, 0] + U24 * np.abs(X0) + U24 * np.maximum(np.abs(X), 0.5)
        dY = h * duv[:, 1] + U24 * np.abs(Y0) + U24 * np.maximum(np.abs(Y), 0.5)
        x0, y0 = np.floor(X), np.floor(Y)
        fx, fy = X - x0, Y - y0
        cols = [np.clip(x0 + k, 0, w - 1) for k in (-1, 0, 1, 2)]
        rows = [np.clip(y0 + k, 0, h - 1) for k in (-1, 0, 1, 2)]
        T = np.stack([np.stack([self._fetch(flat, w, h, c, r) for c in cols], 1) for r in rows], 1)  # (n, row, col)
        a = T[:, 1, 1] * (1 - fx) + T[:, 1, 2] * fx
        b = T[:, 2, 1] * (1 - fx) + T[:, 2, 2] * fx
        val = a * (1 - fy) + b * fy
        # the cells (pairs of adjacent taps) that [X +- dX] x [Y +- dY] meets: cell k of T's axis lies between its
        # entries k and k + 1, the footprint is cell 1
        k3, k4 = np.arange(3)[None, :], np.arange(4)[None, :]
        cl, ch = (np.floor(X - dX) - x0 + 1)[:, None], (np.floor(X + dX) - x0 + 1)[:, None]
        rl, rh = (np.floor(Y - dY) - y0 + 1)[:, None], (np.floor(Y + dY) - y0 + 1)[:, None]
        cells_x, cells_y = (k3 >= cl) & (k3 <= ch), (k3 >= rl) & (k3 <= rh)
        taps_x, taps_y = (k4 >= cl) & (k4 <= ch + 1), (k4 >= rl) & (k4 <= rh + 1)
        gx = (np.abs(T[:, :, 1:] - T[:, :, :-1]) * (taps_y[:, :, None] & cells_x[:, None, :])).max((1, 2))
        gy = (np.abs(T[:, 1:, :] - T[:, :-1, :]) * (cells_y[:, :, None] & taps_x[:, None, :])).max((1, 2))
        return val, gx * dX + gy * dY + 12 * U24, (dX >= 1) | (dY >= 1)

    def alpha_test(self, b, db, mi, sampler):
        """(rejected robustly, marginal, x before the wrap) of the alpha test of material mi at BaseUv b +- db."""
        if self.variant == "swap_samplers":
            sampler = "point" if sampler == "linear" else "linear"
        tex = self.albedo_tex[mi] if self.variant == "albedo_for_alpha" else self.alpha_tex[mi]
        uv, duv, wrapm, x = self.align(b, db, mi, tex)
        cut = self.cutoff[mi]
        if sampler == "point":
            vals, wide = self.point(self.alpha, self.alpha_w, self.alpha_h, uv, duv)
            rej = vals <= cut[:, None] if self.variant == "le_cutoff" else vals < cut[:, None]
            marg = wrapm | wide | (rej.any(1) != rej.all(1))
            return rej.all(1) & ~marg, marg, x
        val, err, wide = self.linear(self.alpha, self.alpha_w, self.alpha_h, uv, duv)
        marg = wrapm | wide | (np.abs(val - cut) <= err)
        rej = val <= cut if self.variant == "le_cutoff" else val < cut
        return rej & ~marg, marg, x

    def tint(self, b, db, mi):
        """(tint (n, 3), robust texel pick) of glass material mi at BaseUv b +- db."""
        uv, duv, wrapm, _ = self.align(b, db, mi, self.albedo_tex[mi])
        vals, wide = self.point(self.tex, self.tex_w, self.tex_h, uv, duv)
        same = (vals == vals[:, :1]).all((1, 2))
        x = vals[:, 0]
        tint = self.color[mi] * x if self.variant == "tint_no_2_3" else self.color[mi] * (x + 2.0) / 3.0
        return tint, same & ~wide & ~wrapm

    # ------------------------------------------------------------------ hooks
    def _pairs(self, m, lo, B, sel, o, d):
        r, k = np.nonzero(sel)
        tri = lo + k
        mm = np.full(len(r), m)
        t, u, v, _, cu, cv = BF.hit_details(self.g, o[r], d[r], mm, tri)
        return r, k, tri, mm, t, u, v, cu, cv

    def _count(self, mi, x, robust_in):
        st = self.stats
        np.add.at(st.mat_hits, mi[robust_in], 1)
        xs = x[robust_in]
        xs = xs[np.isfinite(xs).all(1)]
        st.wrap_neg += int((xs < 0).any(1).sum())
        st.wrap_pos += int((xs >= 0).any(1).sum())

    def check_uv(self, m, tri, o, d, t, u, v, cu, cv):
        """Record UV against surface UV on given hits; accumulates the largest ratio to min(db, db)."""
        b1, d1 = self.base_uv(m, tri, o, d, t, u, v, cu, cv, "record")
        b2, d2 = self.base_uv(m, tri, o, d, t, u, v, cu, cv, "surface")
        ratio = np.abs(b1 - b2) / np.minimum(d1, d2)
        st = self.stats
        st.uv_checked += len(tri)
        if len(tri):
            st.uv_ratio = max(st.uv_ratio, float(ratio.max()))
            st.uv_bad += [int(x) for x in tri[(ratio > 1).any(1)][:5]]

    def closest_hook(self, origins, dirs, far):
        o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)

        def hook(m, lo, hi, B):
            rej, uns = np.zeros(B.t.shape, bool), np.zeros(B.t.shape, bool)
            mi_t = self._mat(m, np.arange(lo, hi))
            cut = (mi_t >= 0) & (self.mat_type[np.maximum(mi_t, 0)] == CUTOUT)
            if not cut.any():
                return rej, uns
            with np.errstate(invalid="ignore"):
                sel = cut[None, :] & B.good & ~BF._uv_out(B) & (B.t > -EPS) & (B.t < far * (1 + EPS))
            r, k, tri, mm, t, u, v, cu, cv = self._pairs(m, lo, B, sel, o, d)
            if not len(r):
                return rej, uns
            mi = mi_t[k]
            b, db = self.base_uv(mm, tri, o[r], d[r], t, u, v, cu, cv)
            rj, mg, x = self.alpha_test(b, db, mi, "linear")
            rej[r, k], uns[r, k] = rj, mg & (not self.sure)
            inn = BF._uv_in(B)[r, k] & (t > EPS)
            self._count(mi, x, inn & ~mg)
            self.stats.marginal_pairs += int((inn & mg).sum())
            return rej, uns

        return hook

    def any_hit_hook(self, origins, dirs, t_end, acc):
        """acc: None (visibility-check mode: no tints), or a dict the tint classes are gathered into."""
        o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)

        def hook(m, lo, hi, B):
            rej, uns = np.zeros(B.t.shape, bool), np.zeros(B.t.shape, bool)
            mi_t = self._mat(m, np.arange(lo, hi))
            safe = np.maximum(mi_t, 0)
            live = (mi_t >= 0) & ((self.tag[safe] & self.skip) == 0)
            cut = live & (self.mat_type[safe] == CUTOUT)
            gls = live & self.glass[safe]
            want = cut | gls if acc is not None else cut & ~gls
            if not want.any():
                return rej, uns
            notout = ~BF._uv_out(B)
            if acc is not None:
                bad = (gls[None, :] & notout & ~B.good).any(1)  # a glass pair whose u, v are not to be had
                acc["unrobust"] |= bad
            r, k, tri, mm, t, u, v, cu, cv = self._pairs(m, lo, B, want[None, :] & B.good & notout, o, d)
            if not len(r):
                return rej, uns
            mi = mi_t[k]
            b, db = self.base_uv(mm, tri, o[r], d[r], t, u, v, cu, cv)
            is_cut, is_gls = cut[k], gls[k]
            rj, mg = np.zeros(len(r), bool), np.zeros(len(r), bool)
            te = t_end[r]
            inn = BF._uv_in(B)[r, k]
            in_t = (t > EPS) & (t < te * (1 - EPS)) & (te > 0)
            if is_cut.any():
                c = np.nonzero(is_cut)[0]
                rj[c], mg[c], x = self.alpha_test(b[c], db[c], mi[c], "point")
                self._count(mi[c], x, (inn & in_t & ~mg)[c])
                self.stats.marginal_pairs += int((inn & in_t & mg)[c].sum())
            op = is_cut & ~is_gls
            rej[r[op], k[op]], uns[r[op], k[op]] = rj[op], mg[op] & (not self.sure)
            if acc is None or not is_gls.any():
                return rej, uns
            keep_tint = self.variant == "cutout_keeps_tint"
            gl = np.nonzero(is_gls & (keep_tint | ~rj))[0]  # a robust Cutout rejection cancels the tint
            tint, pick = self.tint(b[gl], db[gl], mi[gl])
            sure_alpha = np.ones(len(gl), bool) if keep_tint else ~mg[gl]
            in_r = inn[gl] & in_t[gl] & pick & sure_alpha
            with np.errstate(invalid="ignore"):
                out_t = (t[gl] < -EPS) | (t[gl] > te[gl] * (1 + EPS)) | (te[gl] <= 0)
            for j in np.nonzero(in_r)[0]:
                acc["r_prod"][r[gl[j]]] *= tint[j]
                acc["r_n"][r[gl[j]]] += 1
            for j in np.nonzero(~in_r)[0]:
                ray = r[gl[j]]
                range_only = bool(inn[gl[j]] and pick[j] and sure_alpha[j] and out_t[j])
                if self.variant == "tint_in_range_only" and range_only:
                    continue
                if not pick[j]:
                    acc["unrobust"][ray] = True
                acc["o"][ray].append(tint[j])
                acc["o_range"][ray] += range_only
            return rej, uns

        return hook

    # ------------------------------------------------------------------ the two queries
    def closest(self, origins, dirs, far, flags=0, bounce=0, sure=False):
        """bruteforce.Closest with the alpha test, and what the test touched as its `stats`."""
        self.sure, self.stats = sure, Stats(np.zeros(self.n_mat + 1, np.int64))
        ref = BF.closest(self.g, origins, dirs, far, flags, bounce, material=self.closest_hook(origins, dirs, far))
        ref.stats = self.stats
        return ref

    def any_hit(self, origins, dirs, t_ray, visibility_check=False, sure=False):
        """(bruteforce.AnyHit with `stats`, Tint or None in the visibility-check mode, which writes no tint)."""
        self.sure, self.stats = sure, Stats(np.zeros(self.n_mat + 1, np.int64))
        n = len(origins)
        t_ray = np.asarray(t_ray, np.float64)
        t_end = t_ray if visibility_check else np.abs(t_ray)
        acc = None
        if not visibility_check:
            acc = {"r_prod": np.ones((n, 3)), "r_n": np.zeros(n, np.int64), "o": [[] for _ in range(n)],
                   "unrobust": np.zeros(n, bool), "o_range": np.zeros(n, np.int64)}
        ref = BF.any_hit(self.g, origins, dirs, t_ray, visibility_check,
                         material=self.any_hit_hook(origins, dirs, t_end, acc))
        ref.stats = self.stats
        if acc is None:
            return ref, None
        unrobust = acc["unrobust"] | (np.array([len(x) for x in acc["o"]]) > MAX_O)
        return ref, Tint(acc["r_prod"], acc["r_n"], acc["o"], unrobust, acc["o_range"])


def tint_check(tint: Tint, rows, where):
    """Rows (n, 3) of the rays in `where` against the subset rule. Returns (bad ray indices, largest ratio of
    |row - P| to its bound over the rays a subset resolves, rays with O non-empty that a subset resolves,
    rays that need a non-empty S)."""
    bad, worst, resolved, needed = [], 0.0, 0, 0
    rows = np.asarray(rows, np.float64)
    for i in np.nonzero(where & ~tint.unrobust)[0]:
        O = tint.o_tints[i]
        if tint.r_n[i] == 0 and not O:
            if not (rows[i] == 1.0).all():
                bad.append(int(i))
            continue
        best, best_s = np.inf, 0
        for s in range(len(O) + 1):
            for S in itertools.combinations(range(len(O)), s):
                P = tint.r_prod[i].copy()
                for j in S:
                    P = P * O[j]
                n = int(tint.r_n[i]) + s
                bound = ((1 + U24) ** (4 * n + 1) - 1) * np.abs(P)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(bound > 0, np.abs(rows[i] - P) / bound, np.where(rows[i] == P, 0.0, np.inf)).max()
                if ratio < best:
                    best, best_s = float(ratio), s
        if best > 1:
            bad.append(int(i))
        else:
            worst = max(worst, best)
            resolved += bool(O)
            needed += best_s > 0
    return bad, worst, resolved, needed
