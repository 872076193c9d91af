"""Float64 brute-force reference for closest-hit and any-hit queries (test infrastructure: numpy only,
no GPU, no oracle).

Of a ``tthip.Scene`` it reads the triangles (``pos0``, ``posedge1``, ``posedge2``, ``MatDat``), the mesh
records (``W2L``, ``TriOffset``, ``MaterialOffset``) and the materials (``specTrans``, ``Tag``); never the
nodes, the TLAS or anything else a builder or a kernel wrote. Every mesh record is an instance. A ray is
taken into object space with the float64 ``W2L`` and its direction is not renormalised, so ``t`` is the
world parameter. Moller-Trumbore runs for every (ray, instance triangle) pair, vectorised over rays x
triangles in blocks; there is no per-ray Python loop.

Every pair is classified with ``EPS`` = 1e-4 (``abar`` = |a| / (|e1| |e2| |d_obj|), the sine of the angle
between the ray and the triangle's plane):

* IN: u, v, u + v inside the triangle by EPS, t inside the open range by EPS (relative to the range's end,
  absolute at 0), abar > 1e-7 and the material filter accepts robustly;
* OUT: one of those inequalities fails by EPS with abar > 1e-7, or the material filter rejects robustly, or
  the range is empty, or the pair is *termwise parallel* (below);
* MARGINAL: everything else.

Termwise parallel: every one of the six products of the scalar triple product a = e1 . (d_obj x e2) has a
factor that is exactly zero, the components of d_obj counting as zero only where every product W2L[k][j] *
d[j] of theirs has a zero factor. A product with a zero factor is zero in any floating-point format, so the
float32 chain (matrix-vector fma chain, cross, fma dot) gives a = +-0 exactly, 1 / a = +-inf, u = +-inf or
NaN, and ``u >= 0 && u <= 1`` is false: such a pair is rejected whatever the rounding. This is the case of an
axis-parallel ray (two +-0 components) over an axis-aligned triangle, which would otherwise sit at abar = 0.

Material filters (IntersectionKernels.compute:42-47 and the Invisible test behind them for the closest hit;
CommonData.cginc:611-629 for the any-hit). Closest, range (0, far): rejected when IGNORE_GLASS and specTrans
== 1; or IGNORE_BACKFACING at bounce 0 with specTrans != 1 and c <= 0, c = dot(normalize(cross(e1, e2)),
d_obj / |d_obj|), robust for |c| > 1e-5 and marginal otherwise; or at bounce 0 with the Invisible bit of Tag.
Any-hit, range (0, |t_ray|), or (0, t_ray) in the visibility-check mode (empty for t_ray <= 0): rejected for
IsBackground, ShadowCaster or specTrans == 1. A material index outside the table reads a zero material.

Cutout materials and glass tints are the business of materials.py, the float64 texture-space model: it hands
``closest`` and ``any_hit`` a material hook, ``material(m, lo, hi, B) -> (reject, unsure)``, two boolean arrays
of the block's shape. A rejected pair is OUT whatever its geometry (the alpha test rejects robustly), an unsure
pair that is not rejected otherwise is MARGINAL (the alpha test could turn on a float32 rounding). Without a
hook nothing changes: Cutout materials count as opaque, and ``any_hit`` only says for which rays no glass
triangle can have tinted (the tints depend on which nodes a traversal reaches; materials.py bounds them).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import tthip

EPS = 1e-4
ABAR_MIN = 1e-7
C_MIN = 1e-5
# roundings in the float32 chain of one hit: transform 3 + 3, subtract 1, two crosses 2 + 2, two fused dots
# 3 + 3, reciprocal 1, product 1, plus one for slack
K_ROUNDINGS = 20
U24 = 2.0 ** -24
BLOCK = 1 << 20  # (ray, triangle) pairs per block

_TERMS = ((0, 1, 2), (0, 2, 1), (1, 2, 0), (1, 0, 2), (2, 0, 1), (2, 1, 0))  # e1[k] * d[i] * e2[j]


def _norm(x):
    return np.sqrt((x * x).sum(-1))


class Geometry:
    """The triangles, instances and materials the reference tests rays against, all float64."""

    def __init__(self, p0, e1, e2, matdat, w2l, tri_offset, mat_offset, spec_trans, tag):
        self.p0, self.e1, self.e2 = (np.asarray(a, np.float64) for a in (p0, e1, e2))
        self.matdat = np.asarray(matdat).astype(np.uint32).view(np.int32).astype(np.int64)  # (int)MatDat
        self.w2l = np.asarray(w2l, np.float64)
        self.mat_offset = np.asarray(mat_offset, np.int64)
        self.spec_trans = np.asarray(spec_trans, np.float32)
        self.tag = np.asarray(tag).astype(np.int64)
        offs = [int(x) for x in tri_offset]
        starts = sorted(set(offs))
        ends = dict(zip(starts, starts[1:] + [len(self.p0)]))
        self.ranges = [(o, ends[o]) for o in offs]

    @classmethod
    def from_scene(cls, sc, p0=None, e1=None, e2=None, meshdata=None):
        """p0 / e1 / e2 replace the scene's triangle positions (a deformed mesh), meshdata its mesh records
        (moved instances)."""
        md = sc.meshdata if meshdata is None else meshdata
        w2l = md["W2L"].reshape(-1, 4, 4).transpose(0, 2, 1)  # column-major -> row-major
        return cls(sc.tris["pos0"] if p0 is None else p0, sc.tris["posedge1"] if e1 is None else e1,
                   sc.tris["posedge2"] if e2 is None else e2, sc.tris["MatDat"], w2l, md["TriOffset"],
                   md["MaterialOffset"], sc.materials["specTrans"], sc.materials["Tag"])

    def world_corners(self, m):
        """The three corners of every triangle of mesh record m in world space, (3 * n, 3)."""
        lo, hi = self.ranges[m]
        p0 = self.p0[lo:hi]
        obj = np.concatenate([p0, p0 + self.e1[lo:hi], p0 + self.e2[lo:hi]])
        l2w = np.linalg.inv(self.w2l[m])
        return obj @ l2w[:3, :3].T + l2w[:3, 3]

    def bounds(self):
        w = np.concatenate([self.world_corners(m) for m in range(len(self.ranges))])
        return w.min(0), w.max(0)

    def _material(self, m, lo, hi):
        """(glass, tag) per triangle of [lo, hi) under mesh record m; out of range reads zeros."""
        mi = self.mat_offset[m] + self.matdat[lo:hi]
        ok = (mi >= 0) & (mi < len(self.spec_trans))
        mi = np.where(ok, mi, 0)
        if len(self.spec_trans) == 0:
            return np.zeros(hi - lo, bool), np.zeros(hi - lo, np.int64)
        return ok & (self.spec_trans[mi] == np.float32(1.0)), np.where(ok, self.tag[mi], 0)

    def blocks(self, o, d):
        """Moller-Trumbore per block: yields (m, lo, hi, B) with B the (rays, triangles) arrays."""
        n = len(o)
        for m, (t0, t1) in enumerate(self.ranges):
            W = self.w2l[m]
            oo = o @ W[:3, :3].T + W[:3, 3]
            dd = d @ W[:3, :3].T
            zd = ((W[None, :3, :3] == 0) | (d[:, None, :] == 0)).all(2)  # (rays, 3): exactly zero, termwise
            dn = _norm(dd)
            step = max(1, BLOCK // max(n, 1))
            for lo in range(t0, t1, step):
                hi = min(lo + step, t1)
                yield m, lo, hi, _moller_trumbore(oo, dd, dn, zd, self.p0[lo:hi], self.e1[lo:hi], self.e2[lo:hi])


@dataclass
class _Block:
    u: np.ndarray
    v: np.ndarray
    t: np.ndarray
    good: np.ndarray      # abar > ABAR_MIN
    parallel: np.ndarray  # termwise parallel
    c: np.ndarray         # dot(unit normal, unit direction)


def _moller_trumbore(oo, dd, dn, zd, P0, E1, E2):
    h = np.cross(dd[:, None, :], E2[None, :, :])
    a = np.einsum("tk,rtk->rt", E1, h)
    s = oo[:, None, :] - P0[None, :, :]
    q = np.cross(s, E1[None, :, :])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        f = 1.0 / a
        u = f * np.einsum("rtk,rtk->rt", s, h)
        v = f * np.einsum("rk,rtk->rt", dd, q)
        t = f * np.einsum("tk,rtk->rt", E2, q)
        n1, n2 = _norm(E1), _norm(E2)
        abar = np.abs(a) / (n1 * n2)[None, :] / dn[:, None]
        nrm = np.cross(E1, E2)
        nrm = nrm / _norm(nrm)[:, None]
        c = (dd @ nrm.T) / dn[:, None]
    z1, z2 = E1 == 0, E2 == 0
    par = np.ones(a.shape, bool)
    for k, i, j in _TERMS:
        par &= z1[None, :, k] | zd[:, i, None] | z2[None, :, j]
    return _Block(u, v, t, abar > ABAR_MIN, par, c)


def _uv_in(B):
    with np.errstate(invalid="ignore"):  # inf - inf of a ray parallel to the triangle's plane: neither in nor out
        return (B.u > EPS) & (B.u < 1 - EPS) & (B.v > EPS) & (B.u + B.v < 1 - EPS)


def _uv_out(B):
    """Robustly outside the triangle, by u and v alone."""
    with np.errstate(invalid="ignore"):
        return B.parallel | (B.good & ((B.u < -EPS) | (B.u > 1 + EPS) | (B.v < -EPS) | (B.u + B.v > 1 + EPS)))


def _classify(B, t_end, accept, reject):
    """(IN, MARGINAL) of a block for the open range (0, t_end) per ray (empty where t_end <= 0)."""
    te = t_end[:, None]
    with np.errstate(invalid="ignore"):
        inside = _uv_in(B) & (B.t > EPS) & (B.t < te * (1 - EPS)) & B.good & accept & (te > 0)
        outside = _uv_out(B) | (B.good & ((B.t < -EPS) | (B.t > te * (1 + EPS)))) | reject | (te <= 0)
    return inside, ~inside & ~outside


@dataclass
class Closest:
    hit: np.ndarray      # the reference has a winner (an IN triangle)
    mesh: np.ndarray
    tri: np.ndarray      # index into the scene's triangle array, -1 without a winner
    t: np.ndarray
    u: np.ndarray
    v: np.ndarray
    robust: np.ndarray   # the answer (hit or miss) cannot turn on a float32 rounding
    exact: np.ndarray    # some accepted triangle satisfies the closed float64 inequalities (no margins)
    cond_t: np.ndarray   # condition numbers of the winner's t, u, v
    cond_u: np.ndarray
    cond_v: np.ndarray


def closest(g: Geometry, origins, dirs, far, flags=0, bounce=0, honour_invisible=True, material=None) -> Closest:
    """Closest hit per ray. honour_invisible=False leaves the Invisible test out (a deliberately wrong
    reference, for the tests that prove the comparison can fail). material: the hook of the module docstring."""
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    n = len(o)
    best, second, marg = np.full(n, np.inf), np.full(n, np.inf), np.full(n, np.inf)
    mesh, tri = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    t_end = np.full(n, float(far))
    ar = np.arange(n)
    exact = np.zeros(n, bool)
    for m, lo, hi, B in g.blocks(o, d):
        glass, tag = g._material(m, lo, hi)
        reject = np.zeros(B.t.shape, bool)
        unsure = np.zeros(B.t.shape, bool)
        if material is not None:
            mr, mu = material(m, lo, hi, B)
            reject |= mr
            unsure |= mu
        if flags & tthip.TT_TRACE_IGNORE_GLASS:
            reject |= glass[None, :]
        if bounce == 0 and honour_invisible:
            reject |= (((tag >> tthip.FLAG_INVISIBLE) & 1) == 1)[None, :]
        if (flags & tthip.TT_TRACE_IGNORE_BACKFACING) and bounce == 0:
            with np.errstate(invalid="ignore"):
                reject |= ~glass[None, :] & (B.c < -C_MIN)
                unsure = unsure | (~glass[None, :] & ~(np.abs(B.c) > C_MIN))
        unsure = unsure & ~reject
        inside, marginal = _classify(B, t_end, ~reject & ~unsure, reject)
        with np.errstate(invalid="ignore"):
            exact |= ((B.u >= 0) & (B.u <= 1) & (B.v >= 0) & (B.u + B.v <= 1) & (B.t > 0) & (B.t < far) & ~reject).any(axis=1)
        tin = np.where(inside, B.t, np.inf)
        k = np.argmin(tin, axis=1)
        b1 = tin[ar, k]
        tin[ar, k] = np.inf
        b2 = tin.min(axis=1)
        with np.errstate(invalid="ignore"):
            mt = np.where(marginal, np.where(np.isfinite(B.t), np.maximum(B.t, 0.0), 0.0), np.inf).min(axis=1)
        marg = np.minimum(marg, mt)
        second = np.minimum(np.maximum(best, b1), np.minimum(second, b2))
        better = b1 < best
        best = np.where(better, b1, best)
        mesh = np.where(better, m, mesh)
        tri = np.where(better, lo + k, tri)
    hit = np.isfinite(best)
    with np.errstate(invalid="ignore"):
        lim = best * (1 + EPS)
        robust = np.where(hit, ~(marg <= lim) & ~(second <= lim), ~np.isfinite(marg))
    res = Closest(hit, mesh, tri, best, np.zeros(n), np.zeros(n), robust, exact, np.zeros(n), np.zeros(n), np.zeros(n))
    if hit.any():
        w = np.nonzero(hit)[0]
        t, u, v, ct, cu, cv = hit_details(g, o[w], d[w], mesh[w], tri[w])
        res.u[w], res.v[w], res.cond_t[w], res.cond_u[w], res.cond_v[w] = u, v, ct, cu, cv
    return res


def hit_details(g: Geometry, o, d, mesh, tri):
    """(t, u, v, cond_t, cond_u, cond_v) of ray i against triangle tri[i] of mesh record mesh[i].
    With dx = |s| + |W| |o| + |T| the size of the rounding in s = W o + T - pos0 (|W| the Frobenius norm):
    cond_t = |e1||e2| dx / |e2 . q| + |e1||e2||d| / |a|, cond_u = |e2||d| dx / |a|, cond_v = |e1||d| dx / |a|."""
    W = g.w2l[mesh]
    oo = np.einsum("nij,nj->ni", W[:, :3, :3], o) + W[:, :3, 3]
    dd = np.einsum("nij,nj->ni", W[:, :3, :3], d)
    P0, E1, E2 = g.p0[tri], g.e1[tri], g.e2[tri]
    h = np.cross(dd, E2)
    a = (E1 * h).sum(1)
    s = oo - P0
    q = np.cross(s, E1)
    e2q = (E2 * q).sum(1)
    u, v, t = (s * h).sum(1) / a, (dd * q).sum(1) / a, e2q / a
    n1, n2, nd = _norm(E1), _norm(E2), _norm(dd)
    dx = _norm(s) + _norm(W[:, :3, :3].reshape(-1, 9)) * _norm(o) + _norm(W[:, :3, 3])
    with np.errstate(divide="ignore"):
        cond_t = n1 * n2 * dx / np.abs(e2q) + n1 * n2 * nd / np.abs(a)
        cond_u = n2 * nd * dx / np.abs(a)
        cond_v = n1 * nd * dx / np.abs(a)
    return t, u, v, cond_t, cond_u, cond_v


@dataclass
class AnyHit:
    occluded: np.ndarray
    robust: np.ndarray       # occluded, or no MARGINAL triangle at all
    glass_clear: np.ndarray  # every glass triangle is robustly missed in u, v alone: nothing can have tinted


def any_hit(g: Geometry, origins, dirs, t_ray, visibility_check=False, honour_tags=True, material=None) -> AnyHit:
    """Occlusion per shadow ray. honour_tags=False leaves the IsBackground / ShadowCaster skips out (a
    deliberately wrong reference). material: the hook of the module docstring."""
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    t_ray = np.asarray(t_ray, np.float64)
    n = len(o)
    t_end = t_ray if visibility_check else np.abs(t_ray)
    occluded, marginal_any, clear = np.zeros(n, bool), np.zeros(n, bool), np.ones(n, bool)
    skip = (1 << tthip.TT_FLAG_IS_BACKGROUND) | (1 << tthip.TT_FLAG_SHADOW_CASTER)
    for m, lo, hi, B in g.blocks(o, d):
        glass, tag = g._material(m, lo, hi)
        reject = glass.copy()
        if honour_tags:
            reject |= (tag & skip) != 0
        reject = np.broadcast_to(reject[None, :], B.t.shape)
        accept = ~reject
        if material is not None:
            mr, mu = material(m, lo, hi, B)
            reject = reject | mr
            accept = ~reject & ~mu
        inside, marginal = _classify(B, t_end, accept, reject)
        occluded |= inside.any(axis=1)
        marginal_any |= marginal.any(axis=1)
        clear &= (_uv_out(B) | ~glass[None, :]).all(axis=1)
    return AnyHit(occluded, occluded | ~marginal_any, clear)
