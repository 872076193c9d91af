"""Float64 model of the colour side of kernel_shadow and kernel_shadow_heightmap (test infrastructure).

Written from the reference's text alone:
  * packRGBE / unpackRGBE             CommonData.cginc:479-509
  * RGB <-> XYZ, EncodeRGB / DecodeRGB  CommonData.cginc:1555-1619
  * the any-hit accumulations          IntersectionKernels.compute:457-485
  * the heightmap accumulations        IntersectionKernels.compute:573-591
It calls no encoder or pow of the oracle, of the engine or of csrc/tt_encode.h: every value below is numpy
float64 arithmetic, pow is ``x ** y``. Literals the text writes without a float representation (409.6, 2.2f, the
matrix entries) enter as the float32 nearest to them, which is the number a float shader computes with.

What the model takes as given is the visibility record a call wrote (float32 rows, w == 1: the ray reached its
light), as bruteforce_cases.compare_any_hit does for Direct: the rows are pinned by tests/bruteforce.py,
tests/materials.py and tests/terrain_geometry.py. For every ray it then says which words and floats of
GlobalColors / CacheBuffer the call may have changed and what each must hold; everything else must be
bytewise what it was.

Error bounds. U = 2^-24 is the unit roundoff of float32. A float32 chain is followed by class F: a pair
(v, e), v the float64 value of the exact expression and e a bound on |float32 result - v|. Each operation of the
text adds the propagated input errors (first order, with the cross term for products) and one rounding
U * (|v| + propagated) + 2^-150 (the last term: a result that underflows). log2 and exp2 count as one rounding
each (DESIGN.md section 8 pins them correctly rounded); multiplications by a power of two, Le + 0.5 and the products
by the literal 1 are exact and add none. Nothing here is fitted to an output.

  * Direct / Indirect: x = C + il * th * k, all terms >= 0. Roundings by the text: il * th (1), * k (1, none
    when k is the literal 1), the add (1); the heightmap form has the add alone. So N = 3, 2 or 1 and
    |out - x| <= ((1 + U)^N - 1) * x + N * 2^-150.
  * pow(x, y) = exp2(y * log2 x) with float intermediates: log2 x is rounded (U |L|), y * L is rounded
    (U |y L|), rcp(2.2f) is rounded (U y, the 1/2.2 exponent only), so the exponent is off by up to
    2 or 3 times U |y log2 x| and the power by that times ln 2, relative, plus the rounding of exp2.
    At x = 1e-6, y = 2.2 that is 2 * 43.9 * 0.693 + 1 = 62 U: the bound follows |y log2 x|, it is no constant.
  * PrimaryNEERay: o = pow(unpack(P), 2.2) + pow(il, 1 / 2.2) * th with its F error E_c per channel.
    floor(log2 max) is exact and va * scale is exact (scale is a power of two), so a word is right when for one
    exponent e with 2^e <= max(o) + E and max(o) - E < 2^(e + 1): its exponent field is clamp(e + 20, 0, 31) and
    every mantissa m_c has |m_c 2^(e-8) - o_c| <= 2^(e-9) + E_c, or m_c == 511 with o_c 2^(8-e) >= 511 - that
    tolerance (min(511, round) leaves a maximum that rounds to 512 one step short). The same rule holds for
    exponent-saturated words: the scale uses the unclamped e, only the field clamps.
  * CurrentIlluminance: s = Decode(old) + il * th * k with F error eps_s (the float32 decode chain, the two
    products, the add). The fields the text computes before uint() are fL = clamp(409.6 (log2 Y + 20), 0, 16383),
    fu = clamp(820 u, 0, 511), fv likewise. Y is linear in RGB with positive weights and u, v are
    linear-fractional, so over the box s +- eps_s (cut at 0: the float32 sum is never negative) their extremes sit
    at its 8 corners. The interval is then widened by the roundings of the field arithmetic itself (the F chain
    of EncodeRGB on an exact input: the three rows, log2 Y, + 20, * 409.6 -- the last alone is half an ulp of a
    number up to 16384, 2^-11 -- the denominator, the reciprocal, the products). A written field must lie in
    [floor(lo), floor(hi)]; Le == 0 at either end allows the word 0; Le saturates at 16383.
"""
from __future__ import annotations

import dataclasses

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -150
SECOND = 1.0 + 2.0 ** -16  # covers the second-order terms the first-order propagation of exp2 / log2 leaves out
LN2 = float(np.log(2.0))


def lit(x):
    """A literal of the text as the float32 nearest to it."""
    return float(np.float32(x))


# CommonData.cginc:1557-1561 and :1566-1570
RGB2XYZ = [[lit(0.4123907992659595), lit(0.3575843393838780), lit(0.1804807884018343)],
           [lit(0.2126390058715104), lit(0.7151686787677559), lit(0.0721923153607337)],
           [lit(0.0193308187155918), lit(0.1191947797946259), lit(0.9505321522496608)]]
XYZ2RGB = [[lit(3.240969941904522), lit(-1.537383177570094), lit(-0.4986107602930032)],
           [lit(-0.9692436362808803), lit(1.875967501507721), lit(0.04155505740717569)],
           [lit(0.05563007969699373), lit(-0.2039769588889765), lit(1.056971514242878)]]
L_SCALE = lit(409.6)   # :1578, :1596
UV_SCALE = 820.0       # :1587, :1605
GAMMA = lit(2.2)       # IntersectionKernels.compute:481, :590

MUTANTS = ("a Rec.601 luma row", "one transposed XYZ entry", "decode without + 0.5", "Le rounded, not truncated",
           "scale 819", "packRGBE truncates", "gamma 2.0", "pow terms swapped", "throughput dropped from PrimaryNEERay",
           "throughput applied in the terrain form", "k applied without ReSTIR GI", "Data.w tests swapped",
           "t > 0 for t >= 0", "Indirect at bounce 0")


def rgb2xyz(mut=None):
    m = [row[:] for row in RGB2XYZ]
    if mut == "a Rec.601 luma row":
        m[1] = [lit(0.299), lit(0.587), lit(0.114)]
    if mut == "one transposed XYZ entry":
        m[0][1], m[1][0] = m[1][0], m[0][1]
    return m


# ------------------------------------------------------------------ float32 chains with their error
class F:
    """v: the float64 value of the exact expression; e: a bound on |the float32 chain's result - v|."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, F) else F(x)

    @staticmethod
    def _rounded(v, p, exact):
        if exact:
            return F(v, p)
        return F(v, p + U * (np.abs(v) + p) + np.where((v != 0) | (p > 0), TINY, 0.0))  # an exact 0 stays exact

    def add(self, o, exact=False):
        o = F.of(o)
        return F._rounded(self.v + o.v, self.e + o.e, exact)

    def sub(self, o, exact=False):
        o = F.of(o)
        return F._rounded(self.v - o.v, self.e + o.e, exact)

    def mul(self, o, exact=False):
        o = F.of(o)
        return F._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e, exact)

    def div(self, o, exact=False):
        o = F.of(o)
        q = self.v / o.v
        room = np.abs(o.v) - o.e
        p = np.where(room > 0, (self.e + np.abs(q) * o.e) / np.where(room > 0, room, 1.0), np.inf)
        return F._rounded(q, p, exact)

    def log2(self):
        room = np.abs(self.v) - self.e
        p = np.where(self.e == 0, 0.0, np.where(room > 0, self.e / (np.where(room > 0, room, 1.0) * LN2), np.inf))
        return F._rounded(np.log2(self.v), p * SECOND, False)

    def exp2(self):
        v = 2.0 ** self.v
        return F._rounded(v, v * (2.0 ** self.e - 1.0) * SECOND, False)

    def max0(self):
        return F(np.maximum(self.v, 0.0), self.e)


def dot3(row, a, b, c):
    """One row of mul(M, c), in any order of evaluation and with or without fused multiply-adds: at most three
    roundings (five without fma, of which each is at most U times the sum of the magnitudes)."""
    v = row[0] * a.v + row[1] * b.v + row[2] * c.v
    mag = abs(row[0]) * np.abs(a.v) + abs(row[1]) * np.abs(b.v) + abs(row[2]) * np.abs(c.v)
    p = abs(row[0]) * a.e + abs(row[1]) * b.e + abs(row[2]) * c.e
    return F(v, p + 3 * U * (mag + p) + np.where((mag != 0) | (p > 0), TINY, 0.0))


def fpow(x, y, y_err=0.0, mut=None):
    """HLSL pow(x, y) = exp2(y * log2 x) on an exact float32 x >= 0 (F with e == 0)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        zero = x.v == 0
        r = F(np.where(zero, 1.0, x.v)).log2().mul(F(y, y_err)).exp2()
        return F(np.where(zero, 0.0, np.where(zero, 1.0, x.v) ** y), np.where(zero, 0.0, r.e))


# ------------------------------------------------------------------ the encoders, from the text
def unpack_rgbe(x):
    """:498-509. A 9-bit field times 2^(E - 28): exact in float32, so no error term."""
    x = np.asarray(x, np.uint32).astype(np.int64)
    scale = 2.0 ** ((x >> 27) - 20) / 256.0
    return np.stack([(x & 0x1FF) * scale, ((x >> 9) & 0x1FF) * scale, ((x >> 18) & 0x1FF) * scale], -1)


def decode_rgb(word, mut=None):
    """:1592-1619 as three F (R, G, B)."""
    w = np.asarray(word, np.uint32).astype(np.int64)
    Le, ue, ve = w >> 18, (w >> 9) & 0x1FF, w & 0x1FF
    half = 0.0 if mut == "decode without + 0.5" else 0.5
    uvs = 819.0 if mut == "scale 819" else UV_SCALE
    with np.errstate(all="ignore"):
        logY = F(Le + half).div(L_SCALE).sub(20.0)               # :1596
        Y = logY.exp2()                                           # :1597 pow(2, .): log2 2 = 1, the product is exact
        u, v = F(ue + half).div(uvs), F(ve + half).div(uvs)       # :1605
        inv = F(1.0).div(u.mul(6.0).sub(v.mul(16.0, exact=True)).add(12.0))   # :1607
        x, y = u.mul(9.0).mul(inv), v.mul(4.0, exact=True).mul(inv)           # :1608
        s = Y.div(y)                                              # :1614
        X, Z = s.mul(x), s.mul(F(1.0).sub(x).sub(y))              # :1615
        M = XYZ2RGB
        out = [dot3(M[k], X, Y, Z).max0() for k in range(3)]     # :1618
    zero = Le == 0                                                # :1594
    return [F(np.where(zero, 0.0, c.v), np.where(zero, 0.0, c.e)) for c in out]


def decode_real(fL, fu, fv):
    """DecodeRGB's formulas (:1596-1618) in plain float64 on real-valued fields (the text decodes at Le + 0.5, ue + 0.5,
    ve + 0.5). Each channel is monotone in each field, so over a box of fields its extremes sit at the corners."""
    M = XYZ2RGB
    Y = 2.0 ** (fL / L_SCALE - 20.0)
    u, v = fu / UV_SCALE, fv / UV_SCALE
    inv = 1.0 / (6.0 * u - 16.0 * v + 12.0)
    x, y = 9.0 * u * inv, 4.0 * v * inv
    s = Y / y
    X, Z = s * x, s * (1.0 - x - y)
    return np.stack([np.maximum(M[k][0] * X + M[k][1] * Y + M[k][2] * Z, 0.0) for k in range(3)], -1)


def round_trip_bound(word, rgb):
    """|DecodeRGB(EncodeRGB(rgb)) - rgb| per channel for an exact float32 rgb whose word is `word` (Le > 0, no field
    clamped): uint() truncates each field and the decode sits at its middle, so rgb lies in the float64 decode of the
    box [Le, Le + 1) x [ue, ue + 1) x [ve, ve + 1), widened by the field roundings of the encoder; the float32 decode
    adds its own error."""
    w = np.asarray(word, np.uint32).astype(np.int64)
    f = [(w >> 18).astype(np.float64), ((w >> 9) & 0x1FF).astype(np.float64), (w & 0x1FF).astype(np.float64)]
    rnd = _field_roundings([np.asarray(rgb, np.float64)[:, c] for c in range(3)])
    mid = decode_real(f[0] + 0.5, f[1] + 0.5, f[2] + 0.5)
    far = np.zeros_like(mid)
    for corner in range(8):
        g = [f[j] + (1.0 + rnd[j] if (corner >> j) & 1 else -rnd[j]) for j in range(3)]
        far = np.maximum(far, np.abs(decode_real(*g) - mid))
    return far + np.stack([c.e for c in decode_rgb(word)], -1)


def _fields(rgb, mut=None):
    """The three real-valued fields of EncodeRGB (:1577-1587) before uint(), unclamped, in plain float64."""
    M = rgb2xyz(mut)
    uvs = 819.0 if mut == "scale 819" else UV_SCALE
    with np.errstate(all="ignore"):
        X, Y, Z = (M[k][0] * rgb[0] + M[k][1] * rgb[1] + M[k][2] * rgb[2] for k in range(3))
        fL = L_SCALE * (np.log2(Y) + 20.0)
        inv = 1.0 / (-2.0 * X + 12.0 * Y + 3.0 * (X + Y + Z))
        return fL, uvs * (4.0 * X * inv), uvs * (9.0 * Y * inv)


def _field_roundings(rgb, mut=None):
    """Bounds on what the float32 evaluation of the three fields adds on an exact input: the F chain of :1577-1587."""
    M = rgb2xyz(mut)
    c = [F(x) for x in rgb]
    with np.errstate(all="ignore"):
        X, Y, Z = (dot3(M[k], *c) for k in range(3))
        fL = Y.log2().add(20.0).mul(L_SCALE)
        den = X.mul(-2.0, exact=True).add(Y.mul(12.0)).add(X.add(Y).add(Z).mul(3.0))
        inv = F(1.0).div(den)
        fu = X.mul(4.0, exact=True).mul(inv).mul(UV_SCALE)
        fv = Y.mul(9.0).mul(inv).mul(UV_SCALE)
    dark = Y.v == 0   # log2 0 is -inf with no rounding to speak of: Le is 0 and the word is 0
    return [np.where(dark, 0.0, np.where(np.isnan(f.e), np.inf, f.e)) for f in (fL, fu, fv)]


@dataclasses.dataclass
class Fields:
    lo: np.ndarray  # (n, 3) int64: lowest allowed Le, ue, ve
    hi: np.ndarray

    @property
    def two_valued(self):
        """A ray whose word has a field with more than one allowed value (chroma only counts where Le can be > 0)."""
        return (self.hi[:, 0] > self.lo[:, 0]) | ((self.hi[:, 0] > 0) & (self.hi[:, 1:] > self.lo[:, 1:]).any(1))

    def allows(self, word):
        w = np.asarray(word, np.uint32).astype(np.int64)
        f = np.stack([w >> 18, (w >> 9) & 0x1FF, w & 0x1FF], -1)
        inside = ((f >= self.lo) & (f <= self.hi)).all(1) & (f[:, 0] > 0)
        return inside | ((w == 0) & (self.lo[:, 0] == 0))


def encode_fields(s, mut=None) -> Fields:
    """The allowed fields of EncodeRGB(s) for s = three F: the 8 corners of s +- e, widened by the field roundings."""
    n = len(s[0].v)
    lo, hi = np.full((3, n), np.inf), np.full((3, n), -np.inf)
    for corner in range(8):
        with np.errstate(invalid="ignore"):
            rgb = [np.maximum(c.v + (c.e if (corner >> k) & 1 else -c.e), 0.0) for k, c in enumerate(s)]
        for j, f in enumerate(_fields(rgb, mut)):
            f = np.where(np.isnan(f), -np.inf, f)  # Y == 0: log2 is -inf and the chroma 0 / 0; Le is 0 then
            lo[j], hi[j] = np.minimum(lo[j], f), np.maximum(hi[j], f)
    rnd = _field_roundings([np.maximum(c.v, 0.0) for c in s], mut)
    top = (16383.0, 511.0, 511.0)
    out_lo, out_hi = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64)
    bump = 0.5 if mut == "Le rounded, not truncated" else 0.0
    for j in range(3):
        b = bump if j == 0 else 0.0
        with np.errstate(invalid="ignore"):
            a_lo, a_hi = lo[j] - rnd[j] + b, hi[j] + rnd[j] + b
        a_lo, a_hi = np.where(np.isnan(a_lo), -np.inf, a_lo), np.where(np.isnan(a_hi), np.inf, a_hi)
        out_lo[:, j] = np.floor(np.clip(a_lo, 0.0, top[j]))      # clamp, then uint(): :1579, :1587
        out_hi[:, j] = np.floor(np.clip(a_hi, 0.0, top[j]))
    return Fields(out_lo, out_hi)


@dataclasses.dataclass
class PackCheck:
    ok: np.ndarray          # the word satisfies the rule
    two_valued: np.ndarray  # more than one exponent, or a mantissa with two allowed values
    ratio: np.ndarray       # (|m 2^(e-8) - o| - 2^(e-9)) / E, largest over the channels (0 where the rounding alone explains it)


def pack_check(word, o, mut=None) -> PackCheck:
    """packRGBE (:479-496) of o = three F with o >= 0 against the word written."""
    w = np.asarray(word, np.uint32).astype(np.int64)
    field = w >> 27
    m = np.stack([w & 0x1FF, (w >> 9) & 0x1FF, (w >> 18) & 0x1FF], -1).astype(np.float64)
    ov, oe = np.stack([c.v for c in o], -1), np.stack([c.e for c in o], -1)
    mx, E = ov.max(1), oe.max(1)
    n = len(w)
    zero = (mx == 0) & (E == 0)                                      # :483
    with np.errstate(all="ignore"):
        e0 = np.floor(np.log2(np.where(mx > 0, mx, 1.0)))
    ok, ncand = np.zeros(n, bool), np.zeros(n, np.int64)
    ratio, wide = np.zeros(n), np.zeros(n, bool)
    shift = 0.5 if mut == "packRGBE truncates" else 0.0
    for de in (-1.0, 0.0, 1.0):
        e = e0 + de
        cand = (2.0 ** e <= mx + E) & (mx - E < 2.0 ** (e + 1)) & ~zero
        ncand += cand
        sc = 2.0 ** (8.0 - e)                                        # :489, exact
        x, tol = ov * sc[:, None] - shift, 0.5 + oe * sc[:, None]
        d = np.abs(m - x)
        fits = (d <= tol) | ((m == 511) & (x >= 511 - tol))          # :490
        good = cand & (field == np.clip(e + 20, 0, 31)) & fits.all(1)  # :487
        r = np.where(oe > 0, np.maximum(d - 0.5, 0.0) / np.where(oe > 0, oe * sc[:, None], 1.0), 0.0)
        ratio = np.where(good & ~ok, np.where(m == 511, 0.0, r).max(1), ratio)
        ok |= good
        wide |= cand & (de == 0) & (np.floor(x + tol) > np.ceil(x - tol)).any(1)
    ok = np.where(zero, w == 0, ok)
    return PackCheck(ok, (ncand > 1) | wide, ratio)


def pack_rgbe_exact(v):
    """packRGBE of exact float32 inputs: floor(log2 max) and va * scale are exact, round is half-to-even, so the
    word follows with no tolerance (finite v, max >= 2^-119)."""
    v = np.maximum(np.asarray(v, np.float64), 0.0)                   # :481
    mx = v.max(-1)
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.where(mx > 0, mx, 1.0)))
    m = np.minimum(511.0, np.rint(v * (2.0 ** (8.0 - e))[..., None])).astype(np.int64)   # np.rint: half to even
    word = (np.clip(e + 20, 0, 31).astype(np.int64) << 27) | m[..., 0] | (m[..., 1] << 9) | (m[..., 2] << 18)
    return np.where(mx == 0, 0, word).astype(np.uint32)


# ------------------------------------------------------------------ the accumulations
ANY_HIT, LEGACY, TERRAIN = "any-hit", "legacy", "terrain"
RADIANCE_CACHE, RESTIRGI = 1 << 7, 1 << 1   # TT_SHADOW_RADIANCE_CACHE, TT_TRACE_USE_RESTIRGI (include/truetrace_hip.h)


@dataclasses.dataclass
class Sum:
    pix: np.ndarray
    x: np.ndarray       # (k, 3) float64
    bound: np.ndarray   # (k, 3)


@dataclasses.dataclass
class Expect:
    """What one call must leave: per touched field the pixels and the values; every other byte is the input's."""
    reached: np.ndarray         # rays whose branch writes anything
    sums: dict                  # "Direct" / "Indirect" -> Sum
    pnee_pix: np.ndarray
    pnee: list                  # three F
    ci_pix: np.ndarray
    ci: Fields | None
    mut: str | None = None


def _sum(C, term, n_round):
    x = C + term
    return x, ((1.0 + U) ** n_round - 1.0) * x + n_round * TINY


def expect(form, rays, vis, col, cache, bounce, flags, W, H, n, mut=None) -> Expect:
    """rays: the shadow rays handed in; vis: the visibility rows the call wrote (None: every launched ray
    reached, rows of ones); col / cache: GlobalColors / CacheBuffer as handed in (cache may be None); n: rays
    launched. The truth tables are :457-485 (any-hit; the legacy entry keeps Direct alone) and :573-591."""
    rc, restir = bool(flags & RADIANCE_CACHE), bool(flags & RESTIRGI)
    t = rays["t"][:n]
    pix = rays["PixelIndex"][:n].astype(np.int64)
    row = np.ones((n, 4), np.float32) if vis is None else np.asarray(vis[:n], np.float32)
    go = (row[:, 3] == 1.0) & (pix < W * H)       # occluded rays, rows with w != 1 and dropped pixels write nothing
    if form == TERRAIN:
        go &= t != 0                               # :570, the heightmap form alone
    idx = np.nonzero(go)[0]
    assert len(np.unique(pix[idx])) == len(idx), "the model takes one reached ray per pixel"
    t, pix = t[idx], pix[idx]
    il = rays["illumination"][:n][idx].astype(np.float64)
    th = row[idx, :3].astype(np.float64)
    if form == TERRAIN:                            # :577-590 have no throughput
        th = col["throughput"][pix].astype(np.float64) if mut == "throughput applied in the terrain form" else None
    lum = unpack_rgbe(rays["LuminanceIncomming"][:n][idx].view(np.uint32))
    pos = (t > 0) if mut == "t > 0 for t >= 0" else (t >= 0)
    neg = ~pos
    dw = col["Data"][pix, 3]
    ilth = F(il) if th is None else F(il).mul(th)
    n_ilth = 0 if th is None else 1

    def term(sel, with_k):
        a = F(ilth.v[sel], ilth.e[sel])
        return a.mul(lum[sel]).v if with_k else a.v

    sums = {}
    e = Expect(idx, sums, np.zeros(0, np.int64), [], np.zeros(0, np.int64), None, mut)
    # --- CacheBuffer.CurrentIlluminance, :464 / :577
    if rc and cache is not None and form != LEGACY:
        use_k = neg if restir else np.zeros(len(idx), bool)
        if mut == "k applied without ReSTIR GI":
            use_k = neg
        d = decode_rgb(cache["CurrentIlluminance"][pix], mut)
        s = []
        for c in range(3):
            a = F(ilth.v[:, c], ilth.e[:, c])
            ak = a.mul(lum[:, c])
            a = F(np.where(use_k, ak.v, a.v), np.where(use_k, ak.e, a.e))
            s.append(d[c].add(a))
        e.ci_pix, e.ci = pix, encode_fields(s, mut)
    # --- GlobalColors, :466-482 / :579-591
    if bounce == 0:
        sel = pos
        x, b = _sum(col["Direct"][pix[sel]].astype(np.float64), term(sel, False), n_ilth + 1)
        sums["Direct"] = Sum(pix[sel], x, b)
    if form == LEGACY:
        return e
    ind_plain = pos & (bounce != 0) & (not rc)                                      # :472 / :585
    if form == TERRAIN:
        ind_neg, k_neg = neg & (bounce != 0 or mut == "Indirect at bounce 0") & restir, False   # :589
    else:
        own, other = (float(bounce), -1.0)
        if mut == "Data.w tests swapped":
            own, other = other, own
        nz = bounce != 0 or mut == "Indirect at bounce 0"
        if rc:
            ind_neg, k_neg = neg & nz & (restir | (dw == own)), restir               # :477
        else:
            ind_neg, k_neg = neg & nz & ((not restir) & (dw == other)), False        # :479
    xs, bs, ps = [], [], []
    for sel, with_k in ((ind_plain, False), (ind_neg, k_neg)):
        x, b = _sum(col["Indirect"][pix[sel]].astype(np.float64), term(sel, with_k), n_ilth + 1 + int(with_k))
        xs.append(x), bs.append(b), ps.append(pix[sel])
    sums["Indirect"] = Sum(np.concatenate(ps), np.concatenate(xs), np.concatenate(bs))
    sel = neg & ~ind_neg                                                             # :481 / :590
    g1, g2 = GAMMA, 1.0 / GAMMA
    if mut == "gamma 2.0":
        g1, g2 = 2.0, 0.5
    if mut == "pow terms swapped":
        g1, g2 = g2, g1
    p = unpack_rgbe(col["PrimaryNEERay"][pix[sel]])
    o = []
    for c in range(3):
        a = fpow(F(p[:, c]), g1, U * g1 if mut == "pow terms swapped" else 0.0)
        b = fpow(F(il[sel, c]), g2, 0.0 if mut == "pow terms swapped" else U * g2)   # rcp(2.2f) is rounded
        if th is not None and mut != "throughput dropped from PrimaryNEERay":
            b = b.mul(th[sel, c])
        o.append(a.add(b))
    e.pnee_pix, e.pnee = pix[sel], o
    return e


# ------------------------------------------------------------------ comparison
@dataclasses.dataclass
class Report:
    fails: list
    ratios: dict            # float quantity -> worst actual error / bound
    two_valued: float       # share of the reached rays with a two-valued field
    reached: int
    text: str

    def names(self):
        return [f.split(":")[0] for f in self.fails]


CAP = 0.05
COL_FIELDS = {"Direct": 12, "Indirect": 12, "PrimaryNEERay": 4}


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def compare(e: Expect, col_in, col_out, cache_in=None, cache_out=None) -> Report:
    """col_out / cache_out: what the call left, pixels beyond W * H included."""
    fails, ratios = [], {}
    allowed_col = _raw(col_in).copy()       # the input with the fields a branch names taken from the output
    out_col = _raw(col_out)
    two = np.zeros(int(col_in.shape[0]), bool)
    for name, s in e.sums.items():
        off = col_in.dtype.fields[name][1]
        got = col_out[name][s.pix].astype(np.float64)
        with np.errstate(all="ignore"):
            r = np.abs(got - s.x) / s.bound
        r = np.where(np.isnan(r), np.where(got == s.x, 0.0, np.inf), r)
        ratios[name] = float(r.max()) if r.size else 0.0
        bad = np.nonzero((r > 1).any(1))[0]
        if len(bad):
            fails.append(f"{name}: {len(bad)} pixels beyond the bound, first pixel {int(s.pix[bad[0]])}, ratio {r[bad[0]].max():.3g}")
        allowed_col[s.pix, off:off + 12] = out_col[s.pix, off:off + 12]
    if len(e.pnee_pix):
        off = col_in.dtype.fields["PrimaryNEERay"][1]
        pc = pack_check(col_out["PrimaryNEERay"][e.pnee_pix], e.pnee, e.mut)
        ratios["PrimaryNEERay"] = float(pc.ratio.max())
        bad = np.nonzero(~pc.ok)[0]
        if len(bad):
            fails.append(f"PrimaryNEERay: {len(bad)} words break the packRGBE rule, first pixel {int(e.pnee_pix[bad[0]])}")
        two[e.pnee_pix] |= pc.two_valued
        allowed_col[e.pnee_pix, off:off + 4] = out_col[e.pnee_pix, off:off + 4]
    if not np.array_equal(allowed_col, out_col):
        where = np.nonzero((allowed_col != out_col).any(1))[0]
        fails.append(f"GlobalColors untouched: {len(where)} records differ outside the fields their ray's branch writes, "
                     f"first pixel {int(where[0])}")
    if cache_in is not None:
        allowed = _raw(cache_in).copy()
        out = _raw(cache_out)
        if e.ci is not None and len(e.ci_pix):
            off = cache_in.dtype.fields["CurrentIlluminance"][1]
            ok = e.ci.allows(cache_out["CurrentIlluminance"][e.ci_pix])
            bad = np.nonzero(~ok)[0]
            if len(bad):
                fails.append(f"CurrentIlluminance: {len(bad)} words outside the allowed fields, first pixel "
                             f"{int(e.ci_pix[bad[0]])}")
            two[e.ci_pix] |= e.ci.two_valued
            allowed[e.ci_pix, off:off + 4] = out[e.ci_pix, off:off + 4]
        if not np.array_equal(allowed, out):
            where = np.nonzero((allowed != out).any(1))[0]
            fails.append(f"CacheBuffer untouched: {len(where)} records differ outside CurrentIlluminance of a reached "
                         f"ray's pixel, first pixel {int(where[0])}")
    reached = len(e.reached)
    share = float(two.sum()) / max(reached, 1)
    if share > CAP:
        fails.append(f"sharpness cap: {share:.3%} of the reached rays have a two-valued field (cap {CAP:.0%})")
    text = (f"{reached} reached rays, two-valued {share:.2%}, worst error / bound "
            + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    return Report(fails, ratios, share, reached, text)
