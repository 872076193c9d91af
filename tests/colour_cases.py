"""Inputs of the float64 colour pin (tests/colour.py), shared by tests/test_colour_host.py (the oracle and the
terrain expectation) and tests/test_gpu_colour.py (the engine): one ray per pixel, small screens.

  * traced(bounce, flags): the 96 x 64 glass-soup NEE rays of test_gpu_parity.test_shadow_accumulations_match_oracle
    with its seeds and its random initial colours and packed words (tinted throughputs are present), plus random
    bytes in every field no branch writes and PAD records beyond W * H.
  * edge_table(form): 4,095 crafted rays on a 64 x 64 screen that start outside the scene's bounds and point away, so
    every visibility row is (1, 1, 1, 1) and the outputs are a pure function of the inputs. Value classes x the sign
    of t x Data.w in {-1, 0, 1, 5}, then rows with t = -0.0 / +0.0 and PixelIndex W*H - 1, W*H and 2^32 - 1. The
    rows are shuffled, so the head of the table (launches of 1, 255, 256, 257 rays) holds every kind.
  * terrain_set(): tests/terrain_cases.py's 4,096 shadow rays with the same kind of random records.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import colour as CM
import tthip

PAD = 8                     # records beyond W * H: a write there is a write out of the screen
EW = EH = 64                # the edge table's screen
N_EDGE = 4095
LAUNCH_SIZES = (1, 255, 256, 257, 4095)
FLAGS = (tthip.TT_SHADOW_RADIANCE_CACHE, tthip.TT_SHADOW_RADIANCE_CACHE | tthip.TT_TRACE_USE_RESTIRGI, 0,
         tthip.TT_TRACE_USE_RESTIRGI)
assert CM.RADIANCE_CACHE == tthip.TT_SHADOW_RADIANCE_CACHE and CM.RESTIRGI == tthip.TT_TRACE_USE_RESTIRGI


@dataclasses.dataclass
class Case:
    name: str
    form: str               # colour.ANY_HIT or colour.TERRAIN
    scene: object           # the triangle scene (any-hit), None for the terrain set of tests/terrain_cases.py
    rays: np.ndarray        # SHADOW_DTYPE
    col: np.ndarray         # COL_DTYPE, W * H + PAD records
    cache: np.ndarray       # CACHE_DTYPE, W * H + PAD records
    W: int
    H: int

    def __post_init__(self):
        for a in (self.rays, self.col, self.cache):
            a.setflags(write=False)


def _noise(col, cache, rng):
    """Random bytes in the fields no branch of either kernel writes."""
    n = len(col)
    col["throughput"] = rng.uniform(0.1, 0.9, (n, 3))
    col["Flags"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    col["MetRoughIsSpec"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    col["Data"][:, :3] = rng.uniform(-4, 4, (n, 3))
    for f in ("samples", "throughput", "pathLength", "Norm"):
        cache[f] = rng.integers(0, 1 << 32, cache[f].shape, dtype=np.uint64).astype(np.uint32)


# ------------------------------------------------------------------ the traced case
@functools.lru_cache(maxsize=None)
def traced(bounce: int, flags: int) -> Case:
    import handbuilt as hb
    import oracle_ctypes as O
    from parity_util import FAR
    from test_gpu_parity import glass_soup

    seed = 70 + bounce * 4 + flags % 7
    sc = glass_soup(seed)
    W, H = 96, 64
    c2w, ip = tthip.unity_camera((0.3, 0.2, 3.0), (0, 0, -1), (0, 1, 0), 50.0, W, H, 0.05, FAR)
    rays = O.generate(c2w, ip, W, H, 0.05, FAR)
    O.trace(sc, rays, W * H, 0, FAR, W, H)
    rng = np.random.default_rng(seed)
    sr = hb.nee_rays_from_hits(rays, W * H, (0.5, 2.0, 2.5), seed)
    sr["illumination"] *= rng.uniform(0.1, 30.0, (len(sr), 1)).astype(np.float32)
    lum = (rng.integers(14, 26, len(sr)).astype(np.uint32) << 27) | rng.integers(0, 1 << 27, len(sr)).astype(np.uint32)
    sr["LuminanceIncomming"] = lum.view(np.float32)
    col = np.zeros(W * H + PAD, tthip.COL_DTYPE)
    cache = np.zeros(W * H + PAD, tthip.CACHE_DTYPE)
    c, h = col[: W * H], cache[: W * H]
    c["Direct"] = rng.uniform(0, 2, (W * H, 3))
    c["Indirect"] = rng.uniform(0, 2, (W * H, 3))
    c["PrimaryNEERay"] = (rng.integers(12, 24, W * H).astype(np.uint32) << 27) | \
        rng.integers(0, 1 << 27, W * H).astype(np.uint32)
    c["Data"][:, 3] = rng.choice(np.array([-1.0, float(bounce), 5.0], np.float32), W * H)
    h["CurrentIlluminance"] = rng.integers(0, 1 << 32, W * H, dtype=np.uint64).astype(np.uint32)
    h["CurrentIlluminance"][::7] = 0
    dw = col["Data"][:, 3].copy()
    _noise(col, cache, np.random.default_rng(seed + 1000))
    col["Data"][:, 3] = dw
    return Case(f"traced bounce {bounce} flags {flags:#x}", CM.ANY_HIT, sc, sr, col, cache, W, H)


# ------------------------------------------------------------------ the edge table
def _rgbe(e, r, g, b):
    return (int(e) << 27) | int(r) | (int(g) << 9) | (int(b) << 18)


def _logluv(Le, ue, ve):
    return (int(Le) << 18) | (int(ue) << 9) | int(ve)


ONE_RGBE = _rgbe(20, 256, 256, 256)            # unpacks to (1, 1, 1)
Y_ROW_SUM = float(sum(CM.RGB2XYZ[1]))
STRADDLE = (1 - 2.0 ** -22, 1 + 2.0 ** -22, 1 - 2.0 ** -12, 1 + 2.0 ** -12, 1 - 2.0 ** -6, 1 + 2.0 ** -6, 0.5, 2.0)


def _classes(rng):
    """Value classes: dicts of il (3), old (CurrentIlluminance), P (PrimaryNEERay), lum (LuminanceIncomming),
    direct (3), indirect (3). Unset entries are drawn at random ('generic')."""
    generic = lambda: _generic_pad(rng)  # noqa: E731

    def make(**kw):
        d = generic()
        d.update(kw)
        return d

    out = []
    for mask in range(1, 8):                                        # illumination 0 in one, two and three channels
        for _ in range(6):
            d = generic()
            d["il"] = d["il"] * [(mask >> k) & 1 ^ 1 for k in range(3)]
            out.append(d)
    for ch in range(3):                                             # a single pure channel (blue: Y is 0.07 of the max)
        for mag in (1e-3, 0.05, 1.0, 30.0, 2e4):
            il = np.zeros(3)
            il[ch] = mag * rng.uniform(1, 2)
            out.append(make(il=il, old=0, direct=np.zeros(3), indirect=np.zeros(3)))
            out.append(make(il=il))
    # sums straddling Le 0 | 1 and Le 16382 | 16383 (:1578-1580), and Y = 2^-20, 2^20, with old == 0: s = il
    for target in (2.0 ** (-20 + 1 / CM.L_SCALE), 2.0 ** (16383 / CM.L_SCALE - 20), 2.0 ** -20, 2.0 ** 20):
        for f in STRADDLE:
            out.append(make(il=np.full(3, target * f / Y_ROW_SUM), old=0))
    for ue, ve in ((0, 0), (511, 0), (0, 511), (511, 511), (511, 300), (300, 511)):   # decoded chroma at its clamps
        for Le in (1, 4000, 8192, 12000, 16383):
            out.append(make(old=_logluv(Le, ue, ve)))
    for _ in range(16):
        out.append(make(old=0))
    for pe in (0, 31):                                              # exponent fields 0 and 31 of both packed inputs
        for le in (0, 31):
            for j in range(8):
                d = make(P=_rgbe(pe, *rng.integers(1, 512, 3)), lum=_rgbe(le, *rng.integers(1, 512, 3)))
                if j % 4 == 0:
                    d["il"] = np.zeros(3)                           # o = pow(unpack(P), 2.2) alone: below 2^-20 for pe == 0
                if le == 31:
                    d["il"] = d["il"] * 1e-3
                out.append(d)
    for target in (2.0 ** -20, 4096.0, 1.0, 2.0):                   # packRGBE sums straddling 2^-20, 4096, powers of two
        for f in STRADDLE:
            g = (target * f) ** CM.GAMMA
            out.append(make(il=np.array([g, g * 0.3, g * 0.01]), P=0))
    for P in (0, ONE_RGBE, _rgbe(20, 256, 0, 256)):                 # o in {0, 1, 2}: pow(1, y) = 1 and pow(0, y) = 0 exactly
        for il in ((0, 0, 0), (1, 1, 1), (1, 0, 1)):
            out.append(make(il=np.array(il, np.float64), P=P))
    for j in range(1, 9):                                           # a maximum just under a power of two
        out.append(make(il=np.full(3, 1.0 - j * 2.0 ** -24), P=0))
    return out


@functools.lru_cache(maxsize=None)
def edge_table(form: str) -> Case:
    """form: colour.ANY_HIT (rays outside the glass soup's bounds, with that scene) or colour.TERRAIN (rays above the
    terrain boxes of tests/terrain_cases.py, pointing up)."""
    rng = np.random.default_rng(0xC0104)
    cls = _classes(rng)
    n_cls = 500
    while len(cls) < n_cls:
        cls.append(_generic_pad(rng))
    assert len(cls) == n_cls
    rows = []
    for d in cls:
        for t in (1.0, -1.0):
            for dw in (-1.0, 0.0, 1.0, 5.0):
                rows.append((d, t, dw, None))
    gen = lambda: _generic_pad(rng)  # noqa: E731
    for _ in range(40):
        rows.append((gen(), -0.0, float(rng.choice([-1.0, 0.0, 1.0, 5.0])), None))   # t >= 0 holds for -0.0
    for _ in range(40):
        rows.append((gen(), 0.0, float(rng.choice([-1.0, 0.0, 1.0, 5.0])), None))    # the terrain form skips t == 0
    for k in range(15):
        rows.append((gen(), 1.0 if k % 2 else -1.0, 1.0, (EW * EH - 1, EW * EH, 0xFFFFFFFF)[k % 3] if k else EW * EH - 1))
    assert len(rows) == N_EDGE
    order = rng.permutation(N_EDGE)
    rows = [rows[i] for i in order]
    free = iter(rng.permutation(EW * EH - 1))      # pixel W*H - 1 belongs to one of the special rows
    n_pix = EW * EH + PAD
    s = np.zeros(N_EDGE, tthip.SHADOW_DTYPE)
    col, cache = np.zeros(n_pix, tthip.COL_DTYPE), np.zeros(n_pix, tthip.CACHE_DTYPE)
    _noise(col, cache, rng)
    col["Direct"] = rng.uniform(0, 2, (n_pix, 3))
    col["Indirect"] = rng.uniform(0, 2, (n_pix, 3))
    col["PrimaryNEERay"] = [_rgbe(rng.integers(12, 24), *rng.integers(0, 512, 3)) for _ in range(n_pix)]
    col["Data"][:, 3] = 1.0
    cache["CurrentIlluminance"] = [_logluv(rng.integers(5000, 11000), rng.integers(60, 360), rng.integers(60, 460))
                                   for _ in range(n_pix)]
    last_used = False
    for i, (d, t, dw, special) in enumerate(rows):
        pix = next(free) if special is None else special
        if special == EW * EH - 1:
            if last_used:
                pix = next(free)
            last_used = True
        s["PixelIndex"][i] = pix
        s["t"][i] = t
        s["illumination"][i] = d["il"]
        s["LuminanceIncomming"][i] = np.uint32(d["lum"]).view(np.float32)
        if pix < EW * EH:
            col["Direct"][pix], col["Indirect"][pix] = d["direct"], d["indirect"]
            col["PrimaryNEERay"][pix], col["Data"][pix, 3] = d["P"], dw
            cache["CurrentIlluminance"][pix] = d["old"]
    u = rng.uniform(0, 1, (N_EDGE, 3))
    if form == CM.ANY_HIT:
        from test_gpu_parity import glass_soup

        scene = glass_soup(70)
        d = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0) + 0.2 * (u - 0.5)
        s["origin"] = 5.0 + 2.0 * u
    else:
        scene = None
        d = np.array([0.0, 1.0, 0.0]) + 0.2 * (u - 0.5)
        s["origin"] = np.array([-3.9, 20.0, -3.9]) + u * np.array([9.8, 2.0, 7.8])
    s["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return Case(f"edge table ({form})", form, scene, s, col, cache, EW, EH)


def _generic_pad(rng):
    return dict(il=rng.uniform(0.05, 4.0, 3) * 10.0 ** rng.uniform(-2, 1.5),
                old=_logluv(rng.integers(5000, 11000), rng.integers(60, 360), rng.integers(60, 460)),
                P=_rgbe(rng.integers(12, 24), *rng.integers(0, 512, 3)),
                lum=_rgbe(rng.integers(14, 26), *rng.integers(0, 512, 3)),
                direct=rng.uniform(0, 2, 3), indirect=rng.uniform(0, 2, 3))


# ------------------------------------------------------------------ the terrain set
@functools.lru_cache(maxsize=None)
def terrain_set() -> Case:
    import terrain_cases as TC

    rng = np.random.default_rng(0xC0105)
    n_pix = TC.SW * TC.SH + PAD
    col, cache = np.zeros(n_pix, tthip.COL_DTYPE), np.zeros(n_pix, tthip.CACHE_DTYPE)
    _noise(col, cache, rng)
    col["Direct"] = rng.uniform(0, 2, (n_pix, 3))
    col["Indirect"] = rng.uniform(0, 2, (n_pix, 3))
    col["PrimaryNEERay"] = (rng.integers(12, 24, n_pix).astype(np.uint32) << 27) | rng.integers(0, 1 << 27, n_pix).astype(np.uint32)
    col["Data"][:, 3] = rng.choice(np.array([-1.0, 0.0, 1.0, 5.0], np.float32), n_pix)
    cache["CurrentIlluminance"] = rng.integers(0, 1 << 32, n_pix, dtype=np.uint64).astype(np.uint32)
    cache["CurrentIlluminance"][::7] = 0
    s = TC.shadow_rays().copy()
    lum = (rng.integers(14, 26, len(s)).astype(np.uint32) << 27) | rng.integers(0, 1 << 27, len(s)).astype(np.uint32)
    s["LuminanceIncomming"] = lum.view(np.float32)   # (the set's own words reach exponent fields the any-hit set has not)
    return Case("terrain set", CM.TERRAIN, None, s, col, cache, TC.SW, TC.SH)


# ------------------------------------------------------------------ the host side of each case
def host_run(case: Case, bounce: int, flags: int, n=None, legacy=False):
    """What the oracle (any-hit) or the terrain expectation of tests/test_gpu_terrain.py leaves: (vis, col, cache)."""
    n = len(case.rays) if n is None else n
    col, cache = case.col.copy(), case.cache.copy()
    vis = np.full((len(case.rays), 4), -7.5, np.float32)
    if case.form == CM.ANY_HIT:
        import oracle_ctypes as O
        from parity_util import CPU_THREADS

        r = case.rays.copy()
        st, _ = O.shadow(case.scene, r, n, bounce, case.W, case.H, visibility=vis, colors=col,
                         cache=None if legacy else cache, flags=0 if legacy else flags, nthreads=CPU_THREADS)
        assert st == 0
        if legacy:  # tt_trace_shadow's contract is the oracle's Direct alone (test_legacy_shadow_entry_contract)
            keep = case.col.copy()
            keep["Direct"] = col["Direct"]
            col = keep
        return vis, col, cache
    import terrain_cases as TC
    import test_gpu_terrain as TG

    # the expectation has no screen: rays whose pixel lies outside it (dropped writes) are handed over as skipped
    s = case.rays.copy()
    outside = s["PixelIndex"] >= case.W * case.H
    s["t"][outside] = 0.0
    occ, _ = tthip.terrain_occluded_host(TC.terrains(), TC.atlas(), case.rays.copy(), len(s))
    saved = TG._SHADOW_IN
    try:
        TG._SHADOW_IN = (col, cache, np.zeros((len(col), 4), np.float32), vis)
        col, cache, _, vis = TG.shadow_expected(s, occ, bounce, bool(flags & tthip.TT_SHADOW_RADIANCE_CACHE),
                                                bool(flags & tthip.TT_TRACE_USE_RESTIRGI), n=n)
    finally:
        TG._SHADOW_IN = saved
    live = outside & (case.rays["t"] != 0) & (np.arange(len(s)) < n)
    vis[live] = np.where(occ[live, None] == 1, np.float32(0), np.float32(1))
    return vis, col, cache


def check(case: Case, vis, col, cache, bounce, flags, n=None, legacy=False, mut=None) -> CM.Report:
    n = len(case.rays) if n is None else n
    form = CM.LEGACY if legacy else case.form
    e = CM.expect(form, case.rays, vis, case.col, case.cache, bounce, flags, case.W, case.H, n, mut)
    return CM.compare(e, case.col, col, case.cache, cache)


# ------------------------------------------------------------------ pinned edges outside the float64 comparison
INF, NAN = float("inf"), float("nan")
# (illumination, CurrentIlluminance word, PrimaryNEERay word) at bounce 0 with the RadianceCache define, old == 0 and
# PrimaryNEERay == 0, so s = o = the illumination terms alone. By the text and D3D's rules:
#   +inf: Y = inf, Le = 16383, 1 / (-2 inf + 12 inf + ...) is NaN and clamp(NaN) is 0: (16383 << 18);
#         floor(log2 inf) = inf, the field clamps to 31, the scale pow(2, -inf) * 256 is 0, inf * 0 is NaN and
#         min(511, NaN) is 511, the finite channels times 0 are 0: (31 << 27) | 511
#   NaN, -inf, a negative Y: log2 is NaN, clamp(NaN) is 0, Le == 0 returns the word 0; pow of a negative or NaN
#         channel is NaN, max(0, NaN) is 0: that channel packs as 0 beside pow(1, y) = 1 -> 256 at exponent 0
PINNED = (((INF, 1.0, 1.0), 16383 << 18, (31 << 27) | 511),
          ((NAN, 1.0, 1.0), 0, _rgbe(20, 0, 256, 256)),
          ((-INF, 1.0, 1.0), 0, _rgbe(20, 0, 256, 256)),
          ((-5.0, 1.0, 0.0), 0, _rgbe(20, 0, 256, 0)))
PINNED_DIRECT = (0.5, 0.25, 0.125)


@functools.lru_cache(maxsize=None)
def pinned_edges(form: str) -> Case:
    """2 x len(PINNED) rays of the edge table's kind: rows [0, k) have t = -1 (CurrentIlluminance and PrimaryNEERay),
    rows [k, 2k) t = +1 (CurrentIlluminance and Direct). Run at bounce 0 with TT_SHADOW_RADIANCE_CACHE."""
    base = edge_table(form)
    k = len(PINNED)
    s = base.rays[: 2 * k].copy()
    s["PixelIndex"] = np.arange(2 * k)
    s["t"] = [-1.0] * k + [1.0] * k
    s["illumination"] = [p[0] for p in PINNED] * 2
    col, cache = base.col.copy(), base.cache.copy()
    col["PrimaryNEERay"][: 2 * k] = 0
    col["Direct"][: 2 * k] = PINNED_DIRECT
    cache["CurrentIlluminance"][: 2 * k] = 0
    return Case(f"pinned edges ({form})", form, base.scene, s, col, cache, EW, EH)


def check_pinned(case: Case, vis, col, cache):
    """The words exactly; Direct is the one IEEE add of the text (inf, -inf and NaN propagate); nothing else moves."""
    k = len(PINNED)
    assert (vis[: 2 * k] == 1).all()
    want_ci = np.array([p[1] for p in PINNED] * 2, np.uint32)
    assert cache["CurrentIlluminance"][: 2 * k].tolist() == want_ci.tolist()
    assert col["PrimaryNEERay"][:k].tolist() == [p[2] for p in PINNED]
    with np.errstate(invalid="ignore"):
        want_d = np.float32(PINNED_DIRECT) + case.rays["illumination"][k:]
    got_d = col["Direct"][k: 2 * k]
    assert np.array_equal(np.isnan(got_d), np.isnan(want_d)) and np.array_equal(got_d[~np.isnan(want_d)], want_d[~np.isnan(want_d)])
    keep_col, keep_cache = case.col.copy(), case.cache.copy()
    keep_col["PrimaryNEERay"][:k] = col["PrimaryNEERay"][:k]
    keep_col["Direct"][k: 2 * k] = col["Direct"][k: 2 * k]
    keep_cache["CurrentIlluminance"][: 2 * k] = cache["CurrentIlluminance"][: 2 * k]
    assert np.array_equal(_bytes(keep_col), _bytes(col)) and np.array_equal(_bytes(keep_cache), _bytes(cache))


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)
