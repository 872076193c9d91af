"""The float64 colour model (tests/colour.py) on the host: against the oracle's kernel_shadow outputs and the
terrain expectation on every case of tests/colour_cases.py, against the oracle's encoder entry points directly,
against every control mutant of the model, and against edited outputs. tests/test_gpu_colour.py runs the same
comparison on what the engine leaves."""
import functools

import numpy as np
import pytest

import colour as CM
import colour_cases as CC
import oracle_ctypes as O
import tthip

RC, RG = tthip.TT_SHADOW_RADIANCE_CACHE, tthip.TT_TRACE_USE_RESTIRGI


def case_of(kind, bounce, flags):
    if kind == "traced":
        return CC.traced(bounce, flags)
    if kind == "edge":
        return CC.edge_table(CM.ANY_HIT)
    if kind == "terrain set":
        return CC.terrain_set()
    return CC.edge_table(CM.TERRAIN)


@functools.lru_cache(maxsize=None)
def host(kind, bounce, flags):
    """What the host side leaves on a case, computed once (read-only)."""
    case = case_of(kind, bounce, flags)
    out = CC.host_run(case, bounce, flags)
    for a in out:
        a.setflags(write=False)
    return case, out


KINDS = ("traced", "edge", "terrain set", "terrain edge")


@pytest.mark.parametrize("bounce", [0, 1])
@pytest.mark.parametrize("flags", CC.FLAGS)
@pytest.mark.parametrize("kind", KINDS)
def test_model_matches_the_host_side(kind, bounce, flags):
    case, (vis, col, cache) = host(kind, bounce, flags)
    rep = CC.check(case, vis, col, cache, bounce, flags)
    print(f"{case.name} bounce {bounce} flags {flags:#x}: {rep.text}")
    assert not rep.fails, rep.fails
    live = case.rays["t"] != 0 if case.form == CM.TERRAIN else np.ones(len(case.rays), bool)
    if kind in ("edge", "terrain edge"):
        assert (vis[live] == 1).all(), "every ray of the edge table reaches its light with an all-ones row"
        assert rep.reached == int((live & (case.rays["PixelIndex"] < case.W * case.H)).sum())
    else:
        assert rep.reached > 200
    if kind == "traced":
        tinted = (vis[:, 3] == 1) & (vis[:, :3] != 1).any(1)
        assert tinted.sum() > 20, "tinted throughputs are present"
    if flags & RC:
        assert (cache["CurrentIlluminance"] != case.cache["CurrentIlluminance"]).sum() > 100
    else:
        assert np.array_equal(cache, case.cache)


@pytest.mark.parametrize("bounce", [0, 1])
def test_legacy_entry_contract_in_the_model(bounce):
    """tt_trace_shadow leaves Indirect, PrimaryNEERay and the cache to its caller: the model's legacy form names
    Direct at bounce 0 alone."""
    case = CC.traced(bounce, 0)
    vis, col, cache = CC.host_run(case, bounce, 0, legacy=True)
    rep = CC.check(case, vis, col, cache, bounce, 0, legacy=True)
    print(f"legacy bounce {bounce}: {rep.text}")
    assert not rep.fails, rep.fails
    full = host("traced", bounce, 0)[1]
    assert CC.check(case, full[0], full[1], full[2], bounce, 0, legacy=True).fails, "the full contract writes more"


@pytest.mark.parametrize("n", CC.LAUNCH_SIZES[:-1])
def test_edge_table_launch_sizes(n):
    """Rays at index >= n write nothing, in both forms."""
    for form in (CM.ANY_HIT, CM.TERRAIN):
        case = CC.edge_table(form)
        vis, col, cache = CC.host_run(case, 1, RC | RG, n=n)
        rep = CC.check(case, vis, col, cache, 1, RC | RG, n=n)
        assert not rep.fails, rep.fails
        assert (vis[n:] == np.float32(-7.5)).all()


# ------------------------------------------------------------------ the encoder entry points, directly
def _sweep_words(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def test_unpack_rgbe_is_exact():
    rng = np.random.default_rng(31)
    words = np.concatenate([_sweep_words(rng, 3000), np.array([0, 0xFFFFFFFF, 0x07FFFFFF, 31 << 27, 1], np.uint32)])
    want = CM.unpack_rgbe(words)
    got = np.stack([O.unpack_rgbe(int(w)) for w in words]).astype(np.float64)
    assert np.array_equal(got, want)


def test_pack_rgbe_is_exact_on_exact_inputs():
    """floor(log2 max), the power-of-two scale and round-half-to-even leave no freedom on a float32 input."""
    rng = np.random.default_rng(32)
    v = (rng.uniform(0, 1, (4000, 3)) * 10.0 ** rng.uniform(-8, 5, (4000, 1))).astype(np.float32)
    v[::5, 1] = 0.0
    halves = []  # exact half-integer mantissas, a maximum just under a power of two, the two clamps of the exponent
    for e in (-25, -20, -3, 0, 5, 11, 12, 15):
        for m in (0.5, 1.5, 2.5, 255.5, 510.5, 511.5):
            halves.append([2.0 ** e, m * 2.0 ** (e - 8), (m + 1) * 2.0 ** (e - 8)])
        halves.append([np.nextafter(np.float32(2.0 ** (e + 1)), np.float32(0)), 2.0 ** e, 0.0])
    v = np.concatenate([v, np.array(halves, np.float32)])
    want = CM.pack_rgbe_exact(v)
    got = np.array([O.pack_rgbe(x) for x in v], np.uint32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (v[bad[0]], hex(got[bad[0]]), hex(want[bad[0]]))
    for mut, needs in (("packRGBE truncates", True),):
        pc = CM.pack_check(got, [CM.F(v[:, c].astype(np.float64)) for c in range(3)], mut)
        assert (~pc.ok).any() == needs
    pc = CM.pack_check(got, [CM.F(v[:, c].astype(np.float64)) for c in range(3)])
    assert pc.ok.all() and pc.two_valued.mean() <= CM.CAP


def test_decode_rgb_within_the_derived_bound():
    rng = np.random.default_rng(33)
    words = np.concatenate([_sweep_words(rng, 6000), np.array([0, 1 << 18, 0xFFFFFFFF, (16383 << 18) | 511], np.uint32)])
    d = CM.decode_rgb(words)
    got = np.stack([O.decode_rgb(int(w)) for w in words]).astype(np.float64)
    worst = 0.0
    for c in range(3):
        with np.errstate(all="ignore"):
            r = np.where(d[c].e > 0, np.abs(got[:, c] - d[c].v) / np.where(d[c].e > 0, d[c].e, 1.0),
                         np.where(got[:, c] == d[c].v, 0.0, np.inf))
        worst = max(worst, float(r.max()))
    print(f"DecodeRGB: worst error / bound {worst:.3g} over {len(words)} words")
    assert worst <= 1
    # the bound is a float32 bound: a few ulps of the largest channel-row magnitude, nowhere near a field step
    Y = np.maximum.reduce([np.abs(x.v) for x in d])
    big = np.maximum.reduce([x.e for x in d])
    assert np.median(big[Y > 0] / Y[Y > 0]) < 64 * CM.U
    for mut in ("decode without + 0.5", "scale 819"):
        m = CM.decode_rgb(words, mut)
        assert max(float((np.abs(got[:, c] - m[c].v) > m[c].e).mean()) for c in range(3)) > 0.5, mut


def test_encode_rgb_fields_are_sharp():
    rng = np.random.default_rng(34)
    n = 6000
    v = (rng.uniform(0, 1, (n, 3)) * 10.0 ** rng.uniform(-7, 7, (n, 1))).astype(np.float32)
    v[::6, rng.integers(0, 3)] = 0.0
    v[1::6] *= np.eye(3, dtype=np.float32)[rng.integers(0, 3, len(v[1::6]))]   # pure channels
    got = np.array([O.encode_rgb(x) for x in v], np.uint32)
    f = CM.encode_fields([CM.F(v[:, c].astype(np.float64)) for c in range(3)])
    ok = f.allows(got)
    share = float(f.two_valued.mean())
    print(f"EncodeRGB: two-valued {share:.2%} of {n} exact inputs")
    assert ok.all(), (v[~ok][0], hex(got[~ok][0]))
    assert share <= CM.CAP
    assert (got >> 18 == 16383).any() and (got == 0).any()
    for mut in ("a Rec.601 luma row", "one transposed XYZ entry", "Le rounded, not truncated", "scale 819"):
        m = CM.encode_fields([CM.F(v[:, c].astype(np.float64)) for c in range(3)], mut)
        assert not m.allows(got).all(), mut


def test_pow_within_the_derived_bound():
    rng = np.random.default_rng(35)
    x = np.concatenate([10.0 ** rng.uniform(-6, 3, 3000), [1.0, 0.0, 2.0, 1e-6, 1e3]]).astype(np.float32)
    worst = 0.0
    for y, y_err in ((CM.GAMMA, 0.0), (float(np.float32(1.0) / np.float32(2.2)), 0.0)):
        p = CM.fpow(CM.F(x.astype(np.float64)), y, y_err)
        got = np.array([O.hlsl_pow(float(a), y) for a in x])
        r = np.where(p.e > 0, np.abs(got - p.v) / np.where(p.e > 0, p.e, 1.0), np.where(got == p.v, 0.0, np.inf))
        worst = max(worst, float(r.max()))
        assert (p.e <= 3 * (1 + CM.LN2 * np.abs(y * np.log2(np.where(x > 0, x, 1)))) * CM.U * np.maximum(p.v, 1e-300) * 1.01).all()
    print(f"pow: worst error / bound {worst:.3g}")
    assert worst <= 1


# ------------------------------------------------------------------ control mutants and edited outputs
MUTANT_CASES = [("traced", 1, 0), ("traced", 1, RC), ("traced", 0, RC | RG), ("traced", 0, 0), ("edge", 1, 0),
                ("edge", 0, RC), ("terrain set", 1, RC), ("terrain set", 0, RG)]


def test_every_mutant_is_reported():
    """Each one-line edit of the model disagrees, by name, with what the host side leaves on at least one case."""
    found = {}
    for mut in CM.MUTANTS:
        for kind, bounce, flags in MUTANT_CASES:
            case, (vis, col, cache) = host(kind, bounce, flags)
            names = CC.check(case, vis, col, cache, bounce, flags, mut=mut).names()
            names = [x for x in names if x != "sharpness cap"]
            if names:
                found[mut] = (case.name, bounce, flags, sorted(set(names)))
                break
    for mut in CM.MUTANTS:
        print(f"mutant '{mut}': {found.get(mut, 'NOT REPORTED')}")
    assert set(found) == set(CM.MUTANTS), sorted(set(CM.MUTANTS) - set(found))


def test_edited_outputs_are_reported():
    kind, bounce, flags = "traced", 1, RC
    case, (vis, col, cache) = host(kind, bounce, flags)
    assert not CC.check(case, vis, col, cache, bounce, flags).fails
    e = CM.expect(case.form, case.rays, vis, case.col, case.cache, bounce, flags, case.W, case.H, len(case.rays))
    # one Norm word changed
    c2 = cache.copy()
    c2["Norm"][int(e.ci_pix[3])] ^= 1
    assert "CacheBuffer untouched" in CC.check(case, vis, col, c2, bounce, flags).names()
    # one pixel beyond W * H written
    k2 = col.copy()
    k2["Indirect"][case.W * case.H + 1, 2] += 1.0
    assert "GlobalColors untouched" in CC.check(case, vis, k2, cache, bounce, flags).names()
    c3 = cache.copy()
    c3["CurrentIlluminance"][case.W * case.H] += 1 << 18
    assert "CacheBuffer untouched" in CC.check(case, vis, col, c3, bounce, flags).names()
    # one Le off by one on a one-valued field
    j = int(np.nonzero(~e.ci.two_valued & (e.ci.lo[:, 0] > 1) & (e.ci.hi[:, 0] < 16383))[0][0])
    for d in (1, -1):
        c4 = cache.copy()
        c4["CurrentIlluminance"][int(e.ci_pix[j])] = int(cache["CurrentIlluminance"][int(e.ci_pix[j])]) + d * (1 << 18)
        assert "CurrentIlluminance" in CC.check(case, vis, col, c4, bounce, flags).names()
    # one mantissa step of a PrimaryNEERay word, one ulp too many on an Indirect
    kind, bounce, flags = "traced", 1, 0
    case, (vis, col, cache) = host(kind, bounce, flags)
    e = CM.expect(case.form, case.rays, vis, case.col, case.cache, bounce, flags, case.W, case.H, len(case.rays))
    pc = CM.pack_check(col["PrimaryNEERay"][e.pnee_pix], e.pnee)
    j = int(np.nonzero(~pc.two_valued & ((col["PrimaryNEERay"][e.pnee_pix] & 0x1FF) % 511 > 1))[0][0])
    k5 = col.copy()
    k5["PrimaryNEERay"][int(e.pnee_pix[j])] += 1
    assert "PrimaryNEERay" in CC.check(case, vis, k5, cache, bounce, flags).names()
    s = e.sums["Indirect"]
    k6 = col.copy()
    p = int(s.pix[0])
    k6["Indirect"][p, 0] = np.nextafter(np.nextafter(np.nextafter(col["Indirect"][p, 0], np.float32(9)), np.float32(9)), np.float32(9))
    assert "Indirect" in CC.check(case, vis, k6, cache, bounce, flags).names()


# ------------------------------------------------------------------ the two pinned edges
@pytest.mark.parametrize("form", [CM.ANY_HIT, CM.TERRAIN])
def test_non_finite_and_negative_illumination_words(form):
    case = CC.pinned_edges(form)
    CC.check_pinned(case, *CC.host_run(case, 0, RC))


def test_pack_rgbe_below_2_to_minus_119():
    """pow(2, -exponent) * 256 overflows to infinity for a maximum below 2^-119 (:489): the maximum times inf is inf,
    a zero channel times inf is NaN, and min(511, .) makes both 511. Kept as the text has it;
    :481 and :590 cannot reach it (a non-zero pow term of a float32 is above 2^-69)."""
    assert O.pack_rgbe([2.0 ** -126, 0.0, 0.0]) == 0x07FFFFFF
    assert O.pack_rgbe([1.5 * 2.0 ** -120, 0.0, 2.0 ** -121]) == 0x07FFFFFF
    assert O.pack_rgbe([2.0 ** -119, 0.0, 2.0 ** -121]) == 256 | (64 << 18)   # the first maximum with a finite scale
    # and the other end: an infinite maximum has floor(log2) = inf, field 31, scale 0 (:485-490)
    assert O.pack_rgbe([float("inf"), 1.0, 1.0]) == (31 << 27) | 511
    assert O.pack_rgbe([1.0, float("inf"), float("inf")]) == (31 << 27) | (511 << 9) | (511 << 18)
    big = np.array([3e38, 1.5e38, 0.0], np.float32)
    assert O.pack_rgbe(big) == int(CM.pack_rgbe_exact(big)) and O.pack_rgbe(big) >> 27 == 31
