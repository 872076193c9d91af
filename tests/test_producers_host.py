"""The float64 producer model (tests/producers.py) against the oracle's Generate, normal resolve and bounce enqueue on
every case of tests/producers_cases.py, against every control mutant, and against itself where the answer is known in
closed form. CPU only; tests/test_gpu_producers.py runs the same comparisons on the kernels.

Worst values of the oracle, as fractions of the derived bounds (pytest -s prints them):
  Generate, 40 cases                  direction 0.10, origin 0.33 (the far camera's coordinates near 500)
  resolve                             smooth normal 0.09 (5.2e-7 absolute), unsmoothed 0.05 against the restated chain
                                      and against the world triangle, smooth against the analytic ellipsoid 0.72
  bounce                              |direction| - 1 0.63, last_pdf pi - omega_o.y 0.39, direction . norm - last_pdf pi
                                      0.13, direction . norm - disc sample 0.11, pair angle 0.05, origin offset 0.91
  KS at alpha = 0.001                 jitter x 0.46 and y 0.59 of the limit (4,160 pixels); cos^2 0.37 and azimuth 0.52
                                      (6,852 survivors)
  coverage (synthetic set)            |norm.x| > 0.99: 355, [0.95, 0.99): 594, flipped 3,466, unflipped 3,386, mirrored
                                      1,747, far 1,797; rays with two candidate norm codes 2,897 of 6,900
  left open                           0 rays in every case, beside the 48 in-plane rays and the one pdf = 0 ray of the
                                      synthetic set that are marginal by construction
  the model against itself            restated against analytic on 8,000 records: inside the bound on all four parents
"""
import numpy as np
import pytest

import oracle_ctypes as O
import producers as P
import producers_cases as PC
import tthip

FAR = PC.FAR


class OracleSide:
    def generate(self, c2w, ip, W, H, near, far, jitter, frames, max_bounce):
        return O.generate(c2w, ip, W, H, near, far, jitter, frames, max_bounce)

    def trace(self, sc, buf, n, bounce, W, H):
        st, _ = O.trace(sc, buf, n, bounce, FAR, W, H)
        assert st == 0

    def resolve(self, sc, buf, n, bounce, W, H):
        return O.resolve_normals(sc, buf, n, bounce, FAR, W, H)

    def enqueue(self, sc, buf, n, bounce, W, H, frames, max_bounce, frame_pixels):
        if not frame_pixels:
            return O.enqueue_bounce(sc, buf, n, bounce, FAR, W, H, frames, max_bounce)
        # the oracle keys on the pixel as given: frame j alone, on its frame-local pixels, at frames + j
        wh, fp = W * H, frame_pixels
        off, dst = (wh, 0) if bounce % 2 else (0, wh)
        src = buf[off:off + n].copy()
        total = 0
        for j in np.unique(src["PixelIndex"] // fp):
            sub = src[src["PixelIndex"] // fp == j]
            tmp = np.zeros(2 * fp, tthip.RAY_DTYPE)
            tmp[:len(sub)] = sub
            tmp["PixelIndex"][:len(sub)] -= j * fp
            fr = (frames + int(j) + 2 ** 31) % 2 ** 32 - 2 ** 31
            k = O.enqueue_bounce(sc, tmp, len(sub), 0, FAR, fp, 1, fr, max_bounce)
            rows = tmp[fp:fp + k]
            rows["PixelIndex"] += j * fp
            buf[dst + total:dst + total + k] = rows
            total += k
        return total


SIDE = OracleSide()


# ------------------------------------------------------------------ the model against closed forms
def test_random_numbers_are_uniform_and_keyed_on_the_frame_local_pixel():
    p = np.arange(40000)
    rx, ry = P.random2(1, p, 3, 5, 0)
    assert rx.dtype == np.float32 and (rx >= 0).all() and (rx < 1).all()
    for x in (rx, ry):
        assert P.ks_statistic(x) < P.ks_limit(len(p))
    a = P.random2(1, p + 40000, 7, 5, 1, frame_pixels=40000)
    b = P.random2(1, p, 8, 5, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    w = P.random2(0, p[:8], 0x7FFFFFFF, 1, 0)   # frames + 0xdeadbeef wraps
    assert np.isfinite(w[1]).all()
    assert P.ks_statistic(np.linspace(0, 1, 1001)[1:] ** 2) > 0.2   # the statistic can fail


def test_model_generate_equals_the_matrix_path():
    """The parametric model against Generate through camera_matrices in float64: the helper and the model agree to
    float32 rounding of the output, far inside the bound."""
    for cn, W, H, jit, fr, mb in PC.generate_cases():
        cam = PC.CAMERAS[cn]
        c2w, ip = PC.camera_matrices(cam, W, H)
        rays = PC.rays_from_matrices(c2w, ip, W, H, cam.near, cam.far, jit, fr, mb)
        rep = PC.compare_generate(cam, W, H, jit, fr, mb, rays)
        rep.check()
        assert rep.worst["direction"] < 0.1 and rep.worst["origin"] < 0.5
    c2w, ip = PC.camera_matrices(PC.CAMERAS["axis"], 64, 36)
    u2w, uip = tthip.unity_camera((0, 0, -5), (0, 0, 1), (0, 1, 0), 60.0, 64, 36, PC.NEAR, FAR)
    assert np.allclose(c2w, u2w) and np.allclose(ip, uip)


PLANE_N = np.ones(3) / np.sqrt(3.0)


def _plane_scene(M):
    """One triangle in the plane x + y + z = 0 with normals (1, 1, 1) / sqrt(3) under L2W = M, as raw arrays (a
    normal along an axis of the scale would not separate the inverse transpose from L2W)."""
    tris = np.zeros(1, tthip.TRI_DTYPE)
    tris["pos0"], tris["posedge1"], tris["posedge2"] = (-1, 1, 0), (3, -3, 0), (0, 3, -3)
    fx, fy = P.oct_encode_pre(PLANE_N[None, :])
    tris["norms"][:] = np.uint32(np.rint(fx[0])) | (np.uint32(np.rint(fy[0])) << 16)
    md = np.zeros(1, tthip.MESH_DTYPE)
    md["W2L"][0] = tthip.unity_colmajor(np.linalg.inv(M))
    return tris, md


@pytest.mark.parametrize("mirror", (1.0, -1.0))
def test_model_on_a_plane(mirror):
    """A plane under a skew rotation with a non-uniform (and a mirrored) scale: the world normal is
    normalize(M^-T n) in closed form; the restated, the geometric and the closed form agree, and the bounce
    model puts the origin 1e-4 above the plane on the ray's side."""
    M = PC.trs((0.3, -0.2, 0.5), PC.rotation((1, 2, 3), 40.0), (3.0 * mirror, 1.0, 0.5))
    tris, md = _plane_scene(M)
    want = P._unit(np.linalg.inv(M)[:3, :3].T @ PLANE_N)
    n = 64
    rng = np.random.default_rng(5)
    z = np.zeros(n, np.int64)
    code = rng.integers(0, 20000, n).astype(np.uint32) | (rng.integers(0, 20000, n).astype(np.uint32) << 16)
    nm = P.restated_normals(tris, md, z, z, code)
    assert np.linalg.norm(nm.g - want, axis=1).max() <= P.E_OCT_HALF * 6  # the rounded 16:16 code, kappa = 6
    assert np.abs(nm.us - want).max() < 1e-6         # float32 W2L entries
    geo, corner = P.geometric_normal(tris, md, z, z, nm.g)
    assert np.abs(geo - want).max() < 1e-6
    for form in ("W2L", "L2W"):
        assert np.abs(P.restated_normals(tris, md, z, z, code, form=form).g - want).max() > 0.1
    # rays from both sides onto the plane
    src = np.zeros(n, tthip.RAY_DTYPE)
    d = P._unit(rng.normal(size=(n, 3)))
    a, b = rng.uniform(0.1, 0.4, (2, n, 1))
    obj = np.array([-1.0, 1.0, 0.0]) + a * np.array([3.0, -3.0, 0.0]) + b * np.array([0.0, 3.0, -3.0])
    hit = obj @ M[:3, :3].T + M[:3, 3]
    src["direction"], src["origin"] = d, hit - 2.0 * d.astype(np.float32).astype(np.float64)
    src["PixelIndex"] = np.arange(n)
    src["hits"] = np.stack([z, z, np.full(n, np.float32(2.0).view(np.uint32)), code], 1)
    m = P.bounce(tris, md, src, FAR, 0, 3, 5)
    assert m.firm.all() and not m.marginal.any()
    side = np.where((d * want).sum(1) > 0, -1.0, 1.0)
    assert np.array_equal(m.flipped, side < 0)
    assert np.abs(m.n_side - side[:, None] * want).max() < 1e-6
    assert np.abs(((m.pos - corner) * want).sum(1)).max() < 1e-5   # the hit points lie on the plane
    assert np.abs(m.norm[:, 0] - side[:, None] * want).max() < 7 * P.E_OCT_HALF
    assert np.allclose((m.lobe.om ** 2).sum(1), 1.0, atol=1e-12)


def test_model_on_the_ellipsoids():
    """The restated smooth normal of random records against the analytic ellipsoid normal at the world point the
    record names: ties the packed normals' order, the barycentrics and the matrix to the TRS parameters."""
    sc = PC.scene("ellipsoid")
    rays = PC.records(sc, 8000, 77)
    mesh, tri, code = rays["hits"][:, 0].astype(np.int64), rays["hits"][:, 1].astype(np.int64), rays["hits"][:, 3]
    nm = P.restated_normals(sc.tris, sc.meshdata, mesh, tri, code)
    p = PC.world_point(sc, mesh, tri, (code & 0xFFFF), (code >> 16))
    worst = 0.0
    for k, (c, R, s) in enumerate(PC.PARENTS):
        w = mesh == k
        assert w.sum() > 1000
        want = P.analytic_ellipsoid_normal(p[w], c, R, s)
        bound = P.analytic_ellipsoid_bound(sc.tris, tri[w], p[w], p[w], np.zeros(w.sum()), c, R, s)
        err = np.linalg.norm(nm.g[w] - want, axis=1)
        assert (err <= bound).all(), (k, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
        geo, _ = P.geometric_normal(sc.tris, sc.meshdata, mesh[w], tri[w], nm.g[w])
        assert (np.linalg.norm(geo - nm.us[w], axis=1) <= nm.tol_us[w]).all()
        assert ((geo * want).sum(1) > 0.9).all()      # the face normal of a 1,280-triangle sphere is near the smooth one
    print(f"ellipsoids: restated against analytic, worst {worst:.3f} of the bound")
    # the geometric model is the cross product of the brute-force pin's world corners
    import bruteforce as BF

    bg = BF.Geometry.from_scene(sc)
    for k in range(len(PC.PARENTS)):
        lo, hi = bg.ranges[k]
        c0, c1, c2 = bg.world_corners(k).reshape(3, hi - lo, 3)
        face = P._unit(np.cross(c1 - c0, c2 - c0))
        at = np.arange(lo, hi)
        geo, corner = P.geometric_normal(sc.tris, sc.meshdata, np.full(hi - lo, k), at, face)
        assert np.abs(geo - face).max() < 1e-12 and np.abs(corner - c0).max() < 1e-9
    for form in ("W2L", "L2W"):
        bad = P.restated_normals(sc.tris, sc.meshdata, mesh, tri, code, form=form)
        for k in (1, 2):   # only the skewed parents separate the three matrices
            assert np.linalg.norm(bad.g[mesh == k] - nm.g[mesh == k], axis=1).max() > 0.1
        assert np.abs(bad.g[mesh == 0] - nm.g[mesh == 0]).max() < 1e-12


def test_octahedral_round_trip_candidates():
    rng = np.random.default_rng(9)
    n = P._unit(rng.normal(size=(20000, 3)))
    codes, valid, slack = P.oct_round_trip(n, np.full(len(n), 1e-6))
    back = P.oct_decode(codes[:, 0])
    assert np.linalg.norm(back - n, axis=1).max() <= P.E_OCT_HALF
    assert 0.02 < valid[:, 1:].any(1).mean() < 0.5 and (slack > 0).mean() < 1e-3
    c2 = np.uint32(np.rint(P.oct_encode_pre(back)[0])) | (np.uint32(np.rint(P.oct_encode_pre(back)[1])) << 16)
    assert (np.linalg.norm(P.oct_decode(c2) - back, axis=1) < 1e-9).all()   # decoded normals encode to themselves


# ------------------------------------------------------------------ Generate
@pytest.mark.parametrize("case", PC.generate_cases(), ids=lambda c: "-".join(str(x) for x in c))
def test_oracle_generate(case):
    cn, W, H, jit, fr, mb = case
    cam = PC.CAMERAS[cn]
    c2w, ip = PC.camera_matrices(cam, W, H)
    PC.compare_generate(cam, W, H, jit, fr, mb, SIDE.generate(c2w, ip, W, H, cam.near, cam.far, jit, fr, mb)).check().say(
        f"generate {case}")


def test_generate_mutants_are_reported():
    for cn in ("oblique", "shift"):
        cam = PC.CAMERAS[cn]
        for name, (rays, must) in PC.generate_mutants(cam, 64, 65, 3, 5).items():
            if name == "lens-shift terms dropped" and cn != "shift":
                continue
            assert must in PC.compare_generate(cam, 64, 65, 1, 3, 5, rays).names(), (cn, name)


def test_oracle_jitter_is_uniform_over_the_footprint():
    cam = PC.CAMERAS["oblique"]
    W, H = 64, 65
    c2w, ip = PC.camera_matrices(cam, W, H)
    by = {fr: SIDE.generate(c2w, ip, W, H, cam.near, cam.far, 1, fr, 5) for fr in (0, 3, 0x7FFFFFFF)}
    PC.compare_jitter(cam, W, H, by).check().say("jitter")
    assert "same jitter in different frames" in PC.compare_jitter(cam, W, H, {0: by[0], 1: by[0]}).names()
    shifted = PC.rays_from_matrices(c2w, ip, W, H, cam.near, cam.far, 1, 3, 5, centre=0.0)
    assert PC.compare_jitter(cam, W, H, {3: shifted}).names()


# ------------------------------------------------------------------ traced chains
@pytest.mark.parametrize("name", list(PC.TRACED))
def test_oracle_traced_chain(name):
    seen = {}
    for stage, rep in PC.traced_chain(SIDE, name):
        rep.check().say(f"{name} {stage}")
        seen[stage] = rep
    # (a lone convex body sends no bounce back to itself: the far camera's second enqueue is an all-dead launch)
    assert seen["bounce 0"].counts["survivors"] > 300
    assert seen["bounce 1"].counts["survivors"] >= (0 if name == "far" else 30)
    if name == "near":
        assert seen["bounce 0"].counts["mirrored"] >= 100
    if name == "far":
        assert seen["bounce 0"].counts["far"] >= 100


def test_oracle_traces_the_mirrored_parent_as_the_brute_force_does():
    """The traversal under a mirrored record, against the brute-force pin's comparison."""
    import bruteforce as BF
    import bruteforce_cases as BFC

    sname, cam, W, H = PC.TRACED["near"]
    sc = PC.scene(sname)
    c2w, ip = PC.camera_matrices(cam, W, H)
    buf = SIDE.generate(c2w, ip, W, H, cam.near, cam.far, 1, 3, 5)
    SIDE.trace(sc, buf, W * H, 0, W, H)
    pick = np.arange(0, W * H, 5)
    ref = BF.closest(BF.Geometry.from_scene(sc), buf["origin"][pick], buf["direction"][pick], FAR)
    assert (ref.hit & (ref.mesh == PC.MIRRORED)).sum() >= 50
    BFC.compare_closest(ref, buf["hits"][pick]).check()


def test_resolve_mutants_are_reported():
    sname, cam, W, H = PC.TRACED["near"]
    sc = PC.scene(sname)
    c2w, ip = PC.camera_matrices(cam, W, H)
    buf = SIDE.generate(c2w, ip, W, H, cam.near, cam.far, 1, 3, 5)
    SIDE.trace(sc, buf, W * H, 0, W, H)
    src = buf[:W * H]
    out = SIDE.resolve(sc, buf, W * H, 0, W, H)
    PC.compare_resolve(sc, src, out, True).check()
    for form in ("W2L", "L2W"):
        names = PC.compare_resolve(sc, src, PC.mutant_normals(sc, src, out, form), True).names()
        assert {"smooth normal", "smooth normal against the ellipsoid",
                "unsmoothed normal against the world triangle"} <= names, (form, names)
    bad = out.copy()
    bad[~PC.valid_records(sc, src), 4] = 1e-30
    assert "six zeros" in PC.compare_resolve(sc, src, bad, True).names()


def test_oracle_resolve_of_the_synthetic_records():
    c = PC.resolve_case()
    sc = PC.scene(c.scene)
    buf, off, _ = PC.frame_buffer(c)
    n = len(c.src)
    assert n % 256 != 0 and c.bounce == 1 and off == c.W * c.H
    out = SIDE.resolve(sc, buf, n, c.bounce, c.W, c.H)
    rep = PC.compare_resolve(sc, c.src, out, True).check().say("resolve, synthetic")
    assert n - rep.counts["valid"] > 500


# ------------------------------------------------------------------ the synthetic enqueue cases
def test_oracle_coverage_case_and_bounce_mutants():
    c = PC.coverage_case()
    sc = PC.scene(c.scene)
    count, rows, rep = PC.run_enqueue(SIDE, c)
    rep.check()
    m = P.bounce(sc.tris, sc.meshdata, c.src, FAR, c.bounce, c.frames, c.max_bounce)
    rep = PC.compare_bounce(c, count, rows, m).check().say("coverage")
    for k, least in PC.COVERAGE.items():
        assert rep.counts[k] >= least, (k, rep.counts)
    assert rep.counts["pairs"] >= 40
    # the records that are marginal by construction are classed so
    pos = {int(i): k for k, i in enumerate(m.idx)}
    inplane = [pos[i] for i in np.nonzero(c.by_construction)[0][:-1]]
    assert len(inplane) >= 40 and m.marginal_flip[inplane].all()
    assert m.open_pdf[len(c.src) - 1] and m.open_pdf.sum() == 1
    PC.compare_lobe(c, rows, m).check().say("lobe")
    if m.open_pdf[m.idx].any() and len(rows) != len(m.idx):   # the open ray did not survive: mutate the firm rows
        keep = ~m.open_pdf
        c = PC.dataclasses.replace(c, src=c.src[keep], by_construction=c.by_construction[keep])
    for name, (cnt, mrows, must) in PC.bounce_mutants(c, len(rows), rows).items():
        names = PC.compare_bounce(c, cnt, mrows).names()
        assert must in names, (name, names)
        if name == "direction from a uniform hemisphere":
            assert "cosine lobe not distributed as the lobe" in PC.compare_lobe(c, mrows).names()
        if name == "origin offset along -us":
            assert "origin offset" in names


@pytest.mark.parametrize("name", PC.PATTERNS)
def test_oracle_survivor_patterns(name):
    c = PC.pattern_case(name)
    count, rows, rep = PC.run_enqueue(SIDE, c)
    rep.check()
    rep = PC.compare_bounce(c, count, rows).check().say(name)
    # (one per wave: the ragged last wave's single lane is not its live one)
    want = {"all dead": 0, "all live": PC.PATTERN_N, "alternating": PC.PATTERN_N // 2,
            "one per wave": PC.PATTERN_N // 64, "last lane of a tile": 2}[name]
    assert rep.counts["survivors"] == want == count


def test_oracle_look_back_order():
    c = PC.lookback_case()
    count, rows, rep = PC.run_enqueue(SIDE, c)
    rep.check()
    rep = PC.compare_bounce(c, count, rows).check()
    assert 100_000 < count < 170_000
    sw = rows.copy()
    sw[[70000, 70001]] = sw[[70001, 70000]]
    assert "source order" in PC.compare_bounce(c, count, sw).names()


def test_oracle_batched_frames():
    c = PC.batched_case()
    count, rows, rep = PC.run_enqueue(SIDE, c)
    rep.check()
    PC.compare_bounce(c, count, rows).check().say("batched")
    assert (rows["PixelIndex"] >= c.frame_pixels).sum() > 500
    cnt, mrows, must = PC.bounce_mutants(c, count, rows)["PixelIndex of the frame-local pixel"]
    assert must in PC.compare_bounce(c, cnt, mrows).names()
    # an enqueue that ignores frame_pixels draws other directions for frame 1
    plain = PC.dataclasses.replace(c, frame_pixels=0)
    assert PC.compare_bounce(plain, count, rows).names()
