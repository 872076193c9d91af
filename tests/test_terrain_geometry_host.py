"""The host reference of the heightmap kernels (host/tt_terrain.cpp) against geometry: a float64 heightmap
surface written from the shaders' semantics (tests/terrain_geometry.py), on the sets of
tests/terrain_geometry_cases.py. Every other terrain test compares the kernels with that host reference bit for
bit; an error the two share (a swapped rectangle corner, a half-texel shift, dimX where dimZ belongs, a normal of
the wrong handedness) passes them all and fails here. tests/test_gpu_terrain_geometry.py runs the same sets,
classes and assertions on what the kernels write.

Measured on the host reference (a test that measures a figure prints it, as "FIGURE host ..."; run with -s):
  largest slope            scene A terrain 0: 1.4764, terrain 1: 1.8638; scene B: 1.2037
  ambiguous share          A on terrain 0: 0 of 1,500; A on terrain 1: 0.8 % (the rays skimming its plateau); A with
                           both terrains, terrain 1's stage: 0.8 %; B: 0 of 1,200; finite limits: 0; shadow: 0 of 1,319
  classes                  A / terrain 0: 50.3 % must-hit, 42.1 % must-miss, 7.6 % starts-below; B: 51.6 %, 31.4 %,
                           17.0 %; shadow: 21.3 % occluded, 78.7 % clear; finite limits: 420 rays to hit, 335 to keep
                           their record; terrain 0 hits that terrain 1 takes: 70, leaves though it lies on their
                           line: 19
  t - t_cross, must-hit    at most -1.1e-4 (bound +1e-5): the march stops short of the crossing
  gap at the reported hit  2.232e-4 .. 4.08e-4 (bounds -2.4e-4 .. 4.6e-4)
  packed uv / float uv     1.526e-5 (bound 1.566e-5) / 1.8e-7 (bound 4e-6)
  normal against secant    3.5e-6 (A), 1.7e-6 (B) (bound 1e-5)
  bounce                   origin 1.005e-4 from the hit point (bound 2e-4), direction . normal - pdf pi 3.8e-5 (1e-4)
"""
import numpy as np
import pytest

import terrain_geometry as TG
import terrain_geometry_cases as GC
import tthip

FAR, TID = GC.FAR, GC.TID
MISS, HIT, BELOW, AMB = GC.MISS, GC.HIT, GC.BELOW, GC.AMB
FRAMES, MAXB = 3, 4


def show(what, value):
    print(f"FIGURE host {what}: {value}")


def host_trace(c, rays, bounce, terrains=None, n=None, with_info=True):
    """(before, after, info) of the launch window after tt_terrain_trace_host."""
    terrains = c.terrains if terrains is None else terrains
    n = len(rays) if n is None else n
    buf, off = c.frame(bounce, rays)
    start = buf.copy()
    info = c.info() if with_info else None
    tthip.terrain_trace_host(terrains, c.atlas_bits, buf, n, bounce, FAR, c.W, c.H, info=info)
    keep = np.ones(len(buf), bool)
    keep[off:off + n] = False
    assert buf[keep].tobytes() == start[keep].tobytes(), "a ray outside the launch was written"
    return start[off:off + n], buf[off:off + n], info


_TRACED = {}


def traced(name, terrains="all", bounce=0):
    """Scene `name` on miss records through the host reference, once per form."""
    key = (name, terrains, bounce)
    if key not in _TRACED:
        c = GC.case(name)
        _TRACED[key] = host_trace(c, c.rays, bounce, None if terrains == "all" else c.terrains[:1])
    return _TRACED[key]


# ------------------------------------------------------------------ conditions
@pytest.mark.parametrize("name", ["A", "B"])
def test_slopes_are_below_two(name):
    """Nothing in this file means anything at slope 2 or above."""
    c = GC.case(name)
    for i, T in enumerate(c.terrains):
        s = TG.max_slope(T, c.atlas)
        show(f"max slope {name}/{i}", round(s, 4))
        assert s < GC.SLOPE_BOUND


def check_coverage(shares, what):
    show(f"class shares {what}", {k: round(v, 4) for k, v in shares.items()})
    assert shares["ambiguous"] <= 0.02, what
    assert shares["hit"] >= 0.20 and shares["miss"] >= 0.20 and shares["below"] >= 0.03, what


def test_sets_cover_every_class_and_few_rays_are_ambiguous():
    check_coverage(GC.expect_one("B").shares(), "B")
    e0 = GC.expect_one("A")
    check_coverage(e0.shares(), "A, terrain 0")
    k1 = GC._far_classes("A", 1)[0]
    show("ambiguous share A, terrain 1", round(float((k1 == AMB).mean()), 4))
    assert (k1 == AMB).mean() <= 0.02
    after0 = traced("A", "first")[1]
    e2 = GC.expect_two(after0)
    show("class shares A, both terrains, terrain 1's stage", {k: round(v, 4) for k, v in e2.shares().items()})
    assert e2.shares()["ambiguous"] <= 0.02
    front, behind = GC.two_terrain_sides(e2, after0)
    show("terrain 0 hits that terrain 1 takes / keeps", (front, behind))
    assert front >= 10 and behind >= 10  # (a floor on the set, not on an answer: both orders occur more than once)
    sc =GC.shadow_classes()
    live = GC.shadow_set()["t"] != 0
    shares = {k: float((sc[live] == v).mean()) for k, v in (("clear", TG.CLEAR), ("occluded", TG.OCCLUDED),
                                                            ("ambiguous", AMB))}
    show("shadow class shares of the live rays", {k: round(v, 4) for k, v in shares.items()})
    assert shares["ambiguous"] <= 0.02 and shares["occluded"] >= 0.10 and shares["clear"] >= 0.20
    assert (~live).sum() >= 100


# ------------------------------------------------------------------ closest hit
@pytest.mark.parametrize("bounce", [0, 1])
@pytest.mark.parametrize("name", ["A", "B"])
def test_one_terrain_against_the_surface(name, bounce):
    c = GC.case(name)
    before, after, info = traced(name, "first", bounce)
    r = GC.compare_closest(c, GC.expect_one(name), before, after, info, bounce, terrains=c.terrains[:1])
    show(f"closest {name} bounce {bounce}", r.worst)
    r.check()


def test_head_of_each_set():
    for name in ("A", "B"):
        c = GC.case(name)
        before, after, info = host_trace(c, c.rays, 1, c.terrains[:1], n=GC.N_SHORT)
        GC.compare_closest(c, GC.expect_one(name).head(GC.N_SHORT), before, after, info, 1,
                           terrains=c.terrains[:1]).check()


@pytest.mark.parametrize("bounce", [0, 1])
def test_two_terrains_nearer_one_wins(bounce):
    c = GC.scene_a()
    after0 = traced("A", "first", bounce)[1]
    before, after, info = traced("A", "all", bounce)
    r = GC.compare_closest(c, GC.expect_two(after0), before, after, info, bounce)
    show(f"closest A, both terrains, bounce {bounce}", r.worst)
    r.check()


def test_finite_limit_is_measured_from_the_box_entry():
    c = GC.scene_a()
    rays, e, rule_hit, rule_keep = GC.finite_variant()
    sure_hit, sure_keep = rule_hit & (e.kind != AMB), rule_keep & (e.kind != AMB)
    show("finite limit: rays to hit / to keep their record", (int(sure_hit.sum()), int(sure_keep.sum())))
    assert sure_hit.sum() >= 100 and sure_keep.sum() >= 100
    assert (e.kind[sure_hit] == HIT).all() and (e.kind[sure_keep] == MISS).all()
    assert (e.kind == AMB).mean() <= 0.02
    before, after, info = host_trace(c, rays, 0, c.terrains[:1])
    r = GC.compare_closest(c, e, before, after, info, 0, terrains=c.terrains[:1])
    show("closest A, finite limits", r.worst)
    r.check()
    assert (after["hits"][sure_keep, 1] == GC.MARKER).all() and (after["hits"][sure_hit, 0] == TID).all()


# ------------------------------------------------------------------ shadow
def test_shadow_classes():
    c, s = GC.scene_a(), GC.shadow_set()
    occ, _ = tthip.terrain_occluded_host(c.terrains, c.atlas_bits, s.copy(), len(s))
    GC.compare_shadow(GC.shadow_classes(), s["t"] != 0, occ).check()


# ------------------------------------------------------------------ normals, bounce
@pytest.mark.parametrize("name", ["A", "B"])
def test_normals_are_the_secant_normals(name):
    c = GC.case(name)
    before, after, _ = traced(name, "all", 0)
    ter, pos = GC.hit_points(c, before, after)
    assert len(ter) >= 300
    got = np.stack([tthip.terrain_normal_host(c.terrains, c.atlas_bits, p.astype(np.float32), int(i))
                    for p, i in zip(pos, after["hits"][ter, 1])])
    r = GC.compare_normals(GC.normals64(c, after, ter, pos), got)
    show(f"normal error {name}", r.worst["normal"])
    r.check()
    assert (got[:, 1] < 0).all(), "the reference's normal points down"


def test_bounce_leaves_along_the_float64_normal():
    c = GC.scene_a()
    before, after, _ = traced("A", "all", 0)
    buf, off = c.frame(0, after)
    out, sv = tthip.terrain_bounce_host(c.terrains, c.atlas_bits, buf, c.n, 0, FAR, c.W, c.H, frames=FRAMES,
                                        max_bounce=MAXB)
    assert np.array_equal(sv >= 0, after["hits"][:, 0] == TID)
    rows = out[sv == 1]
    assert len(rows) >= 500
    r = GC.compare_bounce(c, after, rows)
    show("bounce A", r.worst)
    r.check()
    assert r.worst["flipped"] >= 50


# ------------------------------------------------------------------ control: the comparison can fail
def _broken(T, atlas, x, z, half_texel=0.5, exchange=False, dim_z_index=1):
    """terrain_geometry.surface with one mistake put in."""
    P, dim, hm = (T[k].astype(np.float64) for k in ("PositionOffset", "TerrainDim", "HeightMap"))
    u, v = np.minimum((x - P[0]) / dim[0], 1.0), np.minimum((z - P[2]) / dim[dim_z_index], 1.0)
    if exchange:
        u, v = v, u
    b = TG.bilinear_clamp(atlas, u * (hm[0] - hm[2]) + hm[2], v * (hm[1] - hm[3]) + hm[3], half_texel=half_texel)
    return P[1] + 0.01 + 2.0 * float(T["HeightScale"]) * b


def no_half_texel(T, atlas, x, z):
    return _broken(T, atlas, x, z, half_texel=0.0)


def uv_exchanged(T, atlas, x, z):
    return _broken(T, atlas, x, z, exchange=True)


def dim_x_for_both(T, atlas, x, z):
    return _broken(T, atlas, x, z, dim_z_index=0)


@pytest.mark.parametrize("name,broken", [("A", no_half_texel), ("B", no_half_texel), ("B", uv_exchanged),
                                         ("B", dim_x_for_both)])
def test_a_broken_surface_is_noticed(name, broken):
    """Each of three mistakes put into the float64 surface makes the same comparison with the same host output
    report violations, of the record / miss assertions and of the hit height."""
    c = GC.case(name)
    before, after, info = traced(name, "first", 0)
    r = GC.compare_closest(c, GC.expect_one(name, surf=broken), before, after, None, 0, terrains=c.terrains[:1],
                           surf=broken)
    show(f"control {name} {broken.__name__}", {k: len(v) for k, v in r.bad.items()})
    assert r.count("record") + r.count("miss") > 0 and r.count("gap") > 0
