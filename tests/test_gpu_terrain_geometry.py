"""The heightmap kernels against geometry, with no host reference in between: what tt_trace_heightmap,
tt_trace_heightmap_hits, tt_trace_shadow_heightmap, tt_resolve_normals and the terrain rows of
tt_enqueue_diffuse_bounce write is compared with the float64 heightmap surface of tests/terrain_geometry.py, on
the sets, classes and assertions of tests/test_terrain_geometry_host.py (tests/terrain_geometry_cases.py holds
them). The parity tests prove kernel == host reference bit for bit; an error the two share passes them all and
fails here. Neither the host reference nor the oracle is called in this file.

Measured on the kernels, MI355X (a test that measures a figure prints it, as "FIGURE gpu ..."; run with -s). The
slopes, class shares and ambiguous shares are properties of the sets: tests/test_terrain_geometry_host.py lists them
(slopes 1.4764, 1.8638 and 1.2037; at most 0.8 % of a set ambiguous).
  t - t_cross, must-hit    at most -1.1e-4 (bound +1e-5)
  gap at the reported hit  2.232e-4 .. 4.08e-4 (bounds -2.4e-4 .. 4.6e-4), host and device pointers, bounce 0 and 1
  packed uv / float uv     1.526e-5 (bound 1.566e-5) / 1.8e-7 (bound 4e-6)
  normal against secant    3.5e-6 (A), 1.7e-6 (B), both triples (bound 1e-5)
  bounce                   1,116 terrain rows; origin 1.005e-4 from the hit point (bound 2e-4), direction . normal -
                           pdf pi 3.8e-5 (bound 1e-4)
No must-hit, must-miss, starts-below, occluded or clear ray disagrees.
"""
import numpy as np
import pytest

import terrain_cases as TC
import terrain_geometry_cases as GC
import tthip

pytestmark = pytest.mark.gpu
FAR, TID = GC.FAR, GC.TID
FRAMES, MAXB = 3, 4
CANARY = 0x5A5A5A5A


def show(what, value):
    print(f"FIGURE gpu {what}: {value}")


@pytest.fixture(scope="module")
def engines():
    """A context of this module's own per upload of terrains: scene A's two, its terrain 0 alone (what terrain 1's
    stage starts from), scene B's one. The triangle scene is the Cornell box throughout; no record here names it."""
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    a, b = GC.scene_a(), GC.scene_b()
    made = {}
    try:
        for key, c, terrains in (("A", a, a.terrains), ("A0", a, a.terrains[:1]), ("B", b, b.terrains)):
            e = made[key] = tthip.Engine(0)
            e.upload(TC.scene())
            e.upload_terrains(terrains, c.atlas_bits)
        yield made
    finally:
        for e in made.values():
            e.close()


def _dev(a):
    import torch

    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def gpu_trace(eng, c, rays, bounce, n=None, device=False, hits=False):
    """(before, after, info[, hit stream]) of the launch window after tt_trace_heightmap(_hits); asserts that no
    ray outside the launch was written."""
    n = len(rays) if n is None else n
    buf, off = c.frame(bounce, rays)
    start, info = buf.copy(), c.info()
    stream = None
    if device or hits:
        d_buf, d_info = _dev(buf), _dev(info)
        if hits:
            import torch

            d_hits = torch.full((n, 4), CANARY, dtype=torch.int32, device="cuda:0")
            eng.trace_heightmap_hits(d_buf, d_hits, n, bounce, FAR, c.W, c.H, info=d_info)
            stream = d_hits.cpu().numpy().view(np.uint32)
        else:
            eng.trace_heightmap(d_buf, n, bounce, FAR, c.W, c.H, info=d_info, device=True)
        buf, info = _host(d_buf, buf), _host(d_info, info)
    else:
        eng.trace_heightmap(buf, n, bounce, FAR, c.W, c.H, info=info)
    keep = np.ones(len(buf), bool)
    keep[off:off + n] = False
    assert buf[keep].tobytes() == start[keep].tobytes(), "a ray outside the launch was written"
    out = (start[off:off + n], buf[off:off + n], info)
    return out + (stream,) if hits else out


_AFTER0 = {}


def after_terrain0(engines, bounce):
    """Scene A's records as the kernel leaves them after terrain 0 alone."""
    if bounce not in _AFTER0:
        c = GC.scene_a()
        _AFTER0[bounce] = gpu_trace(engines["A0"], c, c.rays, bounce)[1]
    return _AFTER0[bounce]


# ------------------------------------------------------------------ closest hit
@pytest.mark.parametrize("device", [False, True], ids=["host_ptrs", "device_ptrs"])
@pytest.mark.parametrize("bounce", [0, 1])
@pytest.mark.parametrize("name", ["A", "B"])
def test_one_terrain_against_the_surface(engines, name, bounce, device):
    c = GC.case(name)
    eng = engines["A0" if name == "A" else "B"]
    e = GC.expect_one(name)
    before, after, info = gpu_trace(eng, c, c.rays, bounce, device=device)
    r = GC.compare_closest(c, e, before, after, info, bounce, terrains=c.terrains[:1])
    show(f"closest {name} bounce {bounce}", r.worst)
    r.check()
    # a launch that ends one lane into a wave: the same rays, the same answers
    before, after, info = gpu_trace(eng, c, c.rays, bounce, n=GC.N_SHORT, device=device)
    GC.compare_closest(c, e.head(GC.N_SHORT), before, after, info, bounce, terrains=c.terrains[:1]).check()


@pytest.mark.parametrize("bounce,device", [(0, False), (1, True)])
def test_two_terrains_nearer_one_wins(engines, bounce, device):
    c = GC.scene_a()
    after0 = after_terrain0(engines, bounce)
    e2 = GC.expect_two(after0)
    front, behind = GC.two_terrain_sides(e2, after0)
    assert front >= 10 and behind >= 10 and e2.shares()["ambiguous"] <= 0.02
    before, after, info = gpu_trace(engines["A"], c, c.rays, bounce, device=device)
    r = GC.compare_closest(c, e2, before, after, info, bounce)
    show(f"closest A, both terrains, bounce {bounce}", r.worst)
    r.check()


def test_finite_limit_is_measured_from_the_box_entry(engines):
    c = GC.scene_a()
    rays, e, rule_hit, rule_keep = GC.finite_variant()
    sure_hit, sure_keep = rule_hit & (e.kind != GC.AMB), rule_keep & (e.kind != GC.AMB)
    assert sure_hit.sum() >= 100 and sure_keep.sum() >= 100
    for bounce, device in ((0, False), (1, True)):
        before, after, info = gpu_trace(engines["A0"], c, rays, bounce, device=device)
        r = GC.compare_closest(c, e, before, after, info, bounce, terrains=c.terrains[:1])
        show(f"closest A, finite limits, bounce {bounce}", r.worst)
        r.check()
        assert (after["hits"][sure_keep, 1] == GC.MARKER).all() and (after["hits"][sure_hit, 0] == TID).all()


@pytest.mark.parametrize("name,bounce", [("B", 0), ("A", 1)])
def test_hit_stream_equals_the_rewritten_records(engines, name, bounce):
    c = GC.case(name)
    eng = engines["A0" if name == "A" else "B"]
    before, after, info, stream = gpu_trace(eng, c, c.rays, bounce, hits=True)
    GC.compare_closest(c, GC.expect_one(name), before, after, info, bounce, terrains=c.terrains[:1]).check()
    rewritten = (after["hits"] != before["hits"]).any(axis=1)
    assert rewritten.sum() >= 0.2 * c.n and (~rewritten).sum() >= 0.2 * c.n
    assert np.array_equal(stream[rewritten], after["hits"][rewritten])
    assert (stream[~rewritten] == CANARY).all()


# ------------------------------------------------------------------ shadow
@pytest.mark.parametrize("bounce", [0, 1])
def test_shadow_classes(engines, bounce):
    s = GC.shadow_set().copy()
    vis = np.full((len(s), 4), -7.5, np.float32)
    engines["A"].shadow_heightmap(s, len(s), bounce, TC.SW, TC.SH, visibility=vis)
    assert np.array_equal(s, GC.shadow_set()), "the rays are not written"
    live = s["t"] != 0
    assert (vis[~live] == np.float32(-7.5)).all(), "a ray with t == 0 is not marched"
    assert np.isin(vis[live], (0.0, 1.0)).all() and (vis[live] == vis[live][:, :1]).all()
    GC.compare_shadow(GC.shadow_classes(), live, np.where(live, 1 - vis[:, 0], 0).astype(np.int64)).check()


# ------------------------------------------------------------------ normals, bounce
@pytest.mark.parametrize("name", ["A", "B"])
def test_resolve_normals_are_the_secant_normals(engines, name):
    c = GC.case(name)
    eng = engines[name]
    before, after, _ = gpu_trace(eng, c, c.rays, 0)
    ter, pos = GC.hit_points(c, before, after)
    assert len(ter) >= 300
    buf, _ = c.frame(0, after)
    out = eng.resolve_normals(buf, c.n, 0, FAR, c.W, c.H)
    want = GC.normals64(c, after, ter, pos)
    for triple in (out[ter, :3], out[ter, 3:]):
        r = GC.compare_normals(want, triple)
        show(f"normal error {name}", r.worst["normal"])
        r.check()
    assert (out[ter, 1] < 0).all(), "the reference's normal points down"


def test_bounce_leaves_along_the_float64_normal(engines):
    c = GC.scene_a()
    _, after, _ = gpu_trace(engines["A"], c, c.rays, 0)
    buf, _ = c.frame(0, after)
    start = buf.copy()
    dst = c.W * c.H
    cnt = engines["A"].enqueue_bounce(buf, c.n, 0, FAR, c.W, c.H, frames=FRAMES, max_bounce=MAXB, terrain_bounce=True)
    assert np.array_equal(buf[:dst], start[:dst]), "the source half is not written"
    rows = buf[dst:dst + cnt]
    assert (rows["hits"][:, 0] == TID).all(), "every other record here is a miss, whose path ends"
    assert cnt >= 500
    r = GC.compare_bounce(c, after, rows)
    show("bounce A", r.worst)
    r.check()
    assert r.worst["flipped"] >= 50
