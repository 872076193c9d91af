"""Deep traversal stacks on the GPU: entries beyond the LDS part of the stack (TT_LDS_STACK = 12 of 16; the rest
spills to a global area) with known answers, in the scalar loops, in the cooperative drain with a stack column
that is not the lane's own, and in the any-hit kernel.

kat_cases.stack_overflow_scene(depth) is a chain whose every level pushes one entry: depth 16 fills the stack
exactly (four spilled entries, all popped again by a closest-hit ray), depth 17 overflows. One such ray alone goes
to the drain phase at once, so the shapes below put whole waves on the chain:
  * 64 identical rays: the wave that dequeues them never enters the drain (they finish in the same iteration,
    before the queue is known dry), so every push and pop is the scalar loop's;
  * 64 rays whose even-indexed ones miss at the root: the 32 live rays sit on odd lanes and regroup onto groups
    led by even lanes, which then address the odd lanes' stack columns;
  * 96 rays: the second wave gets 32 and starts in the drain at exactly TT_WIDE_ENTER live rays.
Expected records are the oracle's (tests/oracle_ctypes.py).
"""
import numpy as np
import pytest

import handbuilt as hb
import kat_cases as K
import oracle_ctypes as O
import tthip

from parity_util import FAR, assert_same, same_floats

pytestmark = pytest.mark.gpu

ORIGIN, DOWN = (0.25, 0.25, 1.0), (0.0, 0.0, -1.0)
AWAY_ORIGIN, AWAY = (0.25, 0.25, 1000.0), (0.0, 0.0, 1.0)  # beyond the TLAS root's box, heading off: one node visit
POISON = [7, 8, 9, 10]
SHAPES = ["full_wave", "odd_lanes_live", "second_wave_of_32"]


def _rays_of(shape):
    """(origins, directions) of a shape; every ray that is not an `away` ray is the chain's ray."""
    n = 96 if shape == "second_wave_of_32" else 64
    o, d = [ORIGIN] * n, [DOWN] * n
    if shape == "odd_lanes_live":
        o[0::2], d[0::2] = [AWAY_ORIGIN] * (n // 2), [AWAY] * (n // 2)
    return n, o, d


def _closest_rays(shape):
    n, o, d = _rays_of(shape)
    r = hb.rays_buffer(o, d, FAR)
    r["hits"][:n] = POISON
    return n, r


@pytest.fixture(scope="module")
def chain16():
    return K.stack_overflow_scene(16)[0]


@pytest.fixture(scope="module")
def chain17():
    return K.stack_overflow_scene(17)[0]


@pytest.fixture(scope="module")
def closest_expected(chain16):
    """The oracle's records and per-ray counts of every shape on the depth-16 chain, computed once."""
    out = {}
    for shape in SHAPES:
        n, r = _closest_rays(shape)
        st, cnt = O.trace(chain16, r, n, 0, FAR, n, 1, counts=True)
        assert st == 0 and int(cnt["max_stack"].max()) == 16
        live = np.ones(n, bool)
        if shape == "odd_lanes_live":
            live[0::2] = False
            assert (cnt["node_visits"][~live] == 1).all(), "the away rays miss at the root"
        assert (r["hits"][:n][live, 1] == 0).all() and (r["hits"][:n][~live, 1] == 0xFFFFFFFF).all()
        out[shape] = (r, cnt)
    return out


# ------------------------------------------------------------------ closest hit
@pytest.mark.parametrize("shape", SHAPES)
def test_closest_depth16_records(engine, chain16, closest_expected, shape):
    want, _ = closest_expected[shape]
    n, got = _closest_rays(shape)
    engine.upload(chain16)
    engine.trace(got, n, 0, FAR, n, 1)
    assert_same(got, want, None, None, 0, n)


def test_closest_depth17_full_wave_overflows(engine, chain17):
    n, r = _closest_rays("full_wave")
    before = r.copy()
    engine.upload(chain17)
    s, st = engine.trace(r, n, 0, FAR, n, 1, check=False)
    assert st == tthip.TT_ERR_STACK_OVERFLOW and s.stack_overflows == 64
    assert (r["hits"][:n] == POISON).all() and np.array_equal(r.view(np.uint8), before.view(np.uint8))


def test_closest_depth16_full_wave_stats(engine, chain16, closest_expected):
    want, cnt = closest_expected["full_wave"]
    n, got = _closest_rays("full_wave")
    engine.upload(chain16)
    s = engine.trace(got, n, 0, FAR, n, 1, stats=True)
    assert_same(got, want, None, None, 0, n)
    assert s.rays == n and s.hits == int((want["hits"][:n, 1] != 0xFFFFFFFF).sum())
    assert s.node_visits == int(cnt["node_visits"].sum()) and s.tri_tests == int(cnt["tri_tests"].sum())
    assert s.blas_entries == int(cnt["blas_entries"].sum()) and s.accepts == int(cnt["accepts"].sum())
    assert s.reps_exhausted == int((cnt["status"] == 1).sum()) == 0 and s.stack_overflows == 0


# ------------------------------------------------------------------ any hit
def _shadow_rays(shape, t=2.0):
    """Shadow rays long enough (|t| = 2 from z = 1) to reach the chain's triangle at z = 0."""
    n, o, d = _rays_of(shape)
    return n, hb.shadow_rays(o, d, [t] * n)


def _shadow_pair(engine, sc, n, rays):
    got, want = rays.copy(), rays.copy()
    vg, vc = np.full((n, 4), 7.0, np.float32), np.full((n, 4), 7.0, np.float32)
    s, st_g = engine.trace_shadow(got, n, 0, n, 1, visibility=vg, check=False)
    st_c, cnt = O.shadow(sc, want, n, 0, n, 1, visibility=vc, counts=True)
    return got, want, vg, vc, s, st_g, st_c, cnt


@pytest.mark.parametrize("shape", SHAPES)
def test_shadow_depth16_records(engine, chain16, shape):
    n, rays = _shadow_rays(shape)
    engine.upload(chain16)
    got, want, vg, vc, _, st_g, st_c, cnt = _shadow_pair(engine, chain16, n, rays)
    assert st_g == 0 and st_c == 0 and int(cnt["max_stack"].max()) == 16
    live = np.ones(n, bool)
    if shape == "odd_lanes_live":
        live[0::2] = False
    assert (cnt["status"][live] == 4).all() and (cnt["status"][~live] == 0).all()  # occluded / reached |t|
    assert same_floats(got["t"], want["t"]) and same_floats(vg, vc)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_shadow_depth16_short_rays_pop_every_entry(engine, chain16):
    """|t| = 0.5 ends before the chain's leaf box: nothing occludes, and the ray pops all 16 entries (the spilled
    ones included) before it reaches its distance."""
    n, rays = _shadow_rays("full_wave", t=0.5)
    engine.upload(chain16)
    got, want, vg, vc, _, st_g, st_c, cnt = _shadow_pair(engine, chain16, n, rays)
    assert st_g == 0 and st_c == 0 and int(cnt["max_stack"].max()) == 16 and (cnt["status"] == 0).all()
    assert same_floats(got["t"], want["t"]) and same_floats(vg, vc)


def test_shadow_depth17_full_wave_overflows(engine, chain17):
    n, rays = _shadow_rays("full_wave")
    engine.upload(chain17)
    s, st = engine.trace_shadow(rays.copy(), n, 0, n, 1, visibility=np.full((n, 4), 7.0, np.float32), check=False)
    assert st == tthip.TT_ERR_STACK_OVERFLOW and s.stack_overflows == 64
