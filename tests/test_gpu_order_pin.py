"""What the adaptive dequeue order IS (tests/test_gpu_order.py pins that it changes no result): the order kernel
against a host reference, the recorded chunk cost map against the CPU oracle, and the slot state of the dispatcher
through tt_trace_chunk_costs. Everything is integer-exact; no comparison here has a tolerance.

1. tt_order_kernel (csrc/tt_order.hip), driven directly through lib/test/libtt_order_probe.so
   (tests/native/order_probe.hip + the engine's own build/tt_order.o) with the synthetic costs of
   tests/order_cases.py: canonical(order) == reference_order on every case, with guard words around both outputs.

2. The cost map record_chunk_cost (csrc/tt_trace.hip) fills, read back with tt_trace_chunk_costs, against

       cost[m] = max(node_visits[r] for rays r of chunk m with node_visits[r] >= 32 that did not overflow), else 0

   from the oracle's per-ray node_visits (order_cases.reference_cost_map). The call sites of record_chunk_cost:
   - the narrow finish (finish_ray): every case; at 1024x512 the 8192 chunks exceed the resident grid (at most
     26 one-wave blocks per CU by the LDS cap of tt_ctx_create: 2 * (80 KiB / (12 * 64 * 8 B))), so lanes are
     refilled in place and most rays finish there;
   - the wide-drain finish (finish_wide): the 256x160 and smaller launches, where every wave dequeues one chunk
     and ends in the drain; every one-ray launch;
   - the wide-drain Reps bound (exhaust_wide): the one-ray kat_cases.case_reps_exhausted launch, and rays 128-129
     of test_reps_bound_in_a_full_wave_and_in_the_drain;
   - the narrow Reps bound: rays 0-63 of test_reps_bound_in_a_full_wave_and_in_the_drain -- 64 rays that reach
     the bound in the same iteration of a full wave, which never enters the drain (it needs at most 32 live rays).

3. The ping-pong (OrderSlot, csrc/tt_dispatch.hip): the map a launch fills was last filled two launches earlier
   and only the order kernel clears it; a screen-size change; an unflagged launch in between; a fresh context;
   truncation and refusals of tt_trace_chunk_costs.

Reference figures of the end-to-end cases (CPU oracle; chunks, chunks with nonzero cost, distinct costs, max Reps):
256x160 full frame 640 / 52.8 % / 43 / 87; n = W*H - 1 640 / 76.9 % / 45; n = 4097 65 / 67.7 % / 18; n = 1000
16 / 75.0 % / 7; n = 63 1 / 0 % / 1; 1024x512 8192 / 32.2 % / 50 / 86; IgnoreBackfacing 256x160 640 / 61.7 % / 64.
(Compacted lists cut the frame into 64-pixel row strips, which meet a long ray more often than 8x8 tiles do.)
"""
import ctypes as C
import os

import numpy as np
import pytest

import handbuilt as hb
import kat_cases as K
import oracle_ctypes as O
import order_cases as OC
import tthip
from parity_util import CPU_THREADS, FAR

pytestmark = pytest.mark.gpu

ORD = tthip.TT_TRACE_ADAPTIVE_ORDER
NEAR = 0.05
PROBE_LIB = os.path.join(tthip.LIB_DIR, "test", "libtt_order_probe.so")
PROBE_GUARD = 64
PROBE_GUARD_WORD = 0xC0DEFACE
PROBE_SENTINEL = 0xFFFFFFFF
CAM_A = ((0.3, 0.2, 2.4), (-0.1, -0.05, -1.0))  # test_gpu_order.py's _soup_frame
CAM_B = ((0.9, 0.2, 2.4), (-0.1, -0.05, -1.0))  # shifted: 37 % of the 256x160 tiles cost more from A than from B
# Generate's jitter sample (frames_accumulated) of the 256x160 frames. Chosen on the CPU oracle, as CAM_B was: a
# compacted list's chunks are 64-pixel strips of the frame's top rows, most of which meet a long ray, and the share
# of the 4097-ray list's 65 chunks with cost 0 moves between 20 % and 32 % with the sample (sample 0: 23.1 %). The
# test asks for 25 % on the reference; sample 11 gives 32.3 % (21 chunks), with the full frame's figures unchanged.
FRAME_256 = 11

_CACHE = {}


# ------------------------------------------------------------------ 1. the order kernel
def _probe():
    assert os.path.exists(PROBE_LIB), "build() makes lib/test/libtt_order_probe.so"
    L = C.CDLL(PROBE_LIB)
    vp, u32 = C.c_void_p, C.c_uint32
    L.tt_order_probe.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp]
    L.tt_order_probe.restype = C.c_int
    return L


def test_order_kernel_matches_reference(engine):
    L = _probe()
    refs = {}
    for name, n_rays, cost, hot in OC.cases():
        n = len(cost)
        cost_in = cost.copy()
        order = np.zeros(n, np.uint32)
        clear = np.full(n, 0xDEADBEEF, np.uint32)  # the map the coming trace fills: never zero before the kernel
        cost_after = np.zeros(n, np.uint32)
        guards = np.zeros(4 * PROBE_GUARD, np.uint32)
        err = L.tt_order_probe(cost_in.ctypes.data, n_rays, n, hot, order.ctypes.data, clear.ctypes.data,
                               cost_after.ctypes.data, guards.ctypes.data)
        assert err == 0, f"{name}: hipError_t {err}"
        assert np.all(guards == PROBE_GUARD_WORD), f"{name}: guard regions {np.nonzero(guards != PROBE_GUARD_WORD)[0]}"
        assert np.array_equal(cost_after, cost) and np.array_equal(cost_in, cost), f"{name}: the input costs changed"
        assert not clear.any(), f"{name}: cost_clear[{np.nonzero(clear)[0][:5]}] not zeroed"
        assert not np.any(order == PROBE_SENTINEL), f"{name}: order entries never written"
        assert OC.is_segment_permutation(order, n), f"{name}: not a permutation of every segment onto itself"
        key = (id(cost), n_rays, hot)
        if key not in refs:
            refs[key] = OC.reference_order(cost, n_rays, n, hot)
        canon = OC.canonical(order, cost, n_rays, n, hot)
        if not np.array_equal(canon, refs[key]):
            bad = np.nonzero(canon != refs[key])[0]
            pytest.fail(f"{name}: canonical(order) != reference_order at {len(bad)} positions, first {bad[:5]}: "
                        f"{canon[bad[:5]]} vs {refs[key][bad[:5]]}; keys non-increasing "
                        f"{OC.keys_non_increasing(order, cost, n_rays, n, hot)}, round-stable "
                        f"{OC.round_stable(order, cost, n_rays, n, hot)}, partial chunk last "
                        f"{OC.partial_chunk_last(order, n_rays, n)}")


# ------------------------------------------------------------------ 2. the recorded cost map
def _scene():
    if "scene" not in _CACHE:
        _CACHE["scene"] = tthip.single_object_scene(tthip.Mesh.soup(41, 30000, 1.0, 0.1))
    return _CACHE["scene"]


def _frame(engine, W, H, cam=CAM_A, frames=0):
    """Generate's rays of the frame: (device buffer of 2 W H RayData, its host copy)."""
    import torch

    c2w, ip = tthip.unity_camera(cam[0], cam[1], (0, 1, 0), 60.0, W, H, NEAR, FAR)
    base = torch.zeros(2 * W * H * 48, dtype=torch.uint8, device=torch.device("cuda:0"))
    engine.generate(base, c2w, ip, W, H, NEAR, FAR, jitter=1, frames=frames, max_bounce=2, device=True)
    torch.cuda.synchronize()
    return base, _host(base)


def _host(base):
    return base.cpu().numpy().view(tthip.RAY_DTYPE).copy()


def _reference(sc, host, n, bounce, W, H, flags=0):
    """The oracle's cost map of the launch (the rays stay as they are: the oracle runs on a copy)."""
    st, cnt = O.trace(sc, host.copy(), n, bounce, FAR, W, H, flags=flags, counts=True, nthreads=CPU_THREADS)
    assert st == 0
    return OC.reference_cost_map(cnt, n, W, H), cnt


def _flagged(engine, base, n, bounce, W, H, extra=0):
    """One TT_TRACE_ADAPTIVE_ORDER launch on a fresh clone of the rays; the cost map read back after it."""
    import torch

    engine.trace(base.clone(), n, bounce, FAR, W, H, device=True, flags=ORD | extra)
    torch.cuda.synchronize()
    return engine.chunk_costs(bounce)


def _assert_map(got, want, tag):
    assert got.dtype == np.uint32 and got.shape == want.shape, f"{tag}: {got.shape} entries, expected {want.shape}"
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (f"{tag}: {len(bad)} of {len(want)} chunk costs differ, first at {bad[:8]}: "
                           f"{got[bad[:8]]} vs the oracle's {want[bad[:8]]}")


def _figures(ref):
    return float(np.mean(ref > 0)), float(np.mean(ref == 0)), len(np.unique(ref))


def _assert_not_vacuous(ref, tag):
    """Conditions on the REFERENCE, so that an equal map means something: long and cheap chunks both common,
    many distinct costs."""
    nonzero, zero, distinct = _figures(ref)
    print(f"{tag}: {len(ref)} chunks, {100 * nonzero:.1f} % nonzero, {distinct} distinct costs, max {ref.max()}")
    assert nonzero >= 0.25, f"{tag}: only {100 * nonzero:.1f} % of the reference's chunks have a cost"
    assert zero >= 0.25, f"{tag}: only {100 * zero:.1f} % of the reference's chunks have cost 0"
    assert distinct >= 10, f"{tag}: only {distinct} distinct costs in the reference"


def _soup_256(engine):
    sc = _scene()
    engine.upload(sc)
    if "256" not in _CACHE:
        _CACHE["256"] = _frame(engine, 256, 160, frames=FRAME_256)
    return (sc,) + _CACHE["256"]


@pytest.mark.parametrize("n", [256 * 160, 256 * 160 - 1, 4097, 1000, 63])
def test_cost_map_256x160(engine, n):
    """Bounce 0 on the soup: the full frame (8x8 tiles), then compacted lists (ray // 64), ragged ones included. Three
    flagged launches each -- the first records (or sorts by what an earlier test left: a hint), the next two dequeue in
    the sorted order -- and the map after each is the same reference: costs do not depend on the dequeue order."""
    W, H = 256, 160
    sc, base, host = _soup_256(engine)
    ref, cnt = _reference(sc, host, n, 0, W, H)
    assert len(ref) == (n + 63) // 64
    if n == W * H:
        assert 0.2 < np.mean(cnt["node_visits"] >= OC.MIN_REPS) < 0.35  # (26 % of the rays reach the threshold)
    if n in (W * H, 4097):
        _assert_not_vacuous(ref, f"256x160 n={n}")
    elif n == 63:
        assert not ref.any()  # a legitimate all-cheap chunk
    else:
        assert ref.any() and not ref.all()
    for k in range(3):
        _assert_map(_flagged(engine, base, n, 0, W, H), ref, f"n={n} launch {k}")


def test_cost_map_1024x512_more_chunks_than_waves(engine):
    """8192 chunks on a grid that holds fewer waves: lanes are refilled in place and rays finish in the narrow loop."""
    import torch

    # tt_ctx_create sizes grid_of[12..17] as CUs * min(occupancy, LDS cap, 32): the LDS cap alone is
    # 2 * (80 KiB // (TT_LDS_STACK 12 * TT_BLOCK 64 * 8 B)) = 26 one-wave blocks per CU
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, H = 1024, 512
    assert cus * 2 * ((80 * 1024) // (12 * 64 * 8)) < W * H // 64
    sc = _scene()
    engine.upload(sc)
    base, host = _frame(engine, W, H)
    ref, _ = _reference(sc, host, W * H, 0, W, H)
    assert len(ref) == 8192
    _assert_not_vacuous(ref, "1024x512")
    for k in range(2):
        _assert_map(_flagged(engine, base, W * H, 0, W, H), ref, f"1024x512 launch {k}")


def test_cost_map_material_check_kernel(engine):
    """tt_trace_kernel_ord_mat: IgnoreBackfacing at bounce 0, the oracle with the same flag."""
    W, H = 256, 160
    sc, base, host = _soup_256(engine)
    flag = tthip.TT_TRACE_IGNORE_BACKFACING
    ref, _ = _reference(sc, host, W * H, 0, W, H, flags=flag)
    plain, _ = _reference(sc, host, W * H, 0, W, H)
    assert np.mean(ref != plain) > 0.1  # the flag changes the costs: the right instantiation is compared
    _assert_not_vacuous(ref, "256x160 IgnoreBackfacing")
    for k in range(3):
        _assert_map(_flagged(engine, base, W * H, 0, W, H, extra=flag), ref, f"IgnoreBackfacing launch {k}")


def test_cost_map_bounce_1_has_a_slot_of_its_own(engine):
    """The compacted survivors of a 200x120 frame at bounce 1: linear chunks, records in the odd half of the buffer,
    costs in slot 1 -- and slot 0 still holds the primary launch's map."""
    W, H = 200, 120
    WH = W * H
    sc = _scene()
    engine.upload(sc)
    base, host = _frame(engine, W, H, frames=2)
    ref0, _ = _reference(sc, host, WH, 0, W, H)
    _assert_not_vacuous(ref0, "200x120 bounce 0")
    engine.trace(base, WH, 0, FAR, W, H, device=True, flags=ORD)  # in place: the enqueue reads the hit records
    _assert_map(engine.chunk_costs(0), ref0, "bounce 0")
    nb = engine.enqueue_bounce(base, WH, 0, FAR, W, H, frames=2, max_bounce=2, device=True)
    assert 64 < nb < WH
    ref1, _ = _reference(sc, _host(base), nb, 1, W, H)
    assert len(ref1) == (nb + 63) // 64 and ref1.any() and len(ref1) != len(ref0)
    for k in range(3):
        _assert_map(_flagged(engine, base, nb, 1, W, H), ref1, f"bounce 1 launch {k}")
        _assert_map(engine.chunk_costs(0), ref0, f"bounce 0 after bounce-1 launch {k}")


def _kat_launches(engine, sc, rays, n, W, H, status=0):
    """Two flagged launches of a hand-built case from host rays (the second in the first's order); returns the map
    after each and the oracle's counts."""
    engine.upload(sc)
    maps = []
    for _ in range(2):
        st = engine.trace(rays.copy(), n, 0, FAR, W, H, flags=ORD, check=False)[1]
        assert st == status, engine.L.tt_last_error(engine.h).decode()
        maps.append(engine.chunk_costs(0))
    _, cnt = O.trace(sc, rays.copy(), n, 0, FAR, W, H, counts=True)
    return maps, cnt


def test_known_answer_rays(engine):
    # the Reps bound: the cost is the loop bound, recorded although the ray writes no hit
    _, sc, rays, n, _ = K.case_reps_exhausted()
    maps, cnt = _kat_launches(engine, sc, rays, n, 1, 1)
    assert cnt["status"][0] == 1 and cnt["node_visits"][0] == 1000
    for m in maps:
        _assert_map(m, np.array([cnt["node_visits"][0]], np.uint32), "reps_exhausted")
    # the longest ray that still finishes: the exact count
    _, sc, rays, n, _ = K.case_chain_within_bound()
    maps, cnt = _kat_launches(engine, sc, rays, n, 1, 1)
    assert cnt["status"][0] == 0 and cnt["node_visits"][0] == 1000
    for m in maps:
        _assert_map(m, np.array([cnt["node_visits"][0]], np.uint32), "chain_within_bound")
    # a stack overflow: reported, and nothing recorded
    sc, rays = K.stack_overflow_scene(17)
    maps, cnt = _kat_launches(engine, sc, rays, 1, 1, 1, status=tthip.TT_ERR_STACK_OVERFLOW)
    assert cnt["status"][0] == OC.STATUS_OVERFLOW
    for m in maps:
        _assert_map(m, np.zeros(1, np.uint32), "stack overflow")


def test_reps_bound_in_a_full_wave_and_in_the_drain(engine):
    """130 rays on the 1001-node chain: rays 0-63 all go down the chain and reach the Reps bound in the same iteration
    of a full wave (the narrow loop's bound: the drain takes at most 32 live rays), rays 64-127 miss at the root
    (cost 0), rays 128-129 go down the chain as two live lanes of a wave (the drain's bound)."""
    _, sc, _, _, _ = K.case_reps_exhausted()
    n = 130
    o, d = [(0.25, 0.25, 1000.0)] * n, [(0.0, 0.0, 1.0)] * n
    for i in list(range(64)) + [128, 129]:
        o[i], d[i] = (0.25, 0.25, 1.0), (0.0, 0.0, -1.0)
    rays = hb.rays_buffer(o, d, FAR)
    maps, cnt = _kat_launches(engine, sc, rays, n, n, 1)
    ref = OC.reference_cost_map(cnt, n, n, 1)
    assert ref.tolist() == [1000, 0, 1000]
    for m in maps:
        _assert_map(m, ref, "reps bound")


def _long_overflow_scene(chain=40, depth=17):
    """kat_cases.stack_overflow_scene below a chain of `chain` one-child nodes: the ray has made more than
    TT_ORDER_MIN_REPS node visits when its stack overflows."""
    E6 = K.E6
    nodes = [hb.make_node((-1.0, -1.0, -1.0), (E6, E6, E6), i + 1, 0, [(0, "inner", (0, 0, 0), (255, 255, 255), 0)])
             for i in range(chain)]
    for i in range(depth):
        nodes.append(hb.make_node((-1.0, -1.0, -1.0), (E6, E6, E6), chain + 2 * i + 1, 0,
                                  [(0, "inner", (0, 0, 0), (255, 255, 255), 0),
                                   (1, "inner", (0, 0, 0), (255, 255, 255), 1)]))
        nodes.append(hb.make_node((-1.0, -1.0, -1.0), (E6, E6, E6), 0, 0, []))
    nodes.append(K._leaf_root())
    return hb.scene(nodes, [K.UNIT_TRI])


@pytest.mark.parametrize("n", [1, 64])
def test_an_overflowed_ray_records_nothing_however_long(engine, n):
    """A ray that overflows the stack after 32 node visits or more: no cost, in the drain (one ray) as in the narrow
    loop (a full wave of them) -- an overflowed ray has no count worth sorting by, and the map must not depend on
    which loop a ray happened to end in."""
    sc = _long_overflow_scene()
    rays = hb.rays_buffer([(0.25, 0.25, 1.0)] * n, [(0.0, 0.0, -1.0)] * n, FAR)
    maps, cnt = _kat_launches(engine, sc, rays, n, n, 1, status=tthip.TT_ERR_STACK_OVERFLOW)
    assert np.all(cnt["status"] == OC.STATUS_OVERFLOW) and np.all(cnt["node_visits"] >= OC.MIN_REPS)
    for m in maps:
        _assert_map(m, np.zeros(1, np.uint32), f"{n} overflowing rays")


# ------------------------------------------------------------------ 3. the ping-pong and the slot state
def test_stale_costs_are_cleared(engine):
    """L1 (camera A), L2, L3 (camera B): L3 fills the map L1 filled, which only the order kernel clears. Were the
    clear lost, the tiles that cost more from A would keep A's cost (an atomic max over old frames)."""
    W, H = 256, 160
    sc, base_a, host_a = _soup_256(engine)
    base_b, host_b = _frame(engine, W, H, cam=CAM_B, frames=FRAME_256)
    ref_a, _ = _reference(sc, host_a, W * H, 0, W, H)
    ref_b, _ = _reference(sc, host_b, W * H, 0, W, H)
    assert np.mean(ref_a > ref_b) >= 0.10  # else a missing clear could hide
    _assert_map(_flagged(engine, base_a, W * H, 0, W, H), ref_a, "L1 (A)")
    _assert_map(_flagged(engine, base_a, W * H, 0, W, H), ref_a, "L2 (A)")
    _assert_map(_flagged(engine, base_b, W * H, 0, W, H), ref_b, "L3 (B)")
    _assert_map(_flagged(engine, base_b, W * H, 0, W, H), ref_b, "L4 (B): the map L2 filled")
    # the same with ragged lists of different lengths on the same screen: the shorter map after the longer one
    n1, n2 = W * H - 1, 4097
    r1, _ = _reference(sc, host_a, n1, 0, W, H)
    r2, _ = _reference(sc, host_b, n2, 0, W, H)
    for k in range(2):
        _assert_map(_flagged(engine, base_a, n1, 0, W, H), r1, f"list A {k}")
    for k in range(2):
        _assert_map(_flagged(engine, base_b, n2, 0, W, H), r2, f"list B {k}")


def test_screen_size_change_on_the_same_slot(engine):
    sc = _scene()
    engine.upload(sc)
    for W, H in ((200, 120), (120, 96), (200, 120)):
        base, host = _frame(engine, W, H)
        ref, _ = _reference(sc, host, W * H, 0, W, H)
        assert len(ref) == W * H // 64 and ref.any()
        _assert_map(_flagged(engine, base, W * H, 0, W, H), ref, f"{W}x{H} first launch")
        _assert_map(_flagged(engine, base, W * H, 0, W, H), ref, f"{W}x{H} second launch")


def test_unflagged_launch_leaves_the_map(engine):
    import torch

    W, H = 256, 160
    sc, base, host = _soup_256(engine)
    base_b, host_b = _frame(engine, W, H, cam=CAM_B, frames=FRAME_256)
    ref, _ = _reference(sc, host, W * H, 0, W, H)
    ref_b, _ = _reference(sc, host_b, W * H, 0, W, H)
    _assert_map(_flagged(engine, base, W * H, 0, W, H), ref, "flagged")
    engine.trace(base_b.clone(), W * H, 0, FAR, W, H, device=True)  # other rays, no flag: records nothing
    engine.trace(base_b.clone(), 4097, 0, FAR, W, H, device=True)
    torch.cuda.synchronize()
    _assert_map(engine.chunk_costs(0), ref, "after two unflagged launches")
    _assert_map(_flagged(engine, base_b, W * H, 0, W, H), ref_b, "flagged again")


def test_fresh_context_has_no_map(engine):
    e2 = tthip.Engine(0)
    try:
        for bounce in (0, 1, 7, 100):
            assert len(e2.chunk_costs(bounce)) == 0
    finally:
        e2.close()


def test_chunk_costs_truncation_and_refusals(engine):
    W, H = 256, 160
    sc, base, host = _soup_256(engine)
    ref, _ = _reference(sc, host, W * H, 0, W, H)
    _assert_map(_flagged(engine, base, W * H, 0, W, H), ref, "flagged")
    call, h = engine.L.tt_trace_chunk_costs, engine.h
    n = C.c_uint32(12345)
    out = np.full(128, 0xA5A5A5A5, np.uint32)
    assert call(h, 0, out.ctypes.data, 100, C.byref(n)) == tthip.TT_OK  # max below the chunk count: truncated
    assert n.value == 100 and np.array_equal(out[:100], ref[:100]) and np.all(out[100:] == 0xA5A5A5A5)
    out = np.full(1024, 0xA5A5A5A5, np.uint32)
    assert call(h, 0, out.ctypes.data, 1024, C.byref(n)) == tthip.TT_OK  # max above it: the chunk count
    assert n.value == 640 and np.array_equal(out[:640], ref) and np.all(out[640:] == 0xA5A5A5A5)
    n.value = 12345
    assert call(h, 0, None, 0, C.byref(n)) == tthip.TT_OK and n.value == 0  # max == 0 with null costs
    bad = tthip.TT_ERR_INVALID_ARG
    assert call(None, 0, out.ctypes.data, 8, C.byref(n)) == bad
    assert call(h, 0, out.ctypes.data, 8, None) == bad
    assert call(h, 0, None, 8, C.byref(n)) == bad
    assert call(h, -1, out.ctypes.data, 8, C.byref(n)) == bad
    _assert_map(engine.chunk_costs(0), ref, "after the refusals")
