"""The checker of the adaptive dequeue order (tests/order_cases.py), on the host: the reference satisfies every
property of the kernel's contract on every case, the case list meets its own conditions, the segment bounds of the
order kernel and of the trace scheduler are one formula, and six wrong orders are each rejected by the comparison
tests/test_gpu_order_pin.py makes (canonical(order) == reference_order)."""
import numpy as np
import pytest

import order_cases as OC


@pytest.fixture(scope="module")
def cases():
    return OC.cases()


def _ref(n_rays, cost, hot):
    return OC.reference_order(cost, n_rays, len(cost), hot)


def _accepted(order, n_rays, cost, hot):
    return np.array_equal(OC.canonical(order, cost, n_rays, len(cost), hot), _ref(n_rays, cost, hot))


def test_segment_bounds_of_both_sources_agree(cases):
    for n in sorted({len(c) for _, _, c, _ in cases} | {0, 1 << 26, (1 << 32) - 1}):
        for s in range(OC.SEGS + 1):
            want = OC.segment_bounds(n, s)
            assert OC.order_kernel_bound(n, s) == want, (n, s)
            if 64 * want < 1 << 32:  # (the scheduler counts in rays: launches hold fewer than 2^32)
                assert OC.scheduler_seg_lo(n, s) == 64 * want, (n, s)
        assert OC.segment_bounds(n, 0) == 0 and OC.segment_bounds(n, OC.SEGS) == n


def test_case_list_is_the_one_specified(cases):
    assert len(cases) == len(OC.CHUNK_COUNTS) * len(OC.PATTERNS) * 3 * len(OC.HOTS)
    assert {len(c) for _, _, c, _ in cases} == {1, 7, 8, 9, 63, 640, 16384, 16395, 32400, 49157}
    for n in OC.CHUNK_COUNTS:
        assert {nr for _, nr, c, _ in cases if len(c) == n} == {64 * n, 64 * n - 1, 64 * n - 63}
    assert {h for _, _, _, h in cases} == {0, 48}
    by_pattern = {}
    for name, _, c, _ in cases:
        by_pattern.setdefault(name.split("-")[0], []).append(c)
    assert all(not c.any() for c in by_pattern["zero"])
    assert all(len(np.unique(c)) == 1 and c[0] != 0 for c in by_pattern["equal"])
    assert all(c.max() <= 1000 for c in by_pattern["uniform"])
    assert max(c.max() for c in by_pattern["uniform"]) == 1000 and min(c.min() for c in by_pattern["uniform"]) == 0
    assert all(set(np.unique(c)) <= {0, 40, 41} for c in by_pattern["three"])
    assert all(np.all(np.diff(c.astype(np.int64)) > 0) for c in by_pattern["ascending"] if len(c) > 1)
    big = [c for c in by_pattern["clamp"] if len(c) >= 63]
    assert all(set(OC.CLAMP_VALUES) <= set(np.unique(c)) for c in big)
    assert all((c < 48).any() and (c > 48).any() for c in big)
    assert all({47, 48, 49} <= set(np.unique(c)) for c in by_pattern["hot_edge"] if len(c) >= 63)


def test_random_patterns_tie_across_rounds(cases):
    """Round stability is only tested where equal keys meet across scatter rounds: in every case of a random
    pattern whose segments span more than one round, at least 25 % of each segment's chunks share their key with
    a chunk of another round."""
    seen = 0
    for name, n_rays, cost, hot in cases:
        n = len(cost)
        if name.split("-")[0] not in OC.RANDOM_PATTERNS or n // OC.SEGS <= OC.ROUND:
            continue
        share = OC.cross_round_share(cost, n_rays, n, hot)
        assert min(share) >= 0.25, (name, share)
        seen += 1
    assert seen == len(OC.RANDOM_PATTERNS) * 4 * 3 * len(OC.HOTS)  # the four counts of 16384 chunks and more


def test_reference_satisfies_every_property(cases):
    for name, n_rays, cost, hot in cases:
        n = len(cost)
        ref = _ref(n_rays, cost, hot)
        assert ref.dtype == np.uint32 and len(ref) == n, name
        assert OC.is_segment_permutation(ref, n), name
        assert OC.keys_non_increasing(ref, cost, n_rays, n, hot), name
        assert OC.round_stable(ref, cost, n_rays, n, hot), name
        assert OC.partial_chunk_last(ref, n_rays, n), name
        assert np.array_equal(OC.canonical(ref, cost, n_rays, n, hot), ref), name  # a fixed point


def test_known_small_orders():
    # one segment per chunk: nothing can move
    c = np.array([5, 900, 0, 41, 41, 7, 1000, 3], np.uint32)
    assert _ref(8 * 64, c, 0).tolist() == list(range(8))
    # 16 chunks, two per segment: each pair longest first, ties and below-`hot` pairs in natural order
    c = np.array([1, 2, 2, 1, 3, 3, 47, 48, 49, 48, 1023, 5000, 0xFFFFFFFF, 1024, 0, 0], np.uint32)
    assert _ref(16 * 64, c, 0).tolist() == [1, 0, 2, 3, 4, 5, 7, 6, 8, 9, 10, 11, 12, 13, 14, 15]
    assert _ref(16 * 64, c, 48).tolist() == [0, 1, 2, 3, 4, 5, 7, 6, 8, 9, 10, 11, 12, 13, 14, 15]
    # ragged: the last chunk is pinned, whatever it cost
    c = np.zeros(16, np.uint32)
    c[15] = 999
    assert _ref(16 * 64 - 1, c, 0).tolist() == list(range(16))
    assert _ref(16 * 64, c, 0).tolist() == list(range(14)) + [15, 14]


def test_canonical_undoes_only_a_permutation_inside_one_round():
    n = 16384 + 11
    cost = OC.make_costs("three", n, np.random.default_rng(3))
    ref = _ref(64 * n, cost, 0)
    key = OC.keys_of(cost, 0)
    lo = OC.segment_bounds(n, 2)
    # reverse one (key, round) run: still accepted
    run = [p for p in range(lo, lo + 600) if key[ref[p]] == 41 and (ref[p] - lo) // OC.ROUND == 0]
    assert len(run) > 10 and run == list(range(run[0], run[-1] + 1))
    w = ref.copy()
    w[run] = ref[run][::-1]
    assert not np.array_equal(w, ref) and _accepted(w, 64 * n, cost, 0)
    assert OC.round_stable(w, cost, 64 * n, n, 0) and OC.keys_non_increasing(w, cost, 64 * n, n, 0)


# ------------------------------------------------------------------ negative controls
@pytest.fixture(scope="module")
def control():
    n = 16384 + 11
    cost = OC.make_costs("uniform", n, np.random.default_rng(11))
    assert len(np.unique(OC.keys_of(cost, 0))) >= 3
    return 64 * n, cost, 0


def test_control_identity_is_rejected(control):
    n_rays, cost, hot = control
    w = np.arange(len(cost), dtype=np.uint32)
    assert not _accepted(w, n_rays, cost, hot)
    assert not OC.keys_non_increasing(w, cost, n_rays, len(cost), hot)


def test_control_ascending_is_rejected(control):
    n_rays, cost, hot = control
    n = len(cost)
    key = OC.keys_of(cost, hot)
    w = np.arange(n, dtype=np.uint32)
    for s in range(OC.SEGS):
        lo, hi = OC.segment_bounds(n, s), OC.segment_bounds(n, s + 1)
        w[lo:hi] = lo + np.argsort(key[lo:hi], kind="stable")
    assert OC.is_segment_permutation(w, n)
    assert not _accepted(w, n_rays, cost, hot)
    assert not OC.keys_non_increasing(w, cost, n_rays, n, hot)


def test_control_duplicate_is_rejected(control):
    n_rays, cost, hot = control
    w = _ref(n_rays, cost, hot)
    w[5] = w[6]
    assert not _accepted(w, n_rays, cost, hot)
    assert not OC.is_segment_permutation(w, len(cost))


def test_control_swap_across_a_segment_boundary_is_rejected(control):
    n_rays, cost, hot = control
    n = len(cost)
    w = _ref(n_rays, cost, hot)
    b = OC.segment_bounds(n, 3)
    w[b - 1], w[b] = w[b], w[b - 1]
    assert not _accepted(w, n_rays, cost, hot)
    assert not OC.is_segment_permutation(w, n)
    # also when the two have equal keys (sorting by another segment's costs can do that)
    key = OC.keys_of(cost, hot)
    ref = _ref(n_rays, cost, hot)
    lo, hi = OC.segment_bounds(n, 2), OC.segment_bounds(n, 4)
    p = next(p for p in range(lo, b) if np.any(key[ref[b:hi]] == key[ref[p]]))
    q = b + int(np.nonzero(key[ref[b:hi]] == key[ref[p]])[0][0])
    w = ref.copy()
    w[p], w[q] = w[q], w[p]
    assert OC.keys_non_increasing(w, cost, n_rays, n, hot)
    assert not _accepted(w, n_rays, cost, hot)


def test_control_equal_keys_of_different_rounds_swapped_is_rejected(control):
    n_rays, cost, hot = control
    n = len(cost)
    ref = _ref(n_rays, cost, hot)
    key = OC.keys_of(cost, hot)
    lo = OC.segment_bounds(n, 1)
    p = next(p for p in range(lo, OC.segment_bounds(n, 2) - 1)
             if key[ref[p]] == key[ref[p + 1]] and (ref[p] - lo) // OC.ROUND != (ref[p + 1] - lo) // OC.ROUND)
    w = ref.copy()
    w[p], w[p + 1] = w[p + 1], w[p]
    assert OC.is_segment_permutation(w, n) and OC.keys_non_increasing(w, cost, n_rays, n, hot)
    assert not _accepted(w, n_rays, cost, hot)
    assert not OC.round_stable(w, cost, n_rays, n, hot)


def test_control_partial_chunk_not_last_is_rejected(control):
    _, cost, hot = control
    n = len(cost)
    cost = cost.copy()
    cost[n - 1] = 1000  # the partial chunk is the segment's longest: a sort that includes it moves it
    n_rays = 64 * n - 5
    w = _ref(64 * n, cost, hot)  # the order of the same costs as whole chunks
    assert w[n - 1] != n - 1
    assert OC.is_segment_permutation(w, n) and OC.keys_non_increasing(w, cost, 64 * n, n, hot)
    assert not _accepted(w, n_rays, cost, hot)
    assert not OC.partial_chunk_last(w, n_rays, n)


# ------------------------------------------------------------------ the cost map's reference
def test_chunk_of_ray_is_the_8x8_tile_of_a_full_frame():
    W, H = 24, 16
    c = OC.chunk_of_ray(W * H, W, H)
    assert c[0] == 0 and c[7] == 0 and c[8] == 1 and c[W * 7 + 23] == 2 and c[W * 8] == 3 and c[W * H - 1] == 5
    assert np.all(np.bincount(c) == 64)
    assert np.array_equal(OC.chunk_of_ray(W * H - 1, W, H), np.arange(W * H - 1) // 64)  # a list: linear
    assert np.array_equal(OC.chunk_of_ray(20 * 12, 20, 12), np.arange(240) // 64)  # sides no multiple of 8


def test_reference_cost_map_threshold_and_overflow():
    dt = np.dtype([("node_visits", "<u4"), ("status", "<u4")])
    cnt = np.zeros(130, dt)
    cnt["node_visits"][:64] = 31  # all cheap: 0
    cnt["node_visits"][64:128] = np.arange(64)
    cnt["node_visits"][70] = 500
    cnt["status"][70] = OC.STATUS_OVERFLOW  # an overflowed ray records nothing
    cnt["node_visits"][128] = 32  # the threshold itself counts
    cnt["node_visits"][129] = 1000
    cnt["status"][129] = 1  # the Reps bound: recorded
    assert OC.reference_cost_map(cnt, 130, 130, 1).tolist() == [0, 63, 1000]
    assert OC.reference_cost_map(cnt, 129, 130, 1).tolist() == [0, 63, 32]
    assert OC.reference_cost_map(cnt, 63, 130, 1).tolist() == [0]
