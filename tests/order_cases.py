"""Host-only reference for the adaptive dequeue order (csrc/tt_order.hip) and the chunk cost map it sorts by
(record_chunk_cost, csrc/tt_trace.hip): plain numpy, no GPU, no library of the package.

The order kernel's contract (its header comment): per scheduler segment, the chunks sorted by descending key with
chunks of equal key in their natural order "up to a permutation inside one round" of 256 consecutive chunks; a
launch whose ray count is no multiple of 64 keeps its partial last chunk last. In this module's terms:

    canonical(gpu_order, cost, n_rays, n_chunks, hot) == reference_order(cost, n_rays, n_chunks, hot)

reference_order is a stable sort; canonical sorts every run of consecutive entries that share (segment, key, round)
ascending, which undoes exactly the freedom the contract leaves and nothing else (two equal-key entries of different
rounds in the wrong order stay in the wrong order, an entry in the wrong segment stays there).

The cost map's reference (reference_cost_map) is the oracle's per-ray node_visits -- the reference loop's Reps --
folded per 64-ray chunk.
"""
import numpy as np

SEGS = 8           # TT_SEGS: scheduler segments, one order-kernel block each
ROUND = 256        # OB: chunks of one scatter round
KEYS = 1024        # OKEYS: cost buckets; costs of 1023 and more share the last one
MIN_REPS = 32      # TT_ORDER_MIN_REPS's documented value: rays below it record nothing
STATUS_OVERFLOW = 2  # oracle counts.status of a ray that overflowed the traversal stack

CHUNK_COUNTS = (1, 7, 8, 9, 63, 640, 16384, 16384 + 11, 32400, 3 * 16384 + 5)
HOTS = (0, 48)
PATTERNS = ("zero", "equal", "uniform", "three", "ascending", "ramp", "clamp", "hot_edge")
RANDOM_PATTERNS = ("uniform", "three", "clamp", "hot_edge")
CLAMP_VALUES = (1023, 1024, 5000, 0xFFFFFFFF)
HOT_EDGE_VALUES = (0, 46, 47, 48, 49, 50, 200)


# ------------------------------------------------------------------ segments
def segment_bounds(n_chunks, s):
    """First chunk of segment s (s = SEGS: one past the last chunk), in exact integer arithmetic."""
    return int(n_chunks) * int(s) // SEGS


def order_kernel_bound(n_chunks, s):
    """tt_order.hip's `(uint32_t)((uint64_t)A.n_chunks * s / TT_SEGS)`, operation by operation."""
    with np.errstate(over="ignore"):
        return int(np.uint32(np.uint64(np.uint32(n_chunks)) * np.uint64(s) // np.uint64(SEGS)))


def scheduler_seg_lo(n_tiles, seg):
    """tt_traverse.h's seg_lo: `(uint32_t)(((uint64_t)n_tiles * seg / TT_SEGS) << 6)`, in rays."""
    with np.errstate(over="ignore"):
        v = (np.uint64(np.uint32(n_tiles)) * np.uint64(seg) // np.uint64(SEGS)) << np.uint64(6)
        return int(np.uint32(v & np.uint64(0xFFFFFFFF)))


def _sorted_bounds(n_rays, n_chunks):
    """[(lo, hi)] per segment: the chunks the kernel sorts (the partial last chunk excluded)."""
    out = []
    for s in range(SEGS):
        lo, hi = segment_bounds(n_chunks, s), segment_bounds(n_chunks, s + 1)
        if s == SEGS - 1 and n_rays % 64 != 0 and hi > lo:
            hi -= 1
        out.append((lo, hi))
    return out


def keys_of(cost, hot):
    c = np.asarray(cost, np.uint32).astype(np.int64)
    return np.where(c < int(hot), 0, np.minimum(c, KEYS - 1))


# ------------------------------------------------------------------ the order
def reference_order(cost, n_rays, n_chunks, hot):
    key = keys_of(cost, hot)
    order = np.arange(n_chunks, dtype=np.uint32)  # (the pinned partial chunk keeps its own index)
    for lo, hi in _sorted_bounds(n_rays, n_chunks):
        if hi > lo:
            order[lo:hi] = lo + np.argsort(-key[lo:hi], kind="stable")
    return order


def _position_fields(order, cost, n_rays, n_chunks, hot):
    """Per position p of `order`: (segment of p, key of the entry, scatter round of the entry, sorted part?).
    An entry that is no chunk index gets key -1 and a round of its own, so nothing groups with it."""
    order = np.asarray(order, np.uint32).astype(np.int64)
    key = keys_of(cost, hot)
    seg = np.zeros(n_chunks, np.int64)
    lo_of = np.zeros(n_chunks, np.int64)
    part = np.zeros(n_chunks, bool)
    for s, (lo, hi) in enumerate(_sorted_bounds(n_rays, n_chunks)):
        full_hi = segment_bounds(n_chunks, s + 1)
        seg[lo:full_hi] = s
        lo_of[lo:full_hi] = lo
        part[lo:hi] = True
    valid = order < n_chunks
    k = np.where(valid, key[np.minimum(order, n_chunks - 1)], -1)
    r = np.where(valid, (order - lo_of) // ROUND, -2 - np.arange(n_chunks))
    return order, seg, k, r, part


def canonical(order, cost, n_rays, n_chunks, hot):
    """`order` with every run of consecutive entries of one (segment, key, round) sorted ascending."""
    order, seg, k, r, part = _position_fields(order, cost, n_rays, n_chunks, hot)
    if n_chunks == 0:
        return order.astype(np.uint32)
    new = np.ones(n_chunks, bool)
    new[1:] = (seg[1:] != seg[:-1]) | (k[1:] != k[:-1]) | (r[1:] != r[:-1]) | (part[1:] != part[:-1])
    gid = np.cumsum(new)
    return order[np.lexsort((order, gid))].astype(np.uint32)


def is_segment_permutation(order, n_chunks):
    """Every segment's positions hold exactly the segment's chunk indices."""
    order = np.asarray(order, np.uint32).astype(np.int64)
    if len(order) != n_chunks:
        return False
    for s in range(SEGS):
        lo, hi = segment_bounds(n_chunks, s), segment_bounds(n_chunks, s + 1)
        if not np.array_equal(np.sort(order[lo:hi]), np.arange(lo, hi)):
            return False
    return True


def keys_non_increasing(order, cost, n_rays, n_chunks, hot):
    _, seg, k, _, part = _position_fields(order, cost, n_rays, n_chunks, hot)
    inside = (seg[1:] == seg[:-1]) & part[1:] & part[:-1]
    return bool(np.all(k[1:][inside] <= k[:-1][inside]))


def round_stable(order, cost, n_rays, n_chunks, hot):
    """Inside a run of equal key, the scatter rounds never go backwards."""
    _, seg, k, r, part = _position_fields(order, cost, n_rays, n_chunks, hot)
    inside = (seg[1:] == seg[:-1]) & part[1:] & part[:-1] & (k[1:] == k[:-1])
    return bool(np.all(r[1:][inside] >= r[:-1][inside]))


def partial_chunk_last(order, n_rays, n_chunks):
    return n_rays % 64 == 0 or n_chunks == 0 or int(np.asarray(order)[n_chunks - 1]) == n_chunks - 1


def cross_round_share(cost, n_rays, n_chunks, hot):
    """Per segment: the fraction of its sorted chunks whose key also occurs in another scatter round."""
    key = keys_of(cost, hot)
    out = []
    for lo, hi in _sorted_bounds(n_rays, n_chunks):
        if hi <= lo:
            out.append(0.0)
            continue
        k = key[lo:hi]
        r = np.arange(hi - lo) // ROUND
        n_rounds = int(r[-1]) + 1
        pairs = np.unique(k * n_rounds + r)
        rounds_of_key = np.bincount(pairs // n_rounds, minlength=KEYS)
        out.append(float(np.mean(rounds_of_key[k] >= 2)))
    return out


# ------------------------------------------------------------------ the case list
def make_costs(pattern, n, rng):
    if pattern == "zero":
        return np.zeros(n, np.uint32)
    if pattern == "equal":
        return np.full(n, 77, np.uint32)
    if pattern == "uniform":
        return rng.integers(0, 1001, n).astype(np.uint32)
    if pattern == "three":
        return rng.choice(np.array([0, 40, 41], np.uint32), n)
    if pattern == "ascending":  # strictly ascending: the keys reverse up to the clamp bucket, which stays stable
        return np.arange(n, dtype=np.uint32)
    if pattern == "ramp":  # ascending inside every segment over 1..1000: a reversal at the large counts too
        c = np.zeros(n, np.uint32)
        for s in range(SEGS):
            lo, hi = segment_bounds(n, s), segment_bounds(n, s + 1)
            if hi > lo:
                c[lo:hi] = 1 + (np.arange(hi - lo, dtype=np.int64) * 1000) // (hi - lo)
        return c
    if pattern == "clamp":
        c = rng.integers(0, 1001, n).astype(np.uint32)
        special = rng.random(n) < 0.25
        c[special] = rng.choice(np.array(CLAMP_VALUES, np.uint32), int(special.sum()))
        return c
    if pattern == "hot_edge":
        return rng.choice(np.array(HOT_EDGE_VALUES, np.uint32), n)
    raise ValueError(pattern)


def cases():
    """[(name, n_rays, costs, hot)]: every chunk count x ragged form x cost pattern x hot."""
    rng = np.random.default_rng(20240611)
    out = []
    for n in CHUNK_COUNTS:
        for pattern in PATTERNS:
            cost = make_costs(pattern, n, rng)
            for n_rays in (64 * n, 64 * n - 1, 64 * n - 63):
                for hot in HOTS:
                    out.append((f"{pattern}-{n}-{n_rays - 64 * n}-hot{hot}", n_rays, cost, hot))
    return out


# ------------------------------------------------------------------ the cost map
def chunk_of_ray(n, W, H):
    """Chunk index of rays 0..n-1: the 8x8 pixel tile, row-major over (W/8) x (H/8), for a full frame whose sides
    are multiples of 8 (the launch's tile swizzle); else ray // 64."""
    i = np.arange(n, dtype=np.int64)
    if n == W * H and W % 8 == 0 and H % 8 == 0:
        return (i // W // 8) * (W // 8) + (i % W) // 8
    return i // 64


def reference_cost_map(counts, n, W, H):
    """cost[m] = max node_visits over chunk m's rays with node_visits >= MIN_REPS that did not overflow, else 0."""
    v = counts["node_visits"][:n].astype(np.int64)
    ok = (v >= MIN_REPS) & (counts["status"][:n] != STATUS_OVERFLOW)
    cost = np.zeros((n + 63) // 64, np.uint32)
    np.maximum.at(cost, chunk_of_ray(n, W, H)[ok], v[ok].astype(np.uint32))
    return cost
