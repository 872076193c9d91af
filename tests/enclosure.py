"""Float64 enclosure model for every buffer of 80-byte CWBVH8 nodes: does each quantised slot box hold what lies below it?

Numpy only: no oracle, no library call beyond the dtypes. It reads nodes, triangles, TLASBVH8Indices, _MeshData and
the instance boxes, and restates nothing of the kernels but the node format (decode_nodes in
test_builder.py): origin p (3 float32), exponent bytes e (3), imask, base_child, base_tri, 8 meta bytes, 6 x 8 q bytes.

Decoding. A slot box is p + q * 2^(e - 127) per axis, in float64; exponent byte 0 decodes to scale 0 (the kernels'
`e << 23` is +0.0f). The sum must be exact, or the model would judge its own rounding: q * scale is exact (8 bits times
a power of two), and p + q * scale is exact in one float64 whenever the exponent gap between p and the quantum is
below 29 bits (24 + 29 = 53). Real builds exceed that gap (a prop whose node origin is 3.8e-16, a rounded sine, under
boxes of extent 6), so the sum is kept as TwoSum leaves it: the float64 sum and its exact error term, an unevaluated
pair that IS p + q * scale. The excess is formed from the pair ((t - s) - err; t - s is exact by Sterbenz wherever the
two are close enough for the sign to be in question). The code asserts that the pair is finite, the only way
TwoSum can fail.

Truth. A leaf slot's truth is the exact float64 bounds of the corners p0, p0 + e1, p0 + e2 of its triangles: the
triangle the trace kernels intersect, not the source vertices. An inner slot's truth is the bounds of ALL triangles
below it, never the child's decoded boxes, so one loose level cannot excuse the next. At the TLAS level the items are
TLASBVH8Indices entries and an item's truth is the float32 {BBMax, BBMin} box of the mesh record it names.

Structure, all exact: every item referenced exactly once (and TLASBVH8Indices a permutation of the records); imask ==
(1 << n_inner) - 1; inner metas 24 .. 24 + n_inner - 1 each once with child bits 001; leaf masks in {1, 3, 7} and at
most 24 items per node; every child index inside the walked node range and no node reached twice; qlo <= qhi per
used slot.

Limits. Excess of the truth over a slot box is reported per slot, axis and side in units of
    U = 2^-24 * max(|x|, |p_axis|, 256 * quantum_axis),
x the truth coordinate, quantum = 2^(e - 127). Two roundings can act against enclosure of a triangle: fl(v - p0) when
an edge is stored (|v - p0| <= node extent <= 256 quanta, so at most 2^-24 * 256 * quantum) and fl(x - P) before
floor / ceil (|x - P| <= 256 quanta likewise); the division by a power of two is exact, floor and ceil only move
outwards. Hence LIMIT_TRIS = 2 U. Instance boxes are the float32 inputs themselves, only fl(x - P) remains:
LIMIT_BOXES = 1 U. Neither figure comes from a measurement.

World level (world_level): mesh_aabbs[m] against the float64 world corners of record m's triangles through inv(W2L)
computed in float64. Per world axis r, with L = inv(W2L) (3x3 part and translation t), M, t' those of W2L, c the
per-axis largest |coordinate| of the local triangle bounds and w the world images of that local box's corners,
    mag_r = (|L| c + |t|)_r         (the per-axis magnitude of refit_many_cases.world_box_bound)
    inv_r = max_w (|L| (|M| |w| + |t'|))_r
    limit_r = 2^-24 * ((3 + k) * mag_r + inv_r),   k = 6 for a box the host made, 4 for one the refit kernel wrote.
Derivation, first order in 2^-24, every term a bound on one source of error in the box or in the truth:
  * the box was made from float32 local bounds of the source vertices, but the truth corner p0 + e1 differs from the
    vertex by the rounding of the stored edge, <= 2^-24 |e1| <= 2^-24 * 2 c per axis: 2 mag_r after |L|;
  * the box was made with float32(local_to_world), the truth with the float64 matrix: 1 mag_r;
  * the arithmetic of the box. The host assembly uses the centre / extent form (centre and half extent: 1 between
    them, since |centre| + extent = c; four-term centre sum and three-term extent sum with rounded products: at most
    4 on every term; the final add: 1): k = 6 (HOST_BOX). The refit kernel's pinned corner chain (three fmaf and
    the add, exact min / max) needs k = 4 (KERNEL_BOX). The caller names the source, so neither check is looser than
    its own derivation;
  * W2L is float32(inv(local_to_world)), so inv(W2L) is not local_to_world: with |dM| <= 2^-24 |M|, |dt'| <= 2^-24 |t'|
    and w = L (x - t'), dw = -L dM w - L dt', so |dw| <= 2^-24 |L| (|M| |w| + |t'|) componentwise: inv_r.
A norm-wise bound, 8 * kappa * 2^-24 * mag with kappa = |M|_inf |M^-1|_inf, would be simpler but is not used: the
host box is not the three-fmaf chain (6 roundings, not 4), and the W2L term is taken componentwise (inv_r <= kappa *
max_r mag_r; once kappa multiplies it, it is no longer per axis). For the rotated, uniformly scaled instances of the
tests inv_r is about mag_r, so the limit is near 10 mag_r for a host box and 8 mag_r for a kernel box.
A limit that is not positive and finite, or an excess that is NaN, counts as a failure (ratio inf).
"""
from dataclasses import dataclass, field

import numpy as np

LIMIT_TRIS = 2.0
LIMIT_BOXES = 1.0
LIMIT_WORLD = 1.0  # world_level reports excess / limit_r directly
HOST_BOX, KERNEL_BOX = 6.0, 4.0  # roundings in the arithmetic of a world box, by who made it (module docstring)
U24 = 2.0 ** -24


@dataclass
class Excess:
    node: int
    slot: int
    axis: int
    side: str  # "lo" / "hi"
    excess: float
    U: float

    @property
    def ratio(self):
        return self.excess / self.U if self.U > 0 else float("inf")

    def __str__(self):
        return (f"node {self.node} slot {self.slot} axis {'xyz'[self.axis]} {self.side}: excess {self.excess:.6g} = "
                f"{self.ratio:.4g} U (U = {self.U:.6g})")


@dataclass
class Report:
    what: str
    limit: float
    structure: list = field(default_factory=list)  # (node, slot or -1, text)
    over: list = field(default_factory=list)       # Excess above the limit
    worst: Excess = None                           # the largest ratio seen, above the limit or not
    n_slots: int = 0
    item_slot: np.ndarray = None                   # (n_items, 2): the (node, slot) that references each item, -1 if none
    table: dict = None                             # per judged slot: depth, node, slot, inner, boxes, truth, q bytes

    @property
    def ratio(self):
        return 0.0 if self.worst is None else self.worst.ratio

    def nodes_reported(self):
        return {s[0] for s in self.structure} | {x.node for x in self.over}

    def slots_over(self):
        return {(x.node, x.slot) for x in self.over}

    def ok(self):
        return not self.structure and not self.over

    def describe(self):
        lines = [f"{self.what}: {len(self.structure)} structure errors, {len(self.over)} slot sides above "
                 f"{self.limit} U, worst {self.worst}"]
        lines += [f"  node {n} slot {s}: {t}" for n, s, t in self.structure[:12]]
        lines += [f"  {x}" for x in sorted(self.over, key=lambda x: -x.ratio)[:12]]
        return "\n".join(lines)

    def check(self):
        assert self.ok(), self.describe()
        return self


def _bytes8(words):
    """(N, 2) little-endian uint32 -> (N, 8) bytes: byte k is (word[k >> 2] >> 8 (k & 3)) & 0xFF."""
    w = np.ascontiguousarray(words, "<u4")
    return w.view(np.uint8).reshape(len(w), 8).astype(np.int64)


def _two_sum(a, b, where, what):
    """(s, err) with s + err == a + b exactly (Knuth's TwoSum)."""
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    bad = ~(np.isfinite(s) & np.isfinite(err)) & where
    assert not bad.any(), f"{what}: p + q * 2^(e-127) is not finite at frontier entry {np.argwhere(bad)[0].tolist()}"
    return s, err


def decode(nodes):
    """Fields of a node array as int64 / float64 arrays; the boxes are made by the walk, where the used slots are known."""
    n = np.ascontiguousarray(nodes)
    ei = n["e_imask"].astype(np.int64)
    e = np.stack([(ei >> s) & 0xFF for s in (0, 8, 16)], 1)
    scale = np.where(e == 0, 0.0, np.ldexp(1.0, (e - 127).astype(np.int32)))
    return dict(p=n["p"].astype(np.float64), e=e, scale=scale, imask=ei >> 24, base_child=n["base_child"].astype(np.int64),
                base_tri=n["base_tri"].astype(np.int64), meta=_bytes8(n["meta"]),
                qlo=np.stack([_bytes8(n["qlo_" + a]) for a in "xyz"], 2),
                qhi=np.stack([_bytes8(n["qhi_" + a]) for a in "xyz"], 2))


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def walk(nodes, root, node_lo, node_hi, child_base, item_lo, item_hi, limit, what):
    """The model proper, level by level with arrays. nodes: the whole node array; the tree may use the nodes
    [node_lo, node_hi) only, its root is `root`, a child is node child_base + base_child + rank. An item is number
    base_tri + offset + j of item_lo / item_hi ((n_items, 3) float64 truth bounds)."""
    n_items = len(item_lo)
    rep = Report(what, limit)
    rep.item_slot = np.full((n_items, 2), -1, np.int64)
    refs = np.zeros(n_items, np.int64)
    if not (node_lo <= root < node_hi <= len(nodes)):
        rep.structure.append((int(root), -1, f"root outside the node range [{node_lo}, {node_hi}) of {len(nodes)} nodes"))
        return rep
    visited = np.zeros(node_hi - node_lo, bool)
    visited[root - node_lo] = True
    frontier = np.array([root], np.int64)
    levels = []
    k8 = np.arange(8)
    while frontier.size:
        d = decode(nodes[frontier])
        meta = d["meta"]
        low5, bits = meta & 0x1F, meta >> 5
        inner = (meta & 0x18) == 0x18
        leaf = ~inner & (bits != 0)
        used = inner | leaf
        n_inner = inner.sum(1)

        def err(mask, text, slots=None):
            for i in np.nonzero(mask)[0][:64]:
                rep.structure.append((int(frontier[i]), -1 if slots is None else int(slots[i]), text(i)))

        err(d["imask"] != (1 << n_inner) - 1, lambda i: f"imask {int(d['imask'][i]):#x} with {int(n_inner[i])} inner slots")
        rank_bits = np.where(inner, 1 << np.clip(low5 - 24, 0, 7), 0).sum(1)
        err(rank_bits != (1 << n_inner) - 1, lambda i: f"inner metas {sorted(low5[i][inner[i]].tolist())} are not 24 .. 24 + n_inner - 1")
        bad_bits = inner & (bits != 1)
        err(bad_bits.any(1), lambda i: "inner meta with child bits other than 001", bad_bits.argmax(1))
        bad_mask = leaf & ~np.isin(bits, (1, 3, 7))
        err(bad_mask.any(1), lambda i: f"leaf mask {int(bits[i][bad_mask[i]][0]):#b} not in (1, 3, 7)", bad_mask.argmax(1))
        count = np.where(leaf, _POP8[bits], 0)
        err(count.sum(1) > 24, lambda i: f"{int(count[i].sum())} items in one node")
        bad_q = used[:, :, None] & (d["qlo"] > d["qhi"])
        err(bad_q.any((1, 2)), lambda i: "qlo > qhi", bad_q.any(2).argmax(1))
        # children
        below = (1 << np.clip(low5 - 24, 0, 7)) - 1
        child = child_base + d["base_child"][:, None] + _POP8[d["imask"][:, None] & below]
        in_range = (child >= node_lo) & (child < node_hi)
        bad_child = inner & ~in_range
        err(bad_child.any(1), lambda i: f"child index {int(child[i][bad_child[i]][0])} outside [{node_lo}, {node_hi})", bad_child.argmax(1))
        descend = inner & in_range
        fi, fk = np.nonzero(descend)
        ch = child[fi, fk]
        # a node reached twice (through two slots of this level, or again from a deeper one) is descended once
        first = np.zeros(len(ch), bool)
        first[np.unique(ch, return_index=True)[1]] = True
        again = ~first | visited[ch - node_lo]
        for j in np.nonzero(again)[0][:64]:
            rep.structure.append((int(frontier[fi[j]]), int(fk[j]), f"child {int(ch[j])} is reached twice"))
        descend[fi[again], fk[again]] = False
        visited[ch[~again] - node_lo] = True
        # items
        first_item = d["base_tri"][:, None] + low5
        j3 = np.arange(3)
        idx = first_item[:, :, None] + j3
        want = leaf[:, :, None] & (j3 < count[:, :, None])
        inside = (idx >= 0) & (idx < n_items)
        bad_item = (want & ~inside).any(2)
        err(bad_item.any(1), lambda i: f"item index {int(first_item[i][bad_item[i]][0])} + count outside [0, {n_items})", bad_item.argmax(1))
        have = want & inside
        np.add.at(refs, idx[have], 1)
        a, b, _ = np.nonzero(have)
        rep.item_slot[idx[have], 0], rep.item_slot[idx[have], 1] = frontier[a], b
        safe = np.clip(idx, 0, max(n_items - 1, 0))
        if n_items:
            t_lo = np.where(have[..., None], item_lo[safe], np.inf).min(2)
            t_hi = np.where(have[..., None], item_hi[safe], -np.inf).max(2)
        else:
            t_lo, t_hi = np.full((len(frontier), 8, 3), np.inf), np.full((len(frontier), 8, 3), -np.inf)
        # boxes, exact
        pp = np.broadcast_to(d["p"][:, None, :], d["qlo"].shape)
        sc = d["scale"][:, None, :]
        check = np.broadcast_to(used[:, :, None], d["qlo"].shape)
        b_lo, r_lo = _two_sum(pp, d["qlo"] * sc, check, what)
        b_hi, r_hi = _two_sum(pp, d["qhi"] * sc, check, what)
        levels.append(dict(frontier=frontier, p=pp, quantum=np.broadcast_to(sc, pp.shape), b_lo=b_lo, b_hi=b_hi,
                           r_lo=r_lo, r_hi=r_hi,
                           t_lo=t_lo, t_hi=t_hi, descend=descend, judged=leaf | descend, qlo=d["qlo"], qhi=d["qhi"]))
        frontier = child[descend]  # row-major: the order np.nonzero(descend) gives below
    # truth of the inner slots, bottom up
    for lv, nxt in zip(levels[-2::-1], levels[:0:-1]):
        lv["t_lo"][lv["descend"]] = nxt["t_lo"].min(1)
        lv["t_hi"][lv["descend"]] = nxt["t_hi"].max(1)
    # every judged slot, for the tests that pick a slot to mutate: depth, node, slot, inner, boxes, truth, q bytes
    at = [np.nonzero(lv["judged"]) for lv in levels]
    rep.table = {k: np.concatenate([lv[k][a] for lv, a in zip(levels, at)])
                 for k in ("b_lo", "b_hi", "t_lo", "t_hi", "quantum", "qlo", "qhi")}
    rep.table.update(depth=np.concatenate([np.full(len(a[0]), i) for i, a in enumerate(at)]),
                     node=np.concatenate([lv["frontier"][a[0]] for lv, a in zip(levels, at)]),
                     slot=np.concatenate([a[1] for a in at]),
                     inner=np.concatenate([lv["descend"][a] for lv, a in zip(levels, at)]))
    for i in np.nonzero(refs != 1)[0][:64]:
        n, s = rep.item_slot[i]
        rep.structure.append((int(n), int(s), f"item {int(i)} is referenced {int(refs[i])} times"))
    # excess
    for lv in levels:
        for side, ex, x in (("lo", (lv["b_lo"] - lv["t_lo"]) + lv["r_lo"], lv["t_lo"]),
                            ("hi", (lv["t_hi"] - lv["b_hi"]) - lv["r_hi"], lv["t_hi"])):
            judged = lv["judged"][:, :, None] & np.isfinite(x)
            rep.n_slots += int(judged[:, :, 0].sum()) if side == "lo" else 0
            with np.errstate(invalid="ignore", divide="ignore"):
                U = U24 * np.maximum(np.maximum(np.abs(x), np.abs(lv["p"])), 256.0 * lv["quantum"])
                ratio = np.where(judged & (ex > 0), ex / U, 0.0)
            if not ratio.size or ratio.max() <= 0:
                continue

            def make(i, k, a):
                return Excess(int(lv["frontier"][i]), int(k), int(a), side, float(ex[i, k, a]), float(U[i, k, a]))

            top = make(*np.unravel_index(np.argmax(ratio), ratio.shape))
            if rep.worst is None or top.ratio > rep.worst.ratio:
                rep.worst = top
            for i, k, a in np.argwhere(ratio > limit)[:256]:
                rep.over.append(make(i, k, a))
    return rep


def tri_bounds(tris):
    """Exact float64 bounds of the corners p0, p0 + e1, p0 + e2 of every triangle record: ((n, 3) lo, (n, 3) hi)."""
    c = tri_corners(tris)
    return c.min(1), c.max(1)


def tri_corners(tris):
    p0, e1, e2 = (tris[f].astype(np.float64) for f in ("pos0", "posedge1", "posedge2"))
    return np.stack([p0, p0 + e1, p0 + e2], 1)


def blas(nodes, tris, root=0, node_lo=0, node_hi=None, what="BLAS"):
    """One BLAS whose nodes are nodes[node_lo:node_hi] with child indices relative to node_lo and whose triangles are
    `tris` (the BLAS's own, leaf ordered)."""
    lo, hi = tri_bounds(tris)
    return walk(nodes, root, node_lo, len(nodes) if node_hi is None else node_hi, node_lo, lo, hi, LIMIT_TRIS, what)


def tlas(nodes, tlas_indices, boxes, n_tlas_nodes, what="TLAS"):
    """The TLAS nodes[0:n_tlas_nodes] over TLASBVH8Indices and the (n_mesh, 6) float32 {BBMax, BBMin} instance boxes."""
    idx = np.asarray(tlas_indices, np.int64)
    b = np.asarray(boxes, np.float32).astype(np.float64).reshape(-1, 6)
    n_mesh = len(b)
    ok = (idx >= 0) & (idx < n_mesh)
    safe = np.clip(idx, 0, n_mesh - 1)
    lo = np.where(ok[:, None], b[safe, 3:6], np.inf)
    hi = np.where(ok[:, None], b[safe, 0:3], -np.inf)
    rep = walk(nodes, 0, 0, int(n_tlas_nodes), 0, lo, hi, LIMIT_BOXES, what)
    times = np.bincount(safe[ok], minlength=n_mesh)
    for m in np.nonzero(times != 1)[0][:64]:
        at = np.nonzero(idx == m)[0]
        n, s = rep.item_slot[at[-1]] if len(at) else (-1, -1)
        rep.structure.append((int(n), int(s), f"mesh record {int(m)} is named by {int(times[m])} TLASBVH8Indices entries"))
    for k in np.nonzero(~ok)[0][:64]:
        rep.structure.append((int(rep.item_slot[k, 0]), int(rep.item_slot[k, 1]), f"TLASBVH8Indices[{int(k)}] = {int(idx[k])}"))
    return rep


def _ranges(offsets, total):
    """Per record the end of its range in a concatenated layout: the next larger distinct offset, or the total."""
    starts = np.unique(np.append(np.asarray(offsets, np.int64), total))
    return starts[np.searchsorted(starts, offsets, side="right")]


def scene(nodes, tris, tlas_indices, meshdata, boxes, n_tlas_nodes, what="scene"):
    """The whole scene from the TLAS root through every record's BLAS: {name: Report}. A BLAS may use only the nodes
    and triangles between its record's NodeOffset / TriOffset and the next BLAS's."""
    out = {"tlas": tlas(nodes, tlas_indices, boxes, n_tlas_nodes, what + ": TLAS")}
    no, to = meshdata["NodeOffset"].astype(np.int64), meshdata["TriOffset"].astype(np.int64)
    root = meshdata["mesh_data_bvh_offsets"].astype(np.int64) & 0x7FFFFFFF
    n_end, t_end = _ranges(no, len(nodes)), _ranges(to, len(tris))
    seen = {}
    for m in range(len(meshdata)):
        key = (int(no[m]), int(to[m]), int(root[m]))
        if key in seen:
            continue
        seen[key] = m
        name = f"{what}: BLAS of record {m}"
        if not (int(n_tlas_nodes) <= no[m] < n_end[m] and 0 <= to[m] <= t_end[m]):
            rep = Report(name, LIMIT_TRIS)
            rep.structure.append((int(no[m]), -1, f"NodeOffset {int(no[m])} / TriOffset {int(to[m])} outside the scene"))
        else:
            rep = blas(nodes, tris[to[m]:t_end[m]], int(root[m]), int(no[m]), int(n_end[m]), name)
        out[f"blas{m}"] = rep
    return out


def check_all(reports):
    bad = [r.describe() for r in reports.values() if not r.ok()]
    assert not bad, "\n".join(bad)
    return max(reports.values(), key=lambda r: r.ratio)


def worst_ratio(reports, prefix):
    return max([r.ratio for k, r in reports.items() if k.startswith(prefix)] or [0.0])


def world_level(boxes, meshdata, tris, box_roundings, records=None):
    """mesh_aabbs against the float64 world corners of each record's triangles (module docstring). box_roundings:
    HOST_BOX or KERNEL_BOX, who made the boxes. Returns (ratio, plain, where): the largest excess / limit_r, the
    largest excess / (2^-24 mag_r), and (record, axis, side) of the first (None when no excess is positive)."""
    assert box_roundings in (HOST_BOX, KERNEL_BOX)
    b = np.asarray(boxes, np.float32).astype(np.float64).reshape(-1, 6)
    to = meshdata["TriOffset"].astype(np.int64)
    t_end = _ranges(to, len(tris))
    worst = (0.0, 0.0, None)
    for m in (range(len(meshdata)) if records is None else records):
        W = meshdata["W2L"][m].astype(np.float64).reshape(4, 4).T
        L = np.linalg.inv(W)
        M, tq, Li, t = np.abs(W[:3, :3]), np.abs(W[:3, 3]), np.abs(L[:3, :3]), np.abs(L[:3, 3])
        local = tri_corners(tris[to[m]:t_end[m]]).reshape(-1, 3)
        world = local @ L[:3, :3].T + L[:3, 3]
        lo, hi = local.min(0), local.max(0)
        mag = Li @ np.maximum(np.abs(lo), np.abs(hi)) + t
        corners = np.array([[(hi if c >> a & 1 else lo)[a] for a in range(3)] for c in range(8)])
        w = np.abs(corners @ L[:3, :3].T + L[:3, 3])
        inv = ((w @ M.T + tq) @ Li.T).max(0)
        limit = U24 * ((3.0 + box_roundings) * mag + inv)
        sound = np.isfinite(limit) & (limit > 0)
        for side, ex in (("hi", world.max(0) - b[m, 0:3]), ("lo", b[m, 3:6] - world.min(0))):
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(sound & np.isfinite(ex), ex / limit, np.inf)  # what cannot be judged fails
                plain = np.where(sound & np.isfinite(ex), ex / (U24 * mag), np.inf)
            a = int(np.argmax(ratio))
            if ratio[a] > worst[0]:
                worst = (float(ratio[a]), float(plain[a]), (int(m), a, side))
    return worst
