"""The float64 enclosure model (tests/enclosure.py) on everything the host and the oracle write into BVH nodes, and
the controls that show the model can fail. No GPU.

Largest excess over a slot box seen here, in units of U (enclosure.py), against the derived limits (2 U for
triangles, 1 U for instance boxes, 1 for the world level's ratio to its own limit):
  builder (host tt_blas_build: Cornell, soups, prop, the 40-instance scene's BLASes)   0.50 U
  refit (the oracle's general-transform refits of refit_many_cases, all seven records)  0.50 U
  TLAS (the oracle's refits on every quantiser edge and on moved boxes, the host build)  0 U
  TLAS (tt_tlas_build over the 70 boxes of enclosure_cases.edge_scene)                  0.50 U
  world level (mesh_aabbs of the 40 rotated, scaled instances)                          0.19 of the limit,
                                                                                       1.93 in units of 2^-24 mag_r
A tight box pulled in by 64 float32 ulps reads 9.7 of the limit (test_world_level_controls).
The tests print the figures of the run (pytest -s)."""
import numpy as np
import pytest

import assemble_cases as AC
import enclosure as E
import enclosure_cases as EC
import oracle_ctypes as O
import refit_many_cases as R
import tlas_rebuild_cases as T
import tthip
from test_builder import decode_nodes


def _say(name, rep):
    print(f"{name}: {rep.n_slots} slots, worst {rep.ratio:.3f} U of {rep.limit} ({rep.worst})")
    return rep


# ------------------------------------------------------------------ host builds
def _soup(seed, n, scale):
    return tthip.Mesh.soup(seed, n, scale, 0.05 * scale)


BLAS_MESHES = {
    "cornell": lambda: tthip.Mesh.cornell(),
    "soup_100": lambda: _soup(1, 100, 1.0),
    "soup_3000": lambda: _soup(2, 3000, 1.0),
    "soup_20000": lambda: _soup(3, 20000, 1.0),
    "soup_3000_x100": lambda: _soup(4, 3000, 100.0),
    "soup_20000_x1000": lambda: _soup(5, 20000, 1000.0),
    "prop_600": lambda: tthip.Mesh.prop(9, 600),
}


@pytest.mark.parametrize("name", list(BLAS_MESHES))
def test_host_blas_build(name):
    b = tthip.Blas(BLAS_MESHES[name]())
    nodes, tris = b.arrays()
    rep = _say(name, E.blas(nodes, tris, what=name)).check()
    assert rep.n_slots >= 1 and (rep.item_slot[:, 0] >= 0).all()


def test_host_builds_of_the_gpu_build_meshes():
    """The meshes the GPU build tests use (one triangle .. 5,000, and the coplanar grid Validate pads)."""
    for name, mesh in EC.build_meshes().items():
        nodes, tris = tthip.Blas(mesh).arrays()
        _say(name, E.blas(nodes, tris, what=name)).check()


def test_instanced_scene_tlas_blas_and_world_level():
    a = T.base_scene(EC.SEED_40, 40)
    boxes = a.meta["mesh_aabbs"]
    reps = E.scene(a.nodes, a.tris, a.tlas, a.meshdata, boxes, a.tlas_nodes, "40 instances")
    assert len(reps) == 1 + 1 + 6  # the TLAS, the static parent, six props
    for k, r in reps.items():
        _say(k, r)
    E.check_all(reps)
    ratio, plain, where = E.world_level(boxes, a.meshdata, a.tris, E.HOST_BOX)
    print(f"world level: worst excess {ratio:.3f} of its limit, {plain:.3f} x 2^-24 mag, at (record, axis, side) {where}")
    assert ratio <= E.LIMIT_WORLD


def test_assemble_cases_scene_s_host_build():
    """Scene S of tests/assemble_cases.py as the host assembles it (the GPU test walks its on-device assembly)."""
    _, s = AC.scene_s()
    reps = E.scene(s.nodes, s.tris, s.tlas, s.meshdata, s.meta["mesh_aabbs"], s.tlas_nodes, "scene S")
    assert len(reps) == 1 + 5
    _say("scene S", E.check_all(reps))
    assert E.world_level(s.meta["mesh_aabbs"], s.meshdata, s.tris, E.HOST_BOX)[0] <= E.LIMIT_WORLD


def test_world_level_controls():
    """The world-level check can fail: a tight box pulled in by 64 float32 ulps on its largest coordinate is reported with
    its record, axis and side; a record whose limit cannot be formed (a singular-to-zero W2L) fails, it does not pass."""
    a = T.base_scene(EC.SEED_40, 40)
    boxes = np.ascontiguousarray(a.meta["mesh_aabbs"], np.float32).copy()
    m, k = 0, int(np.argmax(np.abs(boxes[0])))  # the static parent stands under the identity: its box is tight
    inward = -np.inf if k < 3 else np.inf  # BBMax moves down, BBMin up
    for _ in range(64):
        boxes[m, k] = np.nextafter(boxes[m, k], np.float32(inward), dtype=np.float32)
    ratio, plain, where = E.world_level(boxes, a.meshdata, a.tris, E.HOST_BOX)
    print(f"box {m} entry {k} pulled in by 64 ulps: {ratio:.2f} of the limit at {where}")
    assert ratio > E.LIMIT_WORLD and where == (int(m), int(k % 3), "hi" if k < 3 else "lo")
    md = a.meshdata.copy()
    md["W2L"][2] = np.nan
    with np.errstate(all="ignore"):
        ratio, _, where = E.world_level(a.meta["mesh_aabbs"], md, a.tris, E.HOST_BOX, records=[2])
    assert ratio == np.inf and where[0] == 2


def test_refit_many_case_before_and_after_oracle_refits():
    c = R.case()
    sc = c.sc
    boxes = sc.meta["mesh_aabbs"]
    before = E.scene(sc.nodes, sc.tris, sc.tlas, sc.meshdata, boxes, sc.tlas_nodes, "refit case, built")
    assert len(before) == 1 + 7
    print(f"built: worst {_say('built', E.check_all(before)).ratio:.3f} U")
    assert E.world_level(boxes, sc.meshdata, sc.tris, E.HOST_BOX)[0] <= E.LIMIT_WORLD
    chain = []
    for r in range(7):  # the static soup too: all seven records
        L = R.Layout(r, R.vertices(r, 0.4 + 0.3 * r), [0, c.blases[r].n_tris], transforms=[R.general_matrix(r)])
        chain.append((r, L.vcat, L.icat, L.leaf, L.transforms[0]))
    nodes, tris = R.oracle_chain(sc, chain)
    assert not np.array_equal(nodes, sc.nodes)
    after = E.scene(nodes, tris, sc.tlas, sc.meshdata, boxes, sc.tlas_nodes, "refit case, refit")
    for k, r in after.items():
        if k != "tlas":
            _say(k, r).check()


# ------------------------------------------------------------------ TLAS: host build, oracle refit
def test_oracle_tlas_refit_after_moving_boxes():
    a = T.base_scene(EC.SEED_40, 40)
    _, boxes = T.moved_pose(a, 7)
    st, nodes = O.tlas_refit(a, boxes)
    assert st == 0 and not np.array_equal(nodes[:a.tlas_nodes], a.nodes[:a.tlas_nodes])
    _say("refit", E.tlas(nodes, a.tlas, boxes, a.tlas_nodes, "oracle TLAS refit")).check()


def test_tlas_build_over_caller_boxes():
    a = T.base_scene(EC.SEED_40, 40)
    for name, boxes in (("moved, tied", T.moved_pose(a, 7)[1]), ("permuted", T.permuted_pose(EC.SEED_40, 40, 5)[1]),
                        ("edge scene 70", EC.edge_scene(70).meta["mesh_aabbs"])):
        nodes, idx = tthip.tlas_build(boxes)
        rep = _say(name, E.tlas(nodes, idx, boxes, len(nodes), "tt_tlas_build: " + name)).check()
        assert rep.n_slots >= len(boxes)


@pytest.mark.parametrize("n", EC.EDGE_SIZES)
def test_quantiser_edges_through_the_oracle_refit(n):
    sc = EC.edge_scene(n)
    if n == EC.EDGE_SIZES[-1]:
        built = E.tlas(sc.nodes, sc.tlas, sc.meta["mesh_aabbs"], sc.tlas_nodes, "built").check()
        assert built.table["depth"].max() >= 1, "the TLAS needs a second level"
    worst = 0.0
    for name, boxes in EC.edge_boxes(n):
        assert boxes.min() > -10000.0
        st, nodes = O.tlas_refit(sc, boxes)
        assert st == 0, name
        rep = E.tlas(nodes, sc.tlas, boxes, sc.tlas_nodes, f"{n} instances, {name}").check()
        worst = max(worst, rep.ratio)
    print(f"{n} instances, {len(EC.edge_boxes(n))} edge cases: worst {worst:.3f} U")


def _pow2_ceil_log2(x):
    """pow(2, ceil(log2(x))) of positive normal float32, as NodeUpdate's quantum is pinned."""
    m, k = np.frexp(x)
    return np.ldexp(np.float32(1.0), np.where(m == np.float32(0.5), k - 1, k)).astype(np.float32)


def test_no_extent_quantises_to_256_exhaustive():
    """quantum = pow2_ceil_log2(fl(extent * 0.003921569f)). fl(1/255) > 1/255, so any extent above 255 * 2^k has a
    product above 2^k and gets the next quantum: ceil(extent / quantum) never reaches 256, and a q byte never
    overflows into its neighbour. Every float32 extent of one binade (scaling by 2 is exact in the others)."""
    c = np.float32(0.003921569)
    assert float(c) > 1.0 / 255.0
    ext = np.arange(0x3F800000, 0x40000000, dtype=np.uint32).view(np.float32)  # [1, 2): holds the edge 255 * 2^-7
    assert ext[0] == 1.0 and len(ext) == 1 << 23
    quantum = _pow2_ceil_log2((ext * c).astype(np.float32))
    steps = np.ceil(ext.astype(np.float64) / quantum.astype(np.float64))  # the division by a power of two is exact
    assert set(np.unique(quantum).tolist()) == {2.0 ** -7, 2.0 ** -6}
    assert steps.max() == 255.0 and steps.min() >= 127.0
    edge = np.float32(255.0 * 2.0 ** -7)
    assert quantum[ext == edge][0] == np.float32(2.0 ** -7) and quantum[ext == np.nextafter(edge, np.float32(2))][0] == np.float32(2.0 ** -6)


def test_a_box_below_minus_10000_is_the_refits_empty_slot():
    """Finding kept under the parity contract: NodeUpdate takes a child with
    BBMax.x < -10000 for an empty slot (BVHRefitter.compute:287-290, restated in the oracle and in tt_refit.hip) and
    collapses it to a point at the parent's minimum. The model reports exactly that slot, and no other."""
    n = 70
    sc = EC.edge_scene(n)
    boxes = EC.far_box_case(n)
    st, nodes = O.tlas_refit(sc, boxes)
    assert st == 0
    rep = E.tlas(nodes, sc.tlas, boxes, sc.tlas_nodes, "far box")
    at = int(np.nonzero(sc.tlas == 3)[0][0])
    node, slot = (int(x) for x in rep.item_slot[at])
    assert int((rep.item_slot == (node, slot)).all(1).sum()) == 1, "the slot holds record 3 alone"
    assert not rep.structure
    assert rep.slots_over() == {(node, slot)}, rep.describe()
    assert {(x.axis, x.side) for x in rep.over} >= {(0, "hi"), (1, "hi"), (2, "hi")}
    print(f"far box: {rep.worst}")
    # the same box at x ~ -9000 is kept
    boxes[3, 0] += np.float32(11000.0)
    boxes[3, 3] += np.float32(11000.0)
    st, nodes = O.tlas_refit(sc, boxes)
    E.tlas(nodes, sc.tlas, boxes, sc.tlas_nodes, "box at -9000").check()


# ------------------------------------------------------------------ controls: the model must report each mutation
def _q(nodes, field, ni, k):
    return (int(nodes[field][ni][k >> 2]) >> (8 * (k & 3))) & 0xFF


def _set_q(nodes, field, ni, k, value):
    assert 0 <= value <= 255
    sh = 8 * (k & 3)
    nodes[field][ni][k >> 2] = (int(nodes[field][ni][k >> 2]) & ~(0xFF << sh) & 0xFFFFFFFF) | (value << sh)


def check_blas_1e4(nodes, tris):
    """test_builder.check_blas as it stood before it called the model: leaf slots only, 1e-4 * (1 + |b|)."""
    for p, e, imask, bc, bt, kids in decode_nodes(nodes):
        scale = np.array([2.0 ** (x - 127) for x in e])
        for kind, slot, m, lo, hi in kids:
            if kind == "inner":
                continue
            bmin, bmax = p + np.array(lo) * scale, p + np.array(hi) * scale
            for j in range(bin(m >> 5).count("1")):
                tr = tris[bt + (m & 0x1F) + j]
                v = np.stack([tr["pos0"], tr["pos0"] + tr["posedge1"], tr["pos0"] + tr["posedge2"]]).astype(np.float64)
                assert (v.min(0) >= bmin - 1e-4 * (1 + np.abs(bmin))).all()
                assert (v.max(0) <= bmax + 1e-4 * (1 + np.abs(bmax))).all()


def _pick(table, rows, after, cap=np.inf):
    """Among the table rows `rows` and the three axes, the (row, axis) whose mutant cuts deepest into the truth
    (`after`: the excess the mutation leaves, per row and axis) without exceeding cap."""
    ex = np.where(rows[:, None] & (table["qhi"] > table["qlo"]) & (after <= cap), after, -np.inf)
    r, a = np.unravel_index(np.argmax(ex), ex.shape)
    assert ex[r, a] > 0
    return int(r), int(a), float(ex[r, a])


def _mutants(nodes, clean, leaf_cap):
    """[(name, mutated nodes, node that must be named)] common to a BLAS and a TLAS; clean: the unmutated report."""
    t = clean.table
    out = []
    # qhi - 1 on a leaf slot: the box loses one quantum and now ends `after` inside the truth
    r, a, ex_hi = _pick(t, ~t["inner"], t["quantum"] - (t["b_hi"] - t["t_hi"]), leaf_cap)
    m = nodes.copy()
    ni, k = int(t["node"][r]), int(t["slot"][r])
    _set_q(m, "qhi_" + "xyz"[a], ni, k, _q(m, "qhi_" + "xyz"[a], ni, k) - 1)
    out.append(("qhi - 1 on a leaf slot", m, ni))
    # qlo + 1 on an inner slot as deep as the tree allows, three levels down at the most
    depth = min(3, int(t["depth"][t["inner"]].max()))
    r, a, ex_lo = _pick(t, t["inner"] & (t["depth"] == depth), t["quantum"] - (t["t_lo"] - t["b_lo"]))
    m = nodes.copy()
    ni, k = int(t["node"][r]), int(t["slot"][r])
    _set_q(m, "qlo_" + "xyz"[a], ni, k, _q(m, "qlo_" + "xyz"[a], ni, k) + 1)
    out.append((f"qlo + 1 on an inner slot of depth {depth}", m, ni))
    # one exponent byte decremented: every box of the node shrinks towards p
    ni = int(t["node"][t["depth"] == 1][0])
    m = nodes.copy()
    assert (int(m["e_imask"][ni]) >> 8) & 0xFF > 1
    m["e_imask"][ni] = int(m["e_imask"][ni]) - (1 << 8)
    out.append(("exponent byte of y decremented", m, ni))
    # imask with a bit dropped
    m = nodes.copy()
    imask = int(m["e_imask"][0]) >> 24
    assert imask
    m["e_imask"][0] = int(m["e_imask"][0]) & ~((imask & -imask) << 24) & 0xFFFFFFFF
    out.append(("imask with a bit dropped", m, 0))
    return out, ex_hi, ex_lo


def test_controls_on_a_blas():
    nodes, tris = tthip.Blas(_soup(2, 3000, 1.0)).arrays()
    clean = E.blas(nodes, tris).check()
    check_blas_1e4(nodes, tris)
    assert clean.table["depth"].max() >= 3
    # the leaf mutant is chosen to stay under half of the old tolerance at |b| = 0, so the old check must let it pass
    mutants, ex_hi, ex_lo = _mutants(nodes, clean, leaf_cap=0.5e-4)
    print(f"q mutants cut {ex_hi:.3g} (leaf) and {ex_lo:.3g} (inner) into the truth")
    for name, m, ni in mutants:
        rep = E.blas(m, tris)
        assert not rep.ok() and ni in rep.nodes_reported(), f"{name}: node {ni} not reported\n{rep.describe()}"
        if name.startswith("q"):
            assert rep.slots_over() and not rep.structure and all(x.node == ni for x in rep.over), rep.describe()
            check_blas_1e4(m, tris)  # the gap: the 1e-4 leaf-only check passes both q mutants
    # two triangles swapped between leaves under different root slots
    first, last = 0, len(tris) - 1
    swapped = tris.copy()
    swapped[[first, last]] = tris[[last, first]]
    under = _root_slot_of_items(nodes, len(tris))
    assert under[first] != under[last]
    rep = E.blas(nodes, swapped)
    holders = {int(clean.item_slot[first, 0]), int(clean.item_slot[last, 0])}
    assert not rep.structure and holders <= rep.nodes_reported() and 0 in rep.nodes_reported(), rep.describe()


def _root_slot_of_items(nodes, n_items):
    """Per item the root slot it hangs under, from the per-node Python decode of test_builder (not the model)."""
    dec = decode_nodes(nodes)
    under = np.full(n_items, -1)

    def mark(ni, tag):
        p, e, imask, bc, bt, kids = dec[ni]
        for kind, slot, m, lo, hi in kids:
            t = slot if ni == 0 else tag
            if kind == "inner":
                mark(bc + bin(imask & ((1 << m - 24) - 1)).count("1"), t)
            else:
                for j in range(bin(m >> 5).count("1")):
                    under[bt + (m & 0x1F) + j] = t

    mark(0, -1)
    return under


def test_controls_on_a_tlas():
    a = T.base_scene(EC.SEED_40, 40)
    boxes = a.meta["mesh_aabbs"]
    nodes = a.nodes[:a.tlas_nodes].copy()
    clean = E.tlas(nodes, a.tlas, boxes, a.tlas_nodes).check()
    mutants, _, _ = _mutants(nodes, clean, leaf_cap=np.inf)
    for name, m, ni in mutants:
        rep = E.tlas(m, a.tlas, boxes, a.tlas_nodes)
        assert not rep.ok() and ni in rep.nodes_reported(), f"{name}: node {ni} not reported\n{rep.describe()}"
    # one TLASBVH8Indices entry duplicated over another: one record named twice, one never
    idx = a.tlas.copy()
    idx[5] = idx[6]
    rep = E.tlas(nodes, idx, boxes, a.tlas_nodes)
    texts = [s[2] for s in rep.structure]
    assert any(f"record {int(a.tlas[6])} is named by 2" in t for t in texts), rep.describe()
    assert any(f"record {int(a.tlas[5])} is named by 0" in t for t in texts), rep.describe()
    assert int(clean.item_slot[6, 0]) in rep.nodes_reported()  # the node whose slot holds the entry named twice
