"""tt_blas_refit_many on the GPU: a frame's deforming meshes, renderer by renderer, in two launches. The device
bytes afterwards must be those of the oracle's refits made one mesh at a time (refit_many_cases.py holds the scene,
the part layouts and the expected values; nothing expected comes from the library)."""
import numpy as np
import pytest

import bruteforce as BF
import bruteforce_cases as BC
import oracle_ctypes as O
import refit_many_cases as R
import tthip

pytestmark = pytest.mark.gpu

FAR = BC.FAR
INV, UNS = tthip.TT_ERR_INVALID_ARG, tthip.TT_ERR_UNSUPPORTED


def read_scene(e, sc):
    return e.scene_nodes(0, len(sc.nodes)), e.scene_tris(0, len(sc.tris))


def assert_scene(e, sc, nodes, tris, what=""):
    got_n, got_t = read_scene(e, sc)
    assert np.array_equal(got_t, tris), f"{what}: {int((got_t != tris).sum())} triangle records differ"
    assert np.array_equal(got_n, nodes), f"{what}: {int((got_n != nodes).sum())} nodes differ"


def one_part_layouts(t, matrix=R.general_matrix):
    return [R.Layout(r, R.vertices(r, t), [0, n], transforms=[matrix(r)]) for r, n in zip(R.RECORDS, R.SIZES)]


def chain_of(layouts):
    """The oracle refits of one-transform layouts, in list order."""
    return [(L.record, L.vcat, L.icat, L.leaf, L.transforms[0]) for L in layouts]


def exact_layouts(t=0.9):
    return [R.Layout(r, R.vertices(r, t, exact=True), cuts, strides=(6, 10),
                     transforms=[R.exact_matrix(10 * r + k) for k in range(len(cuts) - 1)], reverse=r % 2 == 0)
            for r, cuts in zip(R.RECORDS, R.CUTS)]


def exact_expected(sc, layouts):
    return R.oracle_chain(sc, [(L.record, L.pretransformed(), L.icat, L.leaf, None) for L in layouts])


def test_one_part_per_mesh_equals_the_oracle_chain_and_the_single_call(engine):
    sc = R.case().sc
    layouts = one_part_layouts(0.4)
    engine.upload(sc)
    engine.timing_reset()
    engine.blas_refit_many([L.item() for L in layouts])
    assert len(engine.timing_read()) == 1  # one entry for the whole list
    nodes, tris = R.oracle_chain(sc, chain_of(layouts))
    assert_scene(engine, sc, nodes, tris, "all meshes")
    assert not np.array_equal(nodes, sc.nodes) and not np.array_equal(tris, sc.tris)
    # a list of one against tt_blas_refit on a second engine, byte for byte
    other = tthip.Engine(0)
    try:
        for L in (layouts[0], layouts[2], layouts[5]):
            engine.upload(sc)
            other.upload(sc)
            engine.blas_refit_many([L.item()])
            p = L.parts[0]
            other.blas_refit(L.record, p.vertices, p.indices, L.leaf, p.transform)
            a, b = read_scene(engine, sc), read_scene(other, sc)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), f"record {L.record}"
            want = R.oracle_chain(sc, chain_of([L]))
            assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1])
    finally:
        other.close()


def test_several_parts_one_transform_equal_the_concatenated_refit(engine):
    sc = R.case().sc
    xf = R.general_matrix(3)
    layouts = [R.Layout(r, R.vertices(r, 1.3), cuts, transforms=[xf] * (len(cuts) - 1), reverse=r % 2 == 1)
               for r, cuts in zip(R.RECORDS, R.CUTS)]
    engine.upload(sc)
    engine.blas_refit_many([L.item() for L in layouts])
    nodes, tris = R.oracle_chain(sc, chain_of(layouts))
    assert_scene(engine, sc, nodes, tris, "several parts, one transform")


def test_parts_with_general_transforms(engine):
    """Every triangle record is the oracle's under its part's transform; the topology is untouched; after the TLAS
    refit from the boxes the call wrote, closest hits equal brute force over the deformed triangles."""
    c = R.case()
    sc = c.sc
    layouts = [R.Layout(r, R.vertices(r, 2.1), cuts, strides=(6, 10),
                        transforms=[R.general_matrix(r + 2 * k) for k in range(len(cuts) - 1)], reverse=r % 2 == 0)
               for r, cuts in zip(R.RECORDS, R.CUTS)]
    engine.upload(sc)
    boxes = np.ascontiguousarray(sc.meta["mesh_aabbs"], np.float32).copy()
    engine.blas_refit_many([L.item(c.l2w[L.record]) for L in layouts], mesh_aabbs=boxes)
    got_n, got_t = read_scene(engine, sc)
    want_t = sc.tris.copy()
    p0, e1, e2 = (sc.tris[f].astype(np.float64) for f in ("pos0", "posedge1", "posedge2"))
    for L in layouts:
        to = int(sc.meshdata["TriOffset"][L.record])
        for k, (a, b) in enumerate(zip(L.cuts[:-1], L.cuts[1:])):
            st, _, tris_k = O.blas_refit(sc, L.record, L.vcat, L.icat, L.leaf, L.transforms[k])
            assert st == 0
            at = to + L.leaf[a:b]
            want_t[at] = tris_k[at]
        cn = L.corners64()
        at = to + L.leaf
        p0[at], e1[at], e2[at] = cn[:, 0], cn[:, 1] - cn[:, 0], cn[:, 2] - cn[:, 0]
    assert np.array_equal(got_t, want_t), f"{int((got_t != want_t).sum())} triangle records differ"
    for f in ("base_child", "base_tri", "meta"):
        assert np.array_equal(got_n[f], sc.nodes[f])
    assert np.array_equal(got_n["e_imask"] >> 24, sc.nodes["e_imask"] >> 24)
    no = int(sc.meshdata["NodeOffset"][1])
    assert np.array_equal(got_n[:no], sc.nodes[:no])  # the TLAS and the static soup's BLAS
    assert not np.array_equal(got_n[no:], sc.nodes[no:])
    assert np.array_equal(boxes[0], sc.meta["mesh_aabbs"][0])
    engine.tlas_refit(sc.tlas_nodes, boxes)
    g = BF.Geometry.from_scene(sc, p0, e1, e2)
    n = 400
    o, d = BC.random_rays(g, 5, n)
    rays = BC.ray_buffer(o, d)
    ref = BC.reference_closest(g, rays, n, 0, 0)
    assert int((ref.hit & ref.robust).sum()) >= 100
    traced = rays.copy()
    engine.trace(traced, n, 0, FAR, n, 1)
    BC.compare_closest(ref, traced["hits"][:n], caps=False).check()


def test_parts_with_exact_transforms_are_byte_exact(engine):
    """Signed axis permutations with translations in quarters over vertices on the 1/64 grid: nothing rounds, so
    nodes and triangles equal the oracle's identity refit of the pre-transformed concatenated buffers."""
    sc = R.case().sc
    layouts = exact_layouts()
    engine.upload(sc)
    engine.blas_refit_many([L.item() for L in layouts])
    nodes, tris = exact_expected(sc, layouts)
    assert_scene(engine, sc, nodes, tris, "exact transforms")


def test_bounds_and_world_boxes(engine):
    c = R.case()
    sc = c.sc
    n_mesh = len(sc.meshdata)
    # identity part transforms, exact local_to_world for the even records, none for the odd ones
    layouts = [R.Layout(r, R.vertices(r, 0.6, exact=True), cuts, strides=(10, 6)) for r, cuts in zip(R.RECORDS, R.CUTS)]
    l2w = {L.record: R.exact_matrix(L.record) for L in layouts if L.record % 2 == 0}
    engine.upload(sc)
    bounds = np.full((len(layouts), 6), 7e7, np.float32)
    boxes = np.full((n_mesh, 6), 7e7, np.float32)
    engine.blas_refit_many([L.item(l2w.get(L.record)) for L in layouts], bounds_out=bounds, mesh_aabbs=boxes)
    for i, L in enumerate(layouts):
        i3 = L.icat.reshape(-1, 3)
        want = R.padded_root_box(L.vcat[:, 0:3][i3])
        assert np.array_equal(bounds[i], want), (L.record, bounds[i], want)  # (numerically: zeros of either sign)
        if L.record in l2w:
            w = R.world_box64(want, l2w[L.record]).astype(np.float32)
            assert np.array_equal(boxes[L.record], w), (L.record, boxes[L.record], w)
        else:
            assert (boxes[L.record] == np.float32(7e7)).all()
    assert (boxes[0] == np.float32(7e7)).all()
    # a general local_to_world: within the rounding bound of the pinned chain around the float64 box
    layouts = one_part_layouts(1.1, matrix=lambda r: np.eye(4))
    gen = {L.record: R.general_matrix(5 + L.record) for L in layouts}
    engine.blas_refit_many([L.item(gen[L.record]) for L in layouts], bounds_out=bounds, mesh_aabbs=boxes)
    for i, L in enumerate(layouts):
        i3 = L.icat.reshape(-1, 3)
        root = R.padded_root_box(L.vcat[:, 0:3][i3])
        assert np.array_equal(bounds[i], root)
        m32 = tthip.unity_colmajor(gen[L.record]).reshape(4, 4).T.astype(np.float64)  # the matrix as the call got it
        err = np.abs(boxes[L.record].astype(np.float64) - R.world_box64(root, m32))
        bound = R.world_box_bound(root, m32)
        print(f"record {L.record}: max error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (L.record, err, bound)
    # one mesh of one part (its descriptors travel in the kernel arguments): the same outputs, bit for bit
    L = layouts[4]
    all_boxes = boxes.copy()
    one_bounds, boxes[:] = np.zeros((1, 6), np.float32), 7e7
    engine.blas_refit_many([L.item(gen[L.record])], bounds_out=one_bounds, mesh_aabbs=boxes)
    assert one_bounds[0].tobytes() == bounds[4].tobytes() and boxes[L.record].tobytes() == all_boxes[L.record].tobytes()
    assert (np.delete(boxes, L.record, 0) == np.float32(7e7)).all()


def test_plan_cache_and_counters(engine):
    c = R.case()
    sc = c.sc
    engine.upload(sc)
    state = (sc.nodes, sc.tris)

    def step(layouts, call):
        nonlocal state
        call()
        state = R.oracle_chain(R.with_arrays(sc, *state), chain_of(layouts))
        assert_scene(engine, sc, state[0], state[1], f"step {step.n}")
        step.n += 1

    step.n = 0
    for t in (0.3, 1.7):  # the same list twice: a counter that was not reset shows in the second
        layouts = one_part_layouts(t)
        step(layouts, lambda: engine.blas_refit_many([L.item() for L in layouts]))
    sub = [one_part_layouts(2.6)[k] for k in (4, 1, 5)]  # a reordered subset
    step(sub, lambda: engine.blas_refit_many([L.item() for L in sub]))
    one = one_part_layouts(0.8)[3]
    p = one.parts[0]
    step([one], lambda: engine.blas_refit(one.record, p.vertices, p.indices, one.leaf, p.transform))
    again = one_part_layouts(3.3)
    step(again, lambda: engine.blas_refit_many([L.item() for L in again]))
    engine.upload(sc)  # a fresh upload: the plans are the old scene generation's
    state = (sc.nodes, sc.tris)
    last = one_part_layouts(0.5)
    step(last, lambda: engine.blas_refit_many([L.item() for L in last]))


def test_plan_cache_follows_a_record_repointed_at_another_blas(engine):
    """tt_scene_update_meshdata may re-point a record at another validated BLAS of the same triangle count without a
    new scene generation. The same (mesh_index, n_tris) list must then refit that BLAS's nodes, not the cached
    forest's: the state equals the oracle's refits over the updated records."""
    from test_blas_refit import deform

    meshes = [tthip.Mesh.soup(1, 120, 3.0, 0.3), tthip.Mesh.prop(21, 600), tthip.Mesh.prop(22, 600)]
    blases = [tthip.Blas(m) for m in meshes]
    am = tthip.AssetManager()
    for k, b in enumerate(blases):
        am.add_parent(b, tthip.trs_matrix((3.0 * k, 0.0, 0.0)), np.zeros(1, tthip.MAT_DTYPE))
    sc = am.build()

    def frame(k1, t):
        """(items, oracle refits): record 1 over mesh k1, record 0 over the soup; two items, so the staged form."""
        items, chain = [], []
        for record, k in ((1, k1), (0, 0)):
            pos, nrm, idx = meshes[k].arrays()
            v = np.full((len(pos), 10), 0.5, np.float32)
            v[:, 0:3], v[:, 3:6] = deform(pos, t), nrm
            idx, leaf = np.ascontiguousarray(idx, np.int32), blases[k].leaf_order()
            items.append(tthip.RefitItem(record, blases[k].n_tris, leaf, [tthip.RefitPart(v, idx)]))
            chain.append((record, v, idx, leaf, None))
        return items, chain

    engine.upload(sc)
    items, chain = frame(1, 0.4)
    engine.blas_refit_many(items)
    state = R.oracle_chain(sc, chain)
    assert_scene(engine, sc, state[0], state[1], "before the update")
    md = sc.meshdata.copy()
    for f in ("NodeOffset", "TriOffset", "mesh_data_bvh_offsets"):
        md[f][1] = md[f][2]
    engine.update_meshdata(0, md)
    items, chain = frame(2, 1.5)  # record 1 now names mesh 2's BLAS: its vertices, indices and leaf order
    engine.blas_refit_many(items)
    moved = tthip.Scene(state[0], state[1], sc.tlas, md, sc.materials, tlas_nodes=sc.tlas_nodes)
    want = R.oracle_chain(moved, chain)
    assert_scene(engine, sc, want[0], want[1], "after the update")
    a, b = (int(sc.meshdata["NodeOffset"][r]) for r in (1, 2))
    assert np.array_equal(want[0][a:b], state[0][a:b]) and not np.array_equal(want[0][b:], state[0][b:])


def trace_records(e, sc_expected, rays, W, H):
    got, want = rays.copy(), rays.copy()
    e.trace(got, W * H, 0, FAR, W, H)
    assert O.trace(sc_expected, want, W * H, 0, FAR, W, H)[0] == 0
    return got["hits"][:W * H], want["hits"][:W * H]


def frame_rays(W, H):
    c2w, ip = tthip.unity_camera((0.5, 2.0, 16.0), (0, -0.1, -1), (0, 1, 0), 60, W, H, 0.3, FAR)
    return O.generate(c2w, ip, W, H, 0.3, FAR)


def test_a_borrower_and_a_frame_slot_see_the_lenders_refit():
    sc = R.case().sc
    W, H = 96, 64
    rays = frame_rays(W, H)
    lender, plain, slot = tthip.Engine(0), tthip.Engine(0), tthip.Engine(0)
    try:
        lender.upload(sc)
        plain.share_scene(lender)
        slot.share_blas(lender, sc.tlas_nodes)
        for e in (plain, slot):  # reads in flight before the lender's mutation
            e.trace(rays.copy(), W * H, 0, FAR, W, H)
        layouts = [R.Layout(r, R.vertices(r, 0.7), cuts, reverse=True) for r, cuts in zip(R.RECORDS, R.CUTS)]
        lender.blas_refit_many([L.item() for L in layouts])
        nodes, tris = R.oracle_chain(sc, chain_of(layouts))
        want = R.with_arrays(sc, nodes, tris)
        for e in (plain, slot):
            got, exp = trace_records(e, want, rays, W, H)
            assert np.array_equal(got, exp)
            assert np.array_equal(e.scene_nodes(0, len(nodes)), nodes)
        with pytest.raises(tthip.TTError) as err:
            plain.blas_refit_many([layouts[0].item()])
        assert err.value.status == INV and "shared scene" in str(err.value)
        with pytest.raises(tthip.TTError) as err:
            slot.blas_refit_many([layouts[0].item()])
        assert err.value.status == INV
    finally:
        lender.close()


def test_the_host_free_chain(engine):
    """Device arrays, every call asynchronous: the refit writes the boxes the TLAS refit reads, then a trace,
    then one sync."""
    import torch

    c = R.case()
    sc = c.sc
    dev = torch.device("cuda", 0)
    layouts = exact_layouts(1.9)
    W, H = 96, 64
    rays = frame_rays(W, H)
    engine.upload(sc)
    keep = []

    def to_dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t

    items = []
    for L in layouts:
        parts = [tthip.RefitPart(to_dev(p.vertices), to_dev(p.indices), p.first_tri, p.transform, n_vertices=p.n_vertices,
                                 vertex_stride=p.vertex_stride, n_tris=p.n_tris) for p in L.parts]
        items.append(tthip.RefitItem(L.record, L.n_tris, to_dev(L.leaf), parts, c.l2w[L.record]))
    boxes0 = np.ascontiguousarray(sc.meta["mesh_aabbs"], np.float32)
    d_boxes, d_bounds, d_rays = to_dev(boxes0), to_dev(np.zeros((len(items), 6), np.float32)), to_dev(rays.view(np.uint8))
    torch.cuda.synchronize(dev)
    engine.blas_refit_many(items, device=True, asynchronous=True, bounds_out=d_bounds, mesh_aabbs=d_boxes)
    engine.tlas_refit(sc.tlas_nodes, d_boxes, device=True, asynchronous=True)
    engine.trace(d_rays, W * H, 0, FAR, W, H, device=True, asynchronous=True)
    engine.sync()
    # expected: the oracle's refits, the boxes numpy derives from the exact vertices, the oracle's TLAS refit
    nodes, tris = exact_expected(sc, layouts)
    boxes = boxes0.copy()
    for i, L in enumerate(layouts):
        pre = L.pretransformed()
        root = R.padded_root_box(pre[:, 0:3][L.icat.reshape(-1, 3)])
        assert np.array_equal(d_bounds[i].cpu().numpy(), root)
        boxes[L.record] = R.world_box64(root, c.l2w[L.record]).astype(np.float32)
    assert np.array_equal(d_boxes.cpu().numpy(), boxes)
    st, nodes2 = O.tlas_refit(R.with_arrays(sc, nodes, tris), boxes)
    assert st == 0
    assert_scene(engine, sc, nodes2, tris, "after the chain")
    want = rays.copy()
    assert O.trace(R.with_arrays(sc, nodes2, tris), want, W * H, 0, FAR, W, H)[0] == 0
    got = d_rays.cpu().numpy().view(tthip.RAY_DTYPE)
    assert np.array_equal(got["hits"][:W * H], want["hits"][:W * H])
    assert int((want["hits"][:W * H, 1] != 0xFFFFFFFF).sum()) > 100


def test_refusals_leave_the_scene_as_it_was(engine):
    import torch

    c = R.case()
    sc = c.sc
    engine.upload(sc)

    def layouts():
        return [R.Layout(r, R.vertices(r, 0.2), cuts) for r, cuts in zip(R.RECORDS, R.CUTS)]

    def refused(items, status, word, **kw):
        with pytest.raises(tthip.TTError) as err:
            engine.blas_refit_many(items, **kw)
        assert err.value.status == status and word in str(err.value), str(err.value)

    refused([], INV, "no items")
    it = layouts()[2].item()
    it.leaf_of_triangle = None
    refused([it], INV, "null")
    it = layouts()[2].item()
    it.parts[0].vertices = None
    refused([layouts()[0].item(), it], INV, "item 1: part 0")
    it = layouts()[3].item()
    it.parts[1].vertex_stride = 5
    refused([it], INV, "vertex_stride < 6")
    it = layouts()[0].item()
    it.mesh_index = len(sc.meshdata)
    refused([it], INV, "out of range")
    refused([layouts()[1].item(), layouts()[4].item(), layouts()[1].item()], INV, "too")
    it = layouts()[5].item()
    it.parts[2].first_tri -= 1  # overlaps its neighbour, leaves the last triangle out
    refused([it], INV, "overlaps")
    it = layouts()[5].item()
    del it.parts[1]
    refused([it], INV, "gap")
    it = layouts()[5].item()
    it.n_tris = len(sc.tris)  # more than the scene holds behind its TriOffset
    refused([it], INV, "exceeds the scene's triangles")
    it = layouts()[4].item()
    it.parts[0].indices = it.parts[0].indices.copy()
    it.parts[0].indices[5] = it.parts[0].n_vertices
    refused([it], INV, "index")
    it = layouts()[4].item()
    it.leaf_of_triangle = it.leaf_of_triangle.copy()
    it.leaf_of_triangle[9] = -1
    refused([it], INV, "leaf_of_triangle[9]")
    refused([layouts()[0].item()], INV, "not device memory", device=True)  # the device flag with host pointers
    L = layouts()[0]
    p = L.parts[0]
    d_v, d_i, d_l = (torch.from_numpy(a).to("cuda:0") for a in (p.vertices, p.indices, L.leaf))
    d_item = tthip.RefitItem(L.record, L.n_tris, d_l, [tthip.RefitPart(d_v, d_i, 0, n_vertices=p.n_vertices,
                                                                        vertex_stride=p.vertex_stride, n_tris=p.n_tris)])
    refused([d_item], INV, "bounds_out or mesh_aabbs", device=True, bounds_out=np.zeros(6, np.float32))
    # two records over one BLAS, and a root that is not the first node: a scene of its own
    blas = tthip.Blas(tthip.Mesh.prop(3, 50))
    am = tthip.AssetManager()
    am.add_parent(c.blases[0])
    ip = am.add_instance_parent(blas)
    am.add_instance(ip, tthip.trs_matrix((2.0, 0.0, 0.0)))
    am.add_instance(ip, tthip.trs_matrix((4.0, 0.0, 0.0)))
    shared = am.build()
    pos, nrm, idx = tthip.Mesh.prop(3, 50).arrays()
    v = np.ascontiguousarray(np.concatenate([pos, nrm], axis=1))
    other = tthip.Engine(0)
    try:
        other.upload(shared)
        twice = [tthip.RefitItem(r, 50, blas.leaf_order(), [tthip.RefitPart(v, idx)]) for r in (1, 2)]
        with pytest.raises(tthip.TTError) as err:
            other.blas_refit_many(twice)
        assert err.value.status == INV and "shares NodeOffset" in str(err.value)
        assert np.array_equal(other.scene_nodes(0, len(shared.nodes)), shared.nodes)
        assert np.array_equal(other.scene_tris(0, len(shared.tris)), shared.tris)
        md = shared.meshdata.copy()
        md["mesh_data_bvh_offsets"][1] += 1  # the record's root is now the BLAS's second node
        other.update_meshdata(0, md)
        with pytest.raises(tthip.TTError) as err:
            other.blas_refit_many(twice[:1])
        assert err.value.status == UNS and "root is not its first node" in str(err.value)
        assert np.array_equal(other.scene_nodes(0, len(shared.nodes)), shared.nodes)
    finally:
        other.close()
    # nothing was enqueued by any refusal: the scene is byte for byte the upload, and the context still traces
    assert_scene(engine, sc, sc.nodes, sc.tris, "after the refusals")
    W, H = 64, 48
    got, want = trace_records(engine, sc, frame_rays(W, H), W, H)
    assert np.array_equal(got, want)
    good = layouts()
    engine.blas_refit_many([L.item() for L in good])  # and the call it refused works
    nodes, tris = R.oracle_chain(sc, chain_of(good))
    assert_scene(engine, sc, nodes, tris, "after a good call")
