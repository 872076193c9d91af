"""TLAS rebuild on the GPU (tt_tlas_rebuild, tt_scene_update_tlas): the other half of AssetManager.RefitTLAS, whose
background task rebuilds the TLAS from the current MeshAABBs and swaps it in -- nodes, TLASBVH8Indices and the refit
plan (AssetManager.cs:1423-1529). The device build must give the host build's bytes, both routes must leave the same
device state, every trace afterwards must equal the oracle on that scene, and a frame slot, a lender with slots, a
plain borrower and a group must each see exactly what the header says they see."""
import numpy as np
import pytest

import oracle_ctypes as O
import tlas_rebuild_cases as T
import tthip
from parity_util import CPU_THREADS, FAR
from test_gpu_slots import _check, _rays

pytestmark = pytest.mark.gpu

W, H = T.W, T.H
SEED = 71


def _engine():
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    return tthip.Engine(0)


def _host_build(a, boxes):
    """(nodes, indices, the TLAS region as an installation leaves it: the nodes, then zeros)."""
    nodes, idx = tthip.tlas_build(boxes)
    region = np.zeros(T.capacity(a), tthip.NODE_DTYPE)
    region[:len(nodes)] = nodes
    return nodes, idx, region


def _state(e, a):
    """What a context holds of scene a's layout: every node and TLASBVH8Indices."""
    return e.scene_nodes(0, len(a.nodes)), e.scene_tlas_indices(0, len(a.tlas))


def _assert_installed(e, a, boxes, md, rays):
    nodes, idx, region = _host_build(a, boxes)
    got = e.scene_nodes(0, T.capacity(a))
    assert got.tobytes() == region.tobytes(), f"{int((got != region).sum())} nodes of the TLAS region differ"
    assert np.array_equal(e.scene_tlas_indices(0, len(idx)), idx)
    sc = T.with_tlas(a, nodes, idx, md)
    assert np.array_equal(e.scene_nodes(0, len(a.nodes)), sc.nodes), "the BLAS nodes are untouched"
    _check(e, sc, rays)
    return sc


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n_mesh", [1, 2, 9, 17, 121])
def test_rebuild_matches_the_host_build_and_the_oracle(n_mesh, device):
    a = T.base_scene(SEED, n_mesh - 1)
    md, boxes = T.moved_pose(a, 7)
    rays = _rays()
    e = _engine()
    try:
        e.upload(a)
        e.update_meshdata(0, md)
        if device:
            import torch

            n = e.tlas_rebuild(torch.from_numpy(boxes).to("cuda:0"), device=True)
        else:
            n = e.tlas_rebuild(boxes)
        assert n == len(tthip.tlas_build(boxes)[0])
        _assert_installed(e, a, boxes, md, rays)
    finally:
        e.close()


@pytest.mark.parametrize("n_mesh", [2, 17, 121])
def test_the_host_route_gives_the_same_state(n_mesh):
    """tt_tlas_build + the asynchronous tt_scene_update_tlas, the caller's arrays overwritten as soon as it returns."""
    a = T.base_scene(SEED, n_mesh - 1)
    md, boxes = T.moved_pose(a, 7)
    rays = _rays()
    e = _engine()
    try:
        e.upload(a)
        e.update_meshdata(0, md)
        nodes, idx = tthip.tlas_build(boxes)
        e.update_tlas(nodes, idx, asynchronous=True)
        nodes.view(np.uint8)[:] = 0xFF
        idx[:] = -1
        _assert_installed(e, a, boxes, md, rays)
        e.timing_reset()
        e.tlas_rebuild(boxes)  # the same TLAS again, through the device route: the same state
        assert len(e.timing_read()) == 3, "presort, BVH2 + BVH8, install"
        _assert_installed(e, a, boxes, md, rays)
    finally:
        e.close()


def test_refit_after_rebuild():
    a = T.base_scene(SEED, 120)
    md, boxes = T.moved_pose(a, 7)
    md3, boxes3 = T.moved_pose(a, 9, ties=False)
    rays = _rays()
    e = _engine()
    try:
        e.upload(a)
        e.update_meshdata(0, md)
        n = e.tlas_rebuild(boxes)
        nodes, idx = tthip.tlas_build(boxes)
        e.update_meshdata(0, md3)
        e.tlas_refit(n, boxes3)
        st, want = O.tlas_refit(T.with_tlas(a, nodes, idx, md3), boxes3)
        assert st == 0
        got = e.scene_nodes(0, len(a.nodes))
        assert np.array_equal(got, want), f"{int((got != want).sum())} nodes differ"
        _check(e, T.with_tlas(a, want[:n], idx, md3), rays)
    finally:
        e.close()


def _slot_scene(s, a, md):
    """The scene as frame slot s traces it: its own TLAS nodes and indices read back, the shared BLASes."""
    nodes, idx = _state(s, a)
    return tthip.Scene(nodes, a.tris, idx, md, a.materials, tlas_nodes=a.tlas_nodes)


def test_frame_slots():
    a = T.base_scene(SEED, 120)
    md_b, box_b = T.moved_pose(a, 9, ties=False)
    md_c, box_c = T.moved_pose(a, 11)
    rays = _rays()
    lender = _engine()
    slots = [tthip.Engine(0) for _ in range(2)]
    try:
        lender.upload(a)
        for s in slots:
            s.share_blas(lender, a.tlas_nodes)
        base_hits = _check(lender, a, rays)
        before = [_state(x, a) for x in (lender, slots[1])]
        # slot 0 rebuilds its own TLAS
        slots[0].update_meshdata(0, md_b)
        n = slots[0].tlas_rebuild(box_b)
        nodes, idx = tthip.tlas_build(box_b)
        assert n == len(nodes) and n > a.tlas_nodes, "this pose's TLAS outgrows the uploaded one (and its old region)"
        assert slots[0].scene_nodes(0, n).tobytes() == nodes.tobytes()
        assert np.array_equal(slots[0].scene_tlas_indices(0, len(idx)), idx)
        sc0 = T.with_tlas(a, nodes, idx, md_b)
        moved = _check(slots[0], sc0, rays)
        assert not np.array_equal(moved, base_hits)
        for x, (nb, ib) in zip((lender, slots[1]), before):
            ng, ig = _state(x, a)
            assert ng.tobytes() == nb.tobytes() and np.array_equal(ig, ib)
            assert np.array_equal(_check(x, a, rays), base_hits)
        # the slot refits what it rebuilt
        slots[0].tlas_refit(n, box_b)
        assert np.array_equal(_check(slots[0], _slot_scene(slots[0], a, md_b), rays), moved)
        # the lender rebuilds while the slots exist: not refused, and no slot sees it
        s0 = _state(slots[0], a)
        lender.update_meshdata(0, md_c)
        lender.tlas_rebuild(box_c)
        _assert_installed(lender, a, box_c, md_c, rays)
        assert _state(slots[0], a)[0][:n].tobytes() == s0[0][:n].tobytes()
        assert np.array_equal(_state(slots[0], a)[1], s0[1])
        assert np.array_equal(_check(slots[0], _slot_scene(slots[0], a, md_b), rays), moved)
        ng, ig = _state(slots[1], a)
        assert ng[:a.tlas_nodes].tobytes() == before[1][0][:a.tlas_nodes].tobytes() and np.array_equal(ig, before[1][1])
        assert np.array_equal(_check(slots[1], _slot_scene(slots[1], a, a.meshdata), rays), base_hits)
        # the host route on the other slot
        slots[1].update_meshdata(0, md_b)
        slots[1].update_tlas(nodes, idx, asynchronous=True)
        assert np.array_equal(_check(slots[1], _slot_scene(slots[1], a, md_b), rays), moved)
    finally:
        lender.close()


def test_a_plain_borrower_sees_the_lenders_rebuilt_tlas_without_a_host_sync():
    import torch

    dev = torch.device("cuda:0")
    a = T.base_scene(SEED, 120)
    md, boxes = T.moved_pose(a, 7)
    nodes, idx = tthip.tlas_build(boxes)
    rays = _rays()
    n = W * H
    st_a, st_b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    lender = tthip.Engine(0, stream=st_a.cuda_stream)
    borrower = tthip.Engine(0, stream=st_b.cuda_stream)
    try:
        lender.upload(a)
        borrower.share_scene(lender)
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).to(dev)
        busy = d_rays.clone()
        torch.cuda.synchronize(dev)
        for _ in range(8):  # the lender's stream is busy: an unordered borrower launch would overtake the install
            lender.trace(busy, n, 0, FAR, W, H, device=True, asynchronous=True)
        lender.update_meshdata(0, md)
        lender.update_tlas(nodes, idx, asynchronous=True)
        borrower.trace(d_rays, n, 0, FAR, W, H, device=True, asynchronous=True)
        torch.cuda.synchronize(dev)
        got = d_rays.cpu().numpy().view(tthip.RAY_DTYPE)
        want = rays.copy()
        assert O.trace(T.with_tlas(a, nodes, idx, md), want, n, 0, FAR, W, H, nthreads=CPU_THREADS)[0] == 0
        assert np.array_equal(got["hits"][:n], want["hits"][:n])
        # and the device route (which synchronizes the lender's stream itself)
        md_c, box_c = T.moved_pose(a, 11)
        lender.update_meshdata(0, md_c)
        lender.tlas_rebuild(box_c)
        _assert_installed(borrower, a, box_c, md_c, rays)
    finally:
        lender.close()


def test_the_leaf_kernel_survives():
    a = T.base_scene(SEED, 0)
    boxes = np.ascontiguousarray(a.meta["mesh_aabbs"], np.float32)
    rays = _rays()
    e = _engine()
    try:
        e.upload(a)
        r = rays.copy()
        e.trace(r, W * H, 0, FAR, W, H)
        assert e.last_trace_form() == tthip.TT_TRACE_FORM_LEAF
        e.tlas_refit(a.tlas_nodes, boxes)  # a device refit: node 0 is no longer known on the host
        e.trace(r, W * H, 0, FAR, W, H)
        assert e.last_trace_form() == tthip.TT_TRACE_FORM_GENERIC
        e.tlas_rebuild(boxes)
        _assert_installed(e, a, boxes, a.meshdata, rays)
        assert e.last_trace_form() == tthip.TT_TRACE_FORM_LEAF
    finally:
        e.close()


def test_refusals_leave_the_scene_as_it_was():
    a = T.base_scene(SEED, 16)
    md, boxes = T.moved_pose(a, 7)
    nodes, idx = tthip.tlas_build(boxes)
    k = len(idx)
    rays = _rays()
    e, b = _engine(), tthip.Engine(0)
    try:
        e.upload(a)
        frame = _check(e, a, rays, bounce_too=False)
        state = _state(e, a)

        def refused(call, status):
            with pytest.raises(tthip.TTError) as ex:
                call()
            assert ex.value.status == status, ex.value
            ng, ig = _state(e, a)
            assert ng.tobytes() == state[0].tobytes() and np.array_equal(ig, state[1])
            assert np.array_equal(_check(e, a, rays, bounce_too=False), frame)

        inner = next(i for i in range(len(nodes)) for c in range(8)
                     if (int(nodes["meta"][i].view(np.uint8)[c]) & 0x18) == 0x18)
        far_child = nodes.copy()
        far_child["base_child"][inner] = T.capacity(a)  # a child index leaving the region
        big = idx.copy()
        big[3] = k  # an index >= n_mesh
        too_many = np.zeros(T.capacity(a) + 1, tthip.NODE_DTYPE)
        too_many[:len(nodes)] = nodes
        nan = boxes.copy()
        nan[5, 1] = np.nan
        INV, UNS = tthip.TT_ERR_INVALID_ARG, tthip.TT_ERR_UNSUPPORTED
        refused(lambda: e.update_tlas(far_child, idx), INV)
        refused(lambda: e.update_tlas(nodes[:len(nodes) - 1], idx), INV)  # the walk leaves the supplied nodes
        refused(lambda: e.update_tlas(nodes, big), INV)
        refused(lambda: e.update_tlas(nodes, idx[:-1]), INV)  # a wrong index count
        refused(lambda: e.update_tlas(too_many, idx), INV)    # n_tlas_nodes above capacity
        refused(lambda: e.tlas_rebuild(nan), UNS)
        refused(lambda: e.tlas_rebuild(boxes[:-1]), INV)
        b.share_scene(e)
        refused(lambda: b.update_tlas(nodes, idx), INV)  # a plain borrower
        refused(lambda: b.tlas_rebuild(boxes), INV)
        # and the context still takes a good TLAS afterwards
        e.update_meshdata(0, md)
        e.update_tlas(nodes, idx)
        _assert_installed(e, a, boxes, md, rays)
    finally:
        e.close()


def test_group_rebuild():
    import torch

    from test_gpu_group import NEAR, oracle_frame

    a = T.base_scene(SEED, 40)
    md, boxes = T.moved_pose(a, 7)
    md_c, box_c = T.moved_pose(a, 11)
    GW, GH = 160, 96
    c2w, ip = tthip.unity_camera((0, 8, 45), (0, -0.2, -1), (0, 1, 0), 70, GW, GH, NEAR, FAR)
    g = tthip.Group(GW, GH, devices=[0, 0], copy=True)
    try:
        g.upload(a)
        out = torch.full((GW * GH, 4), -1, dtype=torch.int32, device="cuda:0")
        g.update_meshdata(0, md)
        n = g.tlas_rebuild(boxes)
        nodes, idx = tthip.tlas_build(boxes)
        assert n == len(nodes)
        g.trace_frame(out, c2w, ip, NEAR, FAR, jitter=1, frames=1)
        want = oracle_frame(T.with_tlas(a, nodes, idx, md), c2w, ip, GW, GH, 1)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want["hits"][:GW * GH])
        # the host route through the group
        nodes_c, idx_c = tthip.tlas_build(box_c)
        g.update_meshdata(0, md_c)
        g.update_tlas(nodes_c, idx_c)
        g.trace_frame(out, c2w, ip, NEAR, FAR, jitter=1, frames=2)
        want = oracle_frame(T.with_tlas(a, nodes_c, idx_c, md_c), c2w, ip, GW, GH, 2)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want["hits"][:GW * GH])
    finally:
        g.close()
