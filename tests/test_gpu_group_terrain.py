"""Groups that march and bounce off terrains (tt_group_scene_upload_terrains, csrc/tt_group.hip), copy gather on one
device: the gathered records and _PrimaryTriangleInfo against the whole frame's kernel_trace + kernel_heightmap
reference, and every member's bounce-1 rays and records against the reference chain of its own pixels (the merged
enqueue expectation of tests/terrain_bounce_cases.py, then trace + heightmap at bounce 1)."""
import ctypes as C

import numpy as np
import pytest

import oracle_ctypes as O
import terrain_bounce_cases as BC
import terrain_cases as TC
import tthip

pytestmark = pytest.mark.gpu
TID = tthip.TT_TERRAIN_MESH_ID
W = H = 64
WH = W * H
TILE = 16
NEAR = BC.NEAR
MAXB = 2


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def _hip():
    L = C.CDLL("libamdhip64.so.7")  # torch's own HIP runtime: copies of raw device pointers the group hands out
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return L


def device_rays(ptr: int, n: int) -> np.ndarray:
    out = np.zeros(n, tthip.RAY_DTYPE)
    if n:
        assert _hip().hipMemcpy(out.ctypes.data, ptr, 48 * n, 2) == 0  # hipMemcpyDeviceToHost
    return out


def frame_reference(frames, batch=1):
    """Per frame b of the call: the whole frame's rays after trace + heightmap, and its info texels."""
    c2w, ip = BC.camera(W, H)
    out = []
    for b in range(batch):
        rays = O.generate(c2w, ip, W, H, NEAR, TC.FAR, jitter=1, frames=frames + b, max_bounce=MAXB)
        info = np.full((WH, 4), 0xA5A5A5A5, np.uint32)
        BC.trace_reference(rays, WH, 0, W, H, info=info)
        out.append((rays, info))
    return out


def check_gathered(hits, info, ref):
    B = len(ref)
    assert hits.shape == (B * WH, 4)
    for b, (rays, inf) in enumerate(ref):
        assert np.array_equal(hits[b * WH:(b + 1) * WH], rays["hits"][:WH]), f"frame {b}: gathered records"
        assert np.array_equal(info[b * WH:(b + 1) * WH], inf), f"frame {b}: gathered _PrimaryTriangleInfo"
    assert (hits[:, 0] == TID).sum() > 500 * B


def check_members(g, ref, frames, world):
    """Every member's primary rays, bounce-1 rays and bounce-1 records against the reference chain of its pixels."""
    B = len(ref)
    n_ter_total = 0
    for m in range(g.local_members()):
        n, nb, ptr = g.frame_rays(m)
        pix = tthip.group_tile_pixels(W, H, world, m, tile=TILE).astype(np.int64)
        k = len(pix)
        assert n == B * k
        r = np.zeros(B * WH + n, tthip.RAY_DTYPE)
        for b, (rays, _) in enumerate(ref):
            r[b * k:(b + 1) * k] = rays[pix]
            r["PixelIndex"][b * k:(b + 1) * k] += b * WH
        rows, cnt, n_ter = BC.expected_enqueue_batched(r, n, W, H, B, frames, MAXB)
        n_ter_total += n_ter
        r[B * WH:B * WH + cnt] = rows
        BC.trace_reference(r, cnt, 1, W, B * H)
        got = device_rays(ptr, B * WH + n)
        assert nb == cnt, (m, nb, cnt)
        assert np.array_equal(got[:n], r[:n]), f"member {m}: primary rays and records"
        assert np.array_equal(got[B * WH:B * WH + nb], r[B * WH:B * WH + nb]), f"member {m}: bounce-1 rays / records"
    assert n_ter_total > 500 * B, "terrain hits bounce"


def make_group(members, torch, slots=2, batch=1, terrains=True):
    g = tthip.Group(W, H, devices=[0] * members, tile=TILE, slots=slots, bounce=True, copy=True, info=True, batch=batch)
    g.upload(TC.scene())
    if terrains:
        g.upload_terrains(TC.terrains(), TC.atlas())
    return g


def device_outputs(torch, batch=1):
    return (torch.full((batch * WH, 4), -1, dtype=torch.int32, device="cuda:0"),
            torch.full((batch * WH, 4), -1, dtype=torch.int32, device="cuda:0"))


def _np(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("members", [1, 3], ids=["direct", "three_members"])
def test_frame_and_member_chains(members):
    torch = _torch()
    frames = 4
    c2w, ip = BC.camera(W, H)
    ref = frame_reference(frames)
    g = make_group(members, torch)
    try:
        hits, info = device_outputs(torch)
        g.trace_frame(hits, c2w, ip, NEAR, TC.FAR, jitter=1, frames=frames, max_bounce=MAXB, info_out=info)
        check_gathered(_np(hits), _np(info), ref)
        check_members(g, ref, frames, members)
        # one context's trace + heightmap of the whole frame
        e = tthip.Engine(0)
        try:
            e.upload(TC.scene())
            e.upload_terrains(TC.terrains(), TC.atlas())
            rays, inf = np.zeros(2 * WH, tthip.RAY_DTYPE), np.zeros((WH, 4), np.uint32)
            e.generate(rays, c2w, ip, W, H, NEAR, TC.FAR, jitter=1, frames=frames, max_bounce=MAXB)
            e.trace(rays, WH, 0, TC.FAR, W, H, info=inf)
            e.trace_heightmap(rays, WH, 0, TC.FAR, W, H, info=inf)
            assert np.array_equal(_np(hits), rays["hits"][:WH]) and np.array_equal(_np(info), inf)
        finally:
            e.close()
        # a host hits_out (synchronous, staged) equals the device result
        h_hits, h_info = np.zeros((WH, 4), np.uint32), np.zeros((WH, 4), np.uint32)
        g.trace_frame(h_hits, c2w, ip, NEAR, TC.FAR, jitter=1, frames=frames, max_bounce=MAXB, info_out=h_info)
        assert np.array_equal(h_hits, _np(hits)) and np.array_equal(h_info, _np(info))
    finally:
        g.close()


@pytest.mark.parametrize("members", [1, 3], ids=["direct", "three_members"])
def test_batched_asynchronous_frames_over_two_slots(members):
    torch = _torch()
    B = 2
    c2w, ip = BC.camera(W, H)
    g = make_group(members, torch, slots=2, batch=B)
    try:
        outs = [device_outputs(torch, B) for _ in range(2)]
        starts = [1, 1 + B]
        for (hits, info), f in zip(outs, starts):
            g.trace_frame(hits, c2w, ip, NEAR, TC.FAR, jitter=1, frames=f, max_bounce=MAXB, asynchronous=True,
                          info_out=info)
        g.sync()
        refs = [frame_reference(f, B) for f in starts]
        for (hits, info), ref in zip(outs, refs):
            check_gathered(_np(hits), _np(info), ref)
        check_members(g, refs[1], starts[1], members)  # the latest call's chains
    finally:
        g.close()


def test_clearing_the_set_returns_todays_frames():
    torch = _torch()
    frames = 2
    c2w, ip = BC.camera(W, H)
    results = []
    for had_terrains in (False, True):
        g = make_group(3, torch, terrains=had_terrains)
        try:
            if had_terrains:
                hits, info = device_outputs(torch)
                g.trace_frame(hits, c2w, ip, NEAR, TC.FAR, jitter=1, frames=frames, max_bounce=MAXB, info_out=info)
                assert (_np(hits)[:, 0] == TID).sum() > 500
                g.upload_terrains(None)  # n = 0 clears the set
            hits, info = device_outputs(torch)
            g.trace_frame(hits, c2w, ip, NEAR, TC.FAR, jitter=1, frames=frames, max_bounce=MAXB, info_out=info)
            rays = []
            for m in range(3):
                n, nb, ptr = g.frame_rays(m)
                rays.append((n, nb, device_rays(ptr, WH + nb)[np.r_[0:n, WH:WH + nb]]))
            results.append((_np(hits), _np(info), rays))
        finally:
            g.close()
    (h0, i0, r0), (h1, i1, r1) = results
    assert not (h0[:, 0] == TID).any()
    assert np.array_equal(h0, h1) and np.array_equal(i0, i1)
    for (n0, nb0, a), (n1, nb1, b) in zip(r0, r1):
        assert (n0, nb0) == (n1, nb1) and np.array_equal(a, b)
    # and they are the oracle's frame without terrains
    full = O.generate(c2w, ip, W, H, NEAR, TC.FAR, jitter=1, frames=frames, max_bounce=MAXB)
    assert O.trace(TC.scene(), full, WH, 0, TC.FAR, W, H)[0] == 0
    assert np.array_equal(h0, full["hits"][:WH])


def test_group_upload_succeeds_where_the_lending_member_context_refuses():
    torch = _torch()
    g = make_group(2, torch, slots=2, terrains=False)
    try:
        t, a = TC.terrains(), TC.atlas()
        st = g.L.tt_scene_upload_terrains(g.member_ctx(0), t.ctypes.data, len(t), a.ctypes.data, a.shape[1], a.shape[0])
        assert st == tthip.TT_ERR_INVALID_ARG, "slot 1 borrows slot 0's scene: the lender refuses"
        assert g.upload_terrains(t, a) == tthip.TT_OK
        hits, info = device_outputs(torch)
        c2w, ip = BC.camera(W, H)
        g.trace_frame(hits, c2w, ip, NEAR, TC.FAR, jitter=1, frames=0, max_bounce=MAXB, info_out=info)
        check_gathered(_np(hits), _np(info), frame_reference(0))
        bad = t.copy()
        bad[1]["HeightMap"][0] = 1.5
        assert g.upload_terrains(bad, a, check=False) == tthip.TT_ERR_INVALID_ARG
    finally:
        g.close()
