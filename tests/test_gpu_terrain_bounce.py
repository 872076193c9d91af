"""The bounce enqueue with TT_ENQUEUE_TERRAIN_BOUNCE (csrc/tt_raygen.hip's terrain instantiation) and
tt_trace_heightmap_hits (csrc/tt_terrain.hip) on the GPU, bit for bit against the merged expectation of
tests/terrain_bounce_cases.py: the oracle's enqueue for the triangle rows, tt_terrain_bounce_host for the terrain
rows, merged by source index. The scene is tests/terrain_cases.py's (a Cornell box on terrain 0, terrain 1
overlapping)."""
import numpy as np
import pytest

import oracle_ctypes as O
import terrain_bounce_cases as BC
import terrain_cases as TC
import tthip

pytestmark = pytest.mark.gpu
TID = tthip.TT_TERRAIN_MESH_ID
NEAR = BC.NEAR
FRAMES, MAXB = 3, 4


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


@pytest.fixture(scope="module")
def eng():
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    e = tthip.Engine(0)
    e.upload(TC.scene())
    e.upload_terrains(TC.terrains(), TC.atlas())
    yield e
    e.close()


@pytest.fixture(scope="module")
def plain():
    """A context with the same scene and no terrain set."""
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    e = tthip.Engine(0)
    e.upload(TC.scene())
    yield e
    e.close()


def _dev(a):
    return _torch().from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


# 1 ---------------------------------------------------------------- the test that fails without the feature
def test_primary_frame_host_pointers_flag_set(eng):
    W = H = 64
    n = W * H
    ref, _ = BC.primary(W, H)
    rows, cnt, n_ter = BC.expected_enqueue(ref, n, 0, W, H, FRAMES, MAXB)
    assert n_ter > 500 and cnt - n_ter > 50, "terrain and triangle survivors"
    assert (rows["hits"][rows["hits"][:, 0] == TID, 1] == 1).any(), "terrain 1 among them"
    rays = ref.copy()
    got = eng.enqueue_bounce(rays, n, 0, TC.FAR, W, H, frames=FRAMES, max_bounce=MAXB, terrain_bounce=True)
    assert got == cnt
    assert np.array_equal(rays[n:n + cnt], rows)
    assert np.array_equal(rays[:n], ref[:n]), "the source window is not written"


# 2 ---------------------------------------------------------------- three tiles, device pointers, device counts
def _indirect(eng, torch, frame, n, count, W, H):
    """The flagged _indirect enqueue of `frame` (a 2 W H array) with the device count `count`, a canary in the
    destination half: (survivor count, the array afterwards)."""
    start = frame.copy()
    start["PixelIndex"][n:] = 0xFFFFFFFF
    d = _dev(start)
    n_dev = torch.tensor([count], dtype=torch.int32, device="cuda:0")
    n_next = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    eng.enqueue_bounce_indirect(d, n_dev, n, n_next, 0, TC.FAR, W, H, frames=FRAMES, max_bounce=MAXB,
                                terrain_bounce=True)
    eng.sync()
    return int(n_next.item()), _host(d, frame)


def test_three_tiles_device_pointers_and_indirect_count(eng):
    torch = _torch()
    W = H = 96
    n = W * H
    assert (n + 4095) // 4096 == 3
    ref, _ = BC.primary(W, H)
    rows, cnt, n_ter = BC.expected_enqueue(ref, n, 0, W, H, FRAMES, MAXB)
    src = rows["PixelIndex"][rows["hits"][:, 0] == TID]  # (a primary ray's PixelIndex is its source index)
    assert (src < 4096).sum() > 500 and (src >= 4096).sum() > 500, "terrain survivors of tile 0 precede tile 1's"
    d = _dev(ref)
    got = eng.enqueue_bounce(d, n, 0, TC.FAR, W, H, frames=FRAMES, max_bounce=MAXB, device=True, terrain_bounce=True)
    assert got == cnt
    assert np.array_equal(_host(d, ref)[n:n + cnt], rows)
    # a device count inside the third tile
    count = 8500
    rows_c, cnt_c, _ = BC.expected_enqueue(ref, count, 0, W, H, FRAMES, MAXB)
    k, out = _indirect(eng, torch, ref, n, count, W, H)
    assert k == cnt_c and np.array_equal(out[n:n + cnt_c], rows_c)
    assert (out["PixelIndex"][n + cnt_c:] == 0xFFFFFFFF).all(), "nothing is written past the survivors"
    # This camera sees sky in the frame's upper rows, so the third tile holds no survivor. The same rays in reverse
    # order put the terrain survivors into tiles 1 and 2: the look-back carries them over three tiles, and the
    # count cuts survivors off (rows past it do not survive).
    rev = ref.copy()
    rev[:n] = ref[:n][::-1]
    rows_r, cnt_r, ter_r = BC.expected_enqueue(rev, count, 0, W, H, FRAMES, MAXB)
    src_r = np.nonzero(np.isin(rev["PixelIndex"][:n], rows_r["PixelIndex"][rows_r["hits"][:, 0] == TID]))[0]
    assert ((src_r >= 4096) & (src_r < 8192)).sum() > 500 and (src_r >= 8192).sum() > 100 and cnt_r < cnt - 500
    k, out = _indirect(eng, torch, rev, n, count, W, H)
    assert k == cnt_r and np.array_equal(out[n:n + cnt_r], rows_r)
    assert (out["PixelIndex"][n + cnt_r:] == 0xFFFFFFFF).all()
    assert not np.isin(rev["PixelIndex"][count:n], out["PixelIndex"][n:n + cnt_r]).any(), "rows past the count"
    # and a count inside the second tile of the frame's own order, where survivors lie past it
    count2 = 4500
    rows_2, cnt_2, _ = BC.expected_enqueue(ref, count2, 0, W, H, FRAMES, MAXB)
    assert cnt_2 < cnt - 300
    k, out = _indirect(eng, torch, ref, n, count2, W, H)
    assert k == cnt_2 and np.array_equal(out[n:n + cnt_2], rows_2)
    assert (out["PixelIndex"][n + cnt_2:] == 0xFFFFFFFF).all()


# 3 ---------------------------------------------------------------- batched frames
def test_batched_frames_draw_per_frame():
    """Two 64 x 64 frames stacked on a 64 x 128 screen with tt_ctx_set_frame_pixels(W H): frame 1's terrain rows
    equal those of the frame enqueued alone at frames + 1 (PixelIndex apart)."""
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    W = H = 64
    n = W * H
    ref, _ = BC.primary(W, H)
    e = tthip.Engine(0)
    try:
        e.upload(TC.scene())
        e.upload_terrains(TC.terrains(), TC.atlas())
        alone = []
        for b in range(2):
            r = ref.copy()
            k = e.enqueue_bounce(r, n, 0, TC.FAR, W, H, frames=FRAMES + b, max_bounce=MAXB, terrain_bounce=True)
            alone.append(r[n:n + k].copy())
        e.set_frame_pixels(n)
        stacked = np.zeros(4 * n, tthip.RAY_DTYPE)
        stacked[:n] = ref[:n]
        stacked[n:2 * n] = ref[:n]
        stacked["PixelIndex"][n:2 * n] += n
        k = e.enqueue_bounce(stacked, 2 * n, 0, TC.FAR, W, 2 * H, frames=FRAMES, max_bounce=MAXB, terrain_bounce=True)
        assert k == len(alone[0]) + len(alone[1])
        got = stacked[2 * n:2 * n + k]
        want1 = alone[1].copy()
        want1["PixelIndex"] += n
        assert np.array_equal(got[:len(alone[0])], alone[0])
        assert np.array_equal(got[len(alone[0]):], want1)
        ter1 = want1["hits"][:, 0] == TID
        assert ter1.sum() > 500 and not np.array_equal(alone[0]["direction"], alone[1]["direction"][:len(alone[0])])
        # and against the two references, frame by frame
        rows, cnt, _ = BC.expected_enqueue_batched(stacked, 2 * n, W, H, 2, FRAMES, MAXB)
        assert cnt == k and np.array_equal(got, rows)
    finally:
        e.close()


# 4 ---------------------------------------------------------------- nothing existing changes
def test_flag_without_terrains_and_terrains_without_flag_are_todays_call(eng, plain):
    W = H = 64
    n = W * H
    ref, _ = BC.primary(W, H)
    # today's call on a context with terrains: terrain rows end (tests/test_gpu_terrain.py's expectation)
    want_rays = ref.copy()
    ter = want_rays["hits"][:n, 0] == TID
    want_rays["hits"][:n][ter, 2] = np.float32(TC.FAR).view(np.uint32)
    want = O.enqueue_bounce(TC.scene(), want_rays, n, 0, TC.FAR, W, H, frames=FRAMES, max_bounce=MAXB)
    clear = ref.copy()
    got = eng.enqueue_bounce(clear, n, 0, TC.FAR, W, H, frames=FRAMES, max_bounce=MAXB)
    assert got == want and np.array_equal(clear[n:n + got], want_rays[n:n + got])
    assert not (clear["hits"][n:n + got, 0] == TID).any()
    # a context without a terrain set: the flag changes nothing (records with mesh 9999999 made triangle misses,
    # as that context would index _MeshData with them otherwise)
    base = want_rays.copy()
    base[n:] = ref[n:]
    a, b = base.copy(), base.copy()
    ka = plain.enqueue_bounce(a, n, 0, TC.FAR, W, H, frames=FRAMES, max_bounce=MAXB)
    kb = plain.enqueue_bounce(b, n, 0, TC.FAR, W, H, frames=FRAMES, max_bounce=MAXB, terrain_bounce=True)
    assert ka == kb == want and np.array_equal(a, b)
    assert np.array_equal(a[n:n + ka], want_rays[n:n + want])


# 5 ---------------------------------------------------------------- malformed input
def test_terrain_record_past_the_set_ends_its_path(eng):
    W = H = 64
    n = W * H
    ref, _ = BC.primary(W, H)
    rays = ref.copy()
    ter = np.nonzero(rays["hits"][:n, 0] == TID)[0]
    bad = ter[::7]
    rays["hits"][bad, 1] = len(TC.terrains())  # triangle_id = n_terrains
    rays["hits"][ter[3], 1] = 0xFFFFFFFF
    rows, cnt, _ = BC.expected_enqueue(rays, n, 0, W, H, FRAMES, MAXB)
    assert not np.isin(rows["PixelIndex"], rays["PixelIndex"][bad]).any()
    work = rays.copy()
    got = eng.enqueue_bounce(work, n, 0, TC.FAR, W, H, frames=FRAMES, max_bounce=MAXB, terrain_bounce=True)
    assert got == cnt and np.array_equal(work[n:n + cnt], rows)


# 6 ---------------------------------------------------------------- the whole chain on the device
def test_whole_chain_asynchronous_with_device_counts(eng):
    torch = _torch()
    W = H = 64
    n = W * H
    c2w, ip = BC.camera(W, H)
    full = O.generate(c2w, ip, W, H, NEAR, TC.FAR, jitter=1, frames=FRAMES, max_bounce=MAXB)
    BC.trace_reference(full, n, 0, W, H)
    rows, cnt, n_ter = BC.expected_enqueue(full, n, 0, W, H, FRAMES, MAXB)
    assert n_ter > 500
    want = full.copy()
    want[n:n + cnt] = rows
    BC.trace_reference(want, cnt, 1, W, H)
    assert (want["hits"][n:n + cnt, 0] == TID).sum() > 100, "bounce-1 rays reach the terrains again"
    d = torch.zeros(2 * n * 48, dtype=torch.uint8, device="cuda:0")
    n_next = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    eng.generate(d, c2w, ip, W, H, NEAR, TC.FAR, jitter=1, frames=FRAMES, max_bounce=MAXB, device=True,
                 asynchronous=True)
    eng.trace(d, n, 0, TC.FAR, W, H, device=True, asynchronous=True)
    eng.trace_heightmap(d, n, 0, TC.FAR, W, H, device=True, asynchronous=True)
    eng.enqueue_bounce_indirect(d, None, n, n_next, 0, TC.FAR, W, H, frames=FRAMES, max_bounce=MAXB,
                                terrain_bounce=True)
    eng.trace_indirect(d, n_next, n, 1, TC.FAR, W, H)
    eng.trace_heightmap_indirect(d, n_next, n, 1, TC.FAR, W, H)
    eng.sync()
    out = _host(d, full)
    assert int(n_next.item()) == cnt
    assert np.array_equal(out[:n], full[:n])
    assert np.array_equal(out[n:n + cnt], want[n:n + cnt])


# 7 ---------------------------------------------------------------- tt_trace_heightmap_hits
def test_heightmap_hits_completes_the_closest_hits_stream(eng):
    torch = _torch()
    W = H = 64
    n = W * H
    ref, ref_info = BC.primary(W, H)
    c2w, ip = BC.camera(W, H)
    gen = tthip.camera_rays_host(c2w, ip, W, H, NEAR, TC.FAR)
    d, info = _dev(gen), torch.zeros(n * 4, dtype=torch.int32, device="cuda:0")
    hits = torch.full((n, 4), -1, dtype=torch.int32, device="cuda:0")
    p = tthip.TraceParams(n_rays=n, bounce=0, far_plane=TC.FAR, screen_width=W, screen_height=H,
                          flags=tthip.TT_TRACE_DEVICE_PTRS)
    import ctypes as C

    assert eng.L.tt_trace_closest_hits(eng.h, C.byref(p), d.data_ptr(), info.data_ptr(), None, hits.data_ptr()) == 0
    eng.trace_heightmap_hits(d, hits, n, 0, TC.FAR, W, H, info=info)
    out = _host(d, gen)
    got_hits = hits.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_hits, out["hits"][:n]) and np.array_equal(out[:n], ref[:n])
    assert np.array_equal(info.cpu().numpy().view(np.uint32).reshape(n, 4), ref_info)
    # the heightmap call alone over a canary: only the rays the reference rewrites change
    tri = gen.copy()
    assert O.trace(TC.scene(), tri, n, 0, TC.FAR, W, H)[0] == 0
    rewritten = (ref["hits"][:n] != tri["hits"][:n]).any(axis=1)
    assert 500 < rewritten.sum() < n
    canary = torch.full((n, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    eng.trace_heightmap_hits(_dev(tri), canary, n, 0, TC.FAR, W, H, asynchronous=True)
    eng.sync()
    c = canary.cpu().numpy().view(np.uint32)
    assert (c[~rewritten] == 0x5A5A5A5A).all() and np.array_equal(c[rewritten], ref["hits"][:n][rewritten])
    # the odd half: ray i of the launch, not of the buffer
    m, off = TC.N_RANDOM, TC.RW * TC.RH
    odd = np.zeros(2 * off, tthip.RAY_DTYPE)
    odd[off:off + m] = TC.random_rays()
    want = odd.copy()
    tthip.terrain_trace_host(TC.terrains(), TC.atlas(), want, m, 1, TC.FAR, TC.RW, TC.RH)
    hit1 = (want["hits"][off:off + m] != odd["hits"][off:off + m]).any(axis=1)
    canary = torch.full((m, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    d_odd = _dev(odd)
    eng.trace_heightmap_hits(d_odd, canary, m, 1, TC.FAR, TC.RW, TC.RH)
    c = canary.cpu().numpy().view(np.uint32)
    assert np.array_equal(_host(d_odd, odd), want)
    assert (c[~hit1] == 0x5A5A5A5A).all() and np.array_equal(c[hit1], want["hits"][off:off + m][hit1])


def test_heightmap_hits_refusals(eng):
    torch = _torch()
    W = H = 64
    n = W * H
    ref, _ = BC.primary(W, H)
    d = _dev(ref)
    hits = torch.zeros((n + 1, 4), dtype=torch.int32, device="cuda:0")
    host_hits = np.zeros((n, 4), np.uint32)
    bad = tthip.TT_ERR_INVALID_ARG
    assert eng.trace_heightmap_hits(d, host_hits, n, 0, TC.FAR, W, H, check=False) == bad          # a host pointer
    assert eng.trace_heightmap_hits(d, hits.data_ptr() + 4, n, 0, TC.FAR, W, H, check=False) == bad  # misaligned
    assert eng.trace_heightmap_hits(d, hits, n, 0, TC.FAR, W, H, flags=tthip.TT_TRACE_STATS, check=False) == bad
    assert eng.trace_heightmap_hits(ref.copy(), hits, n, 0, TC.FAR, W, H, device=False, check=False) == bad
    assert eng.trace_heightmap_hits(d, None, n, 0, TC.FAR, W, H, check=False) == bad
    assert np.array_equal(_host(d, ref), ref), "a refused call writes nothing"
