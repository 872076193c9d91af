"""Expected results of the bounce enqueue with TT_ENQUEUE_TERRAIN_BOUNCE, shared by tests/test_gpu_terrain_bounce.py
and tests/test_gpu_group_terrain.py, built from two references that share no code with the kernels:

  * the oracle's enqueue (oracle/tt_oracle.c) over a copy in which the terrain rows are misses gives the triangle
    survivors in source order, each identified by its unique PixelIndex;
  * the host reference (tt_terrain_bounce_host, host/tt_terrain.cpp) gives the terrain survivors;

merged by source index, which is the order the stable compaction writes. The scene is tests/terrain_cases.py's."""
import functools

import numpy as np

import oracle_ctypes as O
import terrain_cases as TC
import tthip

TID = tthip.TT_TERRAIN_MESH_ID
NEAR = 0.3
CAMERA = ((0.5, 3.5, 8.0), (0.05, -0.42, -1.0), (0, 1, 0), 50)  # the camera of tests/test_gpu_terrain.py's frame


def camera(W, H):
    pos, fwd, up, fov = CAMERA
    return tthip.unity_camera(pos, fwd, up, fov, W, H, NEAR, TC.FAR)


def trace_reference(rays, n, bounce, W, H, info=None):
    """kernel_trace then kernel_heightmap, in place: the oracle's triangle trace and the host terrain march."""
    assert O.trace(TC.scene(), rays, n, bounce, TC.FAR, W, H, info=info)[0] == 0
    tthip.terrain_trace_host(TC.terrains(), TC.atlas(), rays, n, bounce, TC.FAR, W, H, info=info)
    return rays


def expected_enqueue(rays, n, bounce, W, H, frames, max_bounce, terrains=None, n_terrains=None):
    """The compacted survivors of the flagged enqueue over rays' window of `bounce` (a 2 W H array): (rows, count,
    number of terrain rows among them). n_terrains: the terrain count the reference is told (default: all)."""
    T = TC.terrains() if terrains is None else terrains
    if n_terrains is not None:
        T = T[:n_terrains]
    wh = W * H
    src, dst = (wh, 0) if bounce % 2 else (0, wh)
    win = rays[src:src + n]
    pix = win["PixelIndex"].astype(np.int64)
    assert len(np.unique(pix)) == n, "rows are identified by their PixelIndex"
    where = np.full(int(pix.max()) + 1, -1, np.int64)
    where[pix] = np.arange(n)
    tri = rays.copy()
    ter = tri["hits"][src:src + n, 0] == TID
    tri["hits"][src:src + n][ter, 2] = np.float32(TC.FAR).view(np.uint32)  # as a miss: the oracle knows no terrains
    cnt = O.enqueue_bounce(TC.scene(), tri, n, bounce, TC.FAR, W, H, frames=frames, max_bounce=max_bounce)
    tri_rows = tri[dst:dst + cnt]
    tri_src = where[tri_rows["PixelIndex"].astype(np.int64)]
    assert (tri_src >= 0).all() and (np.diff(tri_src) > 0).all(), "the oracle's survivors are in source order"
    out, sv = tthip.terrain_bounce_host(T, TC.atlas(), rays, n, bounce, TC.FAR, W, H, frames=frames,
                                        max_bounce=max_bounce)
    assert ((sv >= 0) == ter).all()
    ter_src = np.nonzero(sv == 1)[0]
    order = np.argsort(np.concatenate([tri_src, ter_src]), kind="stable")
    rows = np.concatenate([tri_rows, out[ter_src]])[order]
    return rows, len(rows), len(ter_src)


def expected_enqueue_batched(rays, n, W, H, batch, frames, max_bounce):
    """The same for a window of `batch` frames stacked on a W x batch H screen (bounce 0; frame b's rows carry
    PixelIndex + b W H and draw at frames + b, tt_ctx_set_frame_pixels(W H)): frame by frame, in source order."""
    wh = W * H
    win = rays[:n]
    fb = win["PixelIndex"] // wh
    assert (np.diff(fb.astype(np.int64)) >= 0).all(), "frame b's rays follow frame b - 1's"
    parts, n_ter = [], 0
    for b in range(batch):
        sel = win[fb == b].copy()
        sel["PixelIndex"] -= b * wh
        one = np.zeros(2 * wh, tthip.RAY_DTYPE)
        one[:len(sel)] = sel
        rows, _, k = expected_enqueue(one, len(sel), 0, W, H, frames + b, max_bounce)
        rows = rows.copy()
        rows["PixelIndex"] += b * wh
        parts.append(rows)
        n_ter += k
    rows = np.concatenate(parts) if parts else np.zeros(0, tthip.RAY_DTYPE)
    return rows, len(rows), n_ter


@functools.lru_cache(maxsize=None)
def primary(W, H):
    """The W x H frame at bounce 0 after kernel_trace + kernel_heightmap (reference), as a 2 W H array, and its
    _PrimaryTriangleInfo."""
    c2w, ip = camera(W, H)
    rays = tthip.camera_rays_host(c2w, ip, W, H, NEAR, TC.FAR)
    info = np.zeros((W * H, 4), np.uint32)
    trace_reference(rays, W * H, 0, W, H, info=info)
    rays.setflags(write=False)
    info.setflags(write=False)
    return rays, info
