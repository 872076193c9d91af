"""GPU parity of the heightmap kernels (csrc/tt_terrain.hip) with the scalar host reference
(host/tt_terrain.cpp), bit for bit, on the scene of tests/terrain_cases.py: a Cornell box standing on terrain 0,
terrain 1 overlapping it in x, a 64 x 48 atlas with both rectangles away from its origin.

The shadow accumulations (IntersectionKernels.compute:573-591) are built here in numpy from the reference's
occlusion answers with the encoders the oracle's Python module exports."""
import functools

import numpy as np
import pytest

import oracle_ctypes as O
import terrain_cases as TC
import tthip

pytestmark = pytest.mark.gpu
TID = tthip.TT_TERRAIN_MESH_ID
W = H = 64
NEAR = 0.3


@pytest.fixture(scope="module")
def eng():
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    e = tthip.Engine(0)
    e.upload(TC.scene())
    e.upload_terrains(TC.terrains(), TC.atlas())
    yield e
    e.close()


def _dev(a):
    import torch

    return torch.from_numpy(a.view(np.uint8).reshape(-1)).to("cuda:0")


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


# ------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def primary():
    """The 64 x 64 frame at bounce 0: rays, the triangle oracle's records + info, the terrain reference's."""
    c2w, ip = tthip.unity_camera((0.5, 3.5, 8.0), (0.05, -0.42, -1.0), (0, 1, 0), 50, W, H, NEAR, TC.FAR)
    gen = tthip.camera_rays_host(c2w, ip, W, H, NEAR, TC.FAR)
    tri, tri_info = gen.copy(), np.zeros((W * H, 4), np.uint32)
    assert O.trace(TC.scene(), tri, W * H, 0, TC.FAR, W, H, info=tri_info)[0] == 0
    ref, ref_info = tri.copy(), tri_info.copy()
    stats = tthip.terrain_trace_host(TC.terrains(), TC.atlas(), ref, W * H, 0, TC.FAR, W, H, info=ref_info)
    for a in (gen, tri, tri_info, ref, ref_info):
        a.setflags(write=False)
    return gen, tri, tri_info, ref, ref_info, stats


@functools.lru_cache(maxsize=None)
def bounce1(restir: bool):
    """The randomized set at bounce 1 (the odd half of an RW x RH screen's buffer)."""
    n, off = TC.N_RANDOM, TC.RW * TC.RH
    flags = tthip.TT_TRACE_USE_RESTIRGI if restir else 0
    tri = np.zeros(2 * off, tthip.RAY_DTYPE)
    tri[off:off + n] = TC.random_rays()
    colors = np.zeros(off, tthip.COL_DTYPE)
    colors["Data"][:, 3] = -1.0
    tri_info = np.full((off, 4), 0x51515151, np.uint32)
    assert O.trace(TC.scene(), tri, n, 1, TC.FAR, TC.RW, TC.RH, info=tri_info, colors=colors, flags=flags)[0] == 0
    ref, ref_info = tri.copy(), tri_info.copy()
    stats = tthip.terrain_trace_host(TC.terrains(), TC.atlas(), ref, n, 1, TC.FAR, TC.RW, TC.RH, info=ref_info,
                                     flags=flags)
    for a in (tri, tri_info, ref, ref_info):
        a.setflags(write=False)
    return tri, tri_info, ref, ref_info, stats, flags


def _same_stats(s, r):
    assert (s.rays, s.hits, s.node_visits, s.reps_exhausted) == (r.rays, r.hits, r.node_visits, r.reps_exhausted)


# ------------------------------------------------------------------ closest hit
def test_primary_frame_host_pointers_with_stats(eng):
    gen, tri, tri_info, ref, ref_info, rstats = primary()
    rays, info = gen.copy(), np.zeros((W * H, 4), np.uint32)
    eng.trace(rays, W * H, 0, TC.FAR, W, H, info=info)  # the engine's own triangle trace, then the terrains
    assert np.array_equal(rays["hits"], tri["hits"])
    s = eng.trace_heightmap(rays, W * H, 0, TC.FAR, W, H, info=info, stats=True)
    assert np.array_equal(rays, ref) and np.array_equal(info, ref_info)
    _same_stats(s, rstats)
    hit = ref["hits"][: W * H, 0] == TID
    assert 0.2 < hit.mean() < 0.95 and (ref["hits"][: W * H][hit, 1] == 1).any()
    assert (tri["hits"][: W * H, 2].view(np.float32) < TC.FAR).mean() > 0.05  # records arrive with triangle hits


def test_primary_frame_device_pointers(eng):
    _, tri, tri_info, ref, ref_info, _ = primary()
    rays, info = _dev(tri.copy()), _dev(tri_info.copy())
    eng.trace_heightmap(rays, W * H, 0, TC.FAR, W, H, info=info, device=True)
    assert np.array_equal(_host(rays, ref), ref) and np.array_equal(_host(info, ref_info), ref_info)
    rays2 = _dev(tri.copy())  # without the info texture, asynchronously
    eng.trace_heightmap(rays2, W * H, 0, TC.FAR, W, H, device=True, asynchronous=True)
    eng.sync()
    assert np.array_equal(_host(rays2, ref), ref)


@pytest.mark.parametrize("restir", [False, True])
def test_bounce1_randomized_set(eng, restir):
    tri, tri_info, ref, ref_info, rstats, flags = bounce1(restir)
    n = TC.N_RANDOM
    rays, info = tri.copy(), tri_info.copy()
    s = eng.trace_heightmap(rays, n, 1, TC.FAR, TC.RW, TC.RH, info=info, flags=flags, stats=True)
    assert np.array_equal(rays, ref) and np.array_equal(info, ref_info)
    _same_stats(s, rstats)
    assert s.reps_exhausted >= 1
    d_rays, d_info = _dev(tri.copy()), _dev(tri_info.copy())
    eng.trace_heightmap(d_rays, n, 1, TC.FAR, TC.RW, TC.RH, info=d_info, flags=flags, device=True)
    assert np.array_equal(_host(d_rays, ref), ref) and np.array_equal(_host(d_info, ref_info), ref_info)
    assert not np.array_equal(ref_info, tri_info)


@pytest.mark.parametrize("count", [0, 2500])
def test_indirect_count_on_the_device(eng, count):
    import torch

    tri, tri_info, _, _, _, flags = bounce1(False)
    n, off = TC.N_RANDOM, TC.RW * TC.RH
    ref, ref_info = tri.copy(), tri_info.copy()
    tthip.terrain_trace_host(TC.terrains(), TC.atlas(), ref, count, 1, TC.FAR, TC.RW, TC.RH, info=ref_info, flags=flags)
    d_rays, d_info = _dev(tri.copy()), _dev(tri_info.copy())
    n_dev = torch.tensor([count], dtype=torch.int32, device="cuda:0")
    eng.trace_heightmap_indirect(d_rays, n_dev, n, 1, TC.FAR, TC.RW, TC.RH, info=d_info, flags=flags)
    eng.sync()
    assert np.array_equal(_host(d_rays, ref), ref) and np.array_equal(_host(d_info, ref_info), ref_info)
    assert np.array_equal(ref[off + count:], tri[off + count:])  # rays past the count keep their records
    st = eng.trace_heightmap_indirect(tri.copy(), n_dev, n, 1, TC.FAR, TC.RW, TC.RH, check=False)
    assert st == tthip.TT_ERR_INVALID_ARG  # host rays with a device count


def test_persistent_form_matches(eng):
    """The refill kernels (TT_TERRAIN_FORM=persistent, read once per process: a child runs them) write what the
    reference does, stats included."""
    import hashlib
    import os
    import subprocess
    import sys

    tri, tri_info, ref, ref_info, rstats, _ = bounce1(False)
    occ, _ = shadow_occluded()
    vis = np.full((TC.N_SHADOW, 4), SENTINEL, np.float32)
    live = TC.shadow_rays()["t"] != 0
    vis[live] = np.where(occ[live, None] == 1, np.float32(0), np.float32(1))
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "terrain_form_child.py")
    r = subprocess.run([sys.executable, child], env=dict(os.environ, TT_TERRAIN_FORM="persistent"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1].split()[1:]
    assert got == [hashlib.sha1(ref.tobytes() + ref_info.tobytes()).hexdigest(), hashlib.sha1(vis.tobytes()).hexdigest(),
                   str(rstats.hits), str(rstats.node_visits), str(rstats.reps_exhausted)]


# ------------------------------------------------------------------ shadow
SENTINEL = np.float32(-7.5)


def _shadow_inputs():
    rng = np.random.default_rng(0x7E44A5)
    n_pix = TC.SW * TC.SH
    colors = np.zeros(n_pix, tthip.COL_DTYPE)
    colors["Direct"] = rng.uniform(0, 2, (n_pix, 3))
    colors["Indirect"] = rng.uniform(0, 2, (n_pix, 3))
    colors["PrimaryNEERay"] = [O.pack_rgbe(v) for v in rng.uniform(0, 3, (n_pix, 3)).astype(np.float32)]
    colors["Data"][:, 3] = -1.0
    cache = np.zeros(n_pix, tthip.CACHE_DTYPE)
    cache["CurrentIlluminance"] = [O.encode_rgb(v) for v in rng.uniform(0, 3, (n_pix, 3)).astype(np.float32)]
    nee = np.full((n_pix, 4), SENTINEL, np.float32)
    vis = np.full((TC.N_SHADOW, 4), SENTINEL, np.float32)
    return colors, cache, nee, vis


_SHADOW_IN = None


def shadow_inputs():
    global _SHADOW_IN
    if _SHADOW_IN is None:
        _SHADOW_IN = _shadow_inputs()
    return tuple(a.copy() for a in _SHADOW_IN)


@functools.lru_cache(maxsize=None)
def shadow_occluded(n: int = TC.N_SHADOW):
    occ, stats = tthip.terrain_occluded_host(TC.terrains(), TC.atlas(), TC.shadow_rays()[:n].copy(), n)
    return occ, stats


def shadow_expected(s, occ, bounce, rc, restir, n=None):
    """:573-591 in float32 numpy, on copies of shadow_inputs()."""
    colors, cache, nee, vis = shadow_inputs()
    f32 = np.float32
    inv22 = f32(1.0) / f32(2.2)
    n = len(s) if n is None else n
    for i in range(n):
        t = s["t"][i]
        if not (t != 0):
            continue
        vis[i] = 0.0 if occ[i] else 1.0
        if occ[i]:
            continue
        pix = int(s["PixelIndex"][i])
        il = s["illumination"][i].astype(f32)
        if bounce == 0:
            nee[pix, :3] = s["origin"][i] + s["direction"][i] * np.abs(t)
            nee[pix, 3] = 0.0
        if rc:
            k = f32(1.0) if (not restir or t >= 0) else O.unpack_rgbe(int(s["LuminanceIncomming"][i:i + 1].view(np.uint32)[0]))
            cache["CurrentIlluminance"][pix] = O.encode_rgb(O.decode_rgb(int(cache["CurrentIlluminance"][pix])) + il * k)
        if t >= 0:
            if bounce == 0:
                colors["Direct"][pix] += il
            elif not rc:
                colors["Indirect"][pix] += il
        elif bounce != 0 and restir:
            colors["Indirect"][pix] += il
        else:
            p = O.unpack_rgbe(int(colors["PrimaryNEERay"][pix]))
            v = f32([f32(O.hlsl_pow(p[c], 2.2)) + f32(O.hlsl_pow(il[c], inv22)) for c in range(3)])
            colors["PrimaryNEERay"][pix] = O.pack_rgbe(v)
    return colors, cache, nee, vis


@pytest.mark.parametrize("restir", [False, True])
@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("bounce", [0, 1])
def test_shadow_all_outputs(eng, bounce, rc, restir):
    s = TC.shadow_rays().copy()
    occ, _ = shadow_occluded()
    flags = (tthip.TT_SHADOW_RADIANCE_CACHE if rc else 0) | (tthip.TT_TRACE_USE_RESTIRGI if restir else 0)
    e_col, e_cache, e_nee, e_vis = shadow_expected(s, occ, bounce, rc, restir)
    colors, cache, nee, vis = shadow_inputs()
    eng.shadow_heightmap(s, TC.N_SHADOW, bounce, TC.SW, TC.SH, visibility=vis, colors=colors, nee_pos=nee, cache=cache,
                         flags=flags)
    assert np.array_equal(s, TC.shadow_rays()), "an occluded ray keeps its t: the rays are not written"
    assert np.array_equal(vis, e_vis)
    assert np.array_equal(nee, e_nee)
    assert np.array_equal(colors, e_col)
    assert np.array_equal(cache, e_cache)
    if bounce == 0 and not rc and not restir:  # the inputs exercise every branch
        live = (s["t"] != 0) & (occ == 0)
        assert (occ == 1).sum() > 200 and (live & (s["t"] > 0)).sum() > 200 and (live & (s["t"] < 0)).sum() > 200
        assert (vis[s["t"] == 0] == SENTINEL).all()


def test_shadow_device_pointers_indirect_and_null_outputs(eng):
    import torch

    s = TC.shadow_rays().copy()
    flags = tthip.TT_SHADOW_RADIANCE_CACHE
    count = 3001
    occ, _ = shadow_occluded()
    e_col, e_cache, e_nee, e_vis = shadow_expected(s, occ, 0, True, False, n=count)
    colors, cache, nee, vis = shadow_inputs()
    d = [_dev(a) for a in (s, vis, colors, nee, cache)]
    n_dev = torch.tensor([count], dtype=torch.int32, device="cuda:0")
    eng.shadow_heightmap(d[0], TC.N_SHADOW, 0, TC.SW, TC.SH, visibility=d[1], colors=d[2], nee_pos=d[3], cache=d[4],
                         flags=flags, n_rays_dev=n_dev)
    eng.sync()
    assert np.array_equal(_host(d[1], vis), e_vis) and np.array_equal(_host(d[3], nee), e_nee)
    assert np.array_equal(_host(d[2], colors), e_col) and np.array_equal(_host(d[4], cache), e_cache)
    # every output NULL: the call marches and writes nothing; visibility alone; colours alone
    eng.shadow_heightmap(s, TC.N_SHADOW, 0, TC.SW, TC.SH, flags=flags)
    assert np.array_equal(s, TC.shadow_rays())
    f_col, _, _, f_vis = shadow_expected(s, occ, 0, True, False)
    vis2 = shadow_inputs()[3]
    eng.shadow_heightmap(s, TC.N_SHADOW, 0, TC.SW, TC.SH, visibility=vis2, flags=flags)
    assert np.array_equal(vis2, f_vis)
    col2 = shadow_inputs()[0]
    eng.shadow_heightmap(_dev(s), TC.N_SHADOW, 0, TC.SW, TC.SH, flags=flags, device=True)
    d_col = _dev(col2)
    eng.shadow_heightmap(_dev(s), TC.N_SHADOW, 0, TC.SW, TC.SH, colors=d_col, flags=flags, device=True)
    assert np.array_equal(_host(d_col, col2), f_col)
    p = tthip.ShadowParams(n_rays=TC.N_SHADOW, bounce=0, screen_width=TC.SW, screen_height=TC.SH,
                           flags=tthip.TT_SHADOW_VISIBILITY_CHECK)
    import ctypes as C

    assert eng.L.tt_trace_shadow_heightmap(eng.h, C.byref(p), s.ctypes.data, None, None, None, None) == \
        tthip.TT_ERR_INVALID_ARG


def test_kernel_shadow_then_heightmap_pair(eng):
    """The reference's TerrainExists form of kernel_shadow: tt_trace_shadow_ex with NULL accumulation outputs zeroes
    the t of rays a triangle occludes, then tt_trace_shadow_heightmap accumulates the rays nothing occludes."""
    s0 = TC.shadow_rays().copy()
    after_tri = s0.copy()
    assert O.shadow(TC.scene(), after_tri, TC.N_SHADOW, 0, TC.SW, TC.SH)[0] == 0
    tri_occ = (after_tri["t"] == 0) & (s0["t"] != 0)
    ter_occ, _ = tthip.terrain_occluded_host(TC.terrains(), TC.atlas(), after_tri, TC.N_SHADOW)
    ter_only, _ = shadow_occluded()
    assert (tri_occ & (ter_only == 0)).sum() > 20, "rays only a triangle blocks"
    assert ((ter_occ == 1) & ~tri_occ).sum() > 200, "rays only the terrain blocks"
    e_col, e_cache, e_nee, e_vis = shadow_expected(after_tri, ter_occ, 0, True, False)
    s = s0.copy()
    colors, cache, nee, vis = shadow_inputs()
    eng.trace_shadow(s, TC.N_SHADOW, 0, TC.SW, TC.SH, flags=tthip.TT_SHADOW_RADIANCE_CACHE)
    assert np.array_equal(s, after_tri)
    eng.shadow_heightmap(s, TC.N_SHADOW, 0, TC.SW, TC.SH, visibility=vis, colors=colors, nee_pos=nee, cache=cache,
                         flags=tthip.TT_SHADOW_RADIANCE_CACHE)
    assert np.array_equal(s, after_tri)
    assert np.array_equal(vis, e_vis) and np.array_equal(nee, e_nee)
    assert np.array_equal(colors, e_col) and np.array_equal(cache, e_cache)


# ------------------------------------------------------------------ resolve, enqueue
def test_resolve_normals_on_terrain_hits(eng):
    _, _, _, ref, _, _ = primary()
    n = W * H
    out = eng.resolve_normals(ref.copy(), n, 0, TC.FAR, W, H)
    hits = ref["hits"][:n]
    ter = np.nonzero(hits[:, 0] == TID)[0]
    assert len(ter) > 500
    t = hits[:, 2].view(np.float32)
    pos = ref["direction"][:n] * t[:, None] + ref["origin"][:n]
    for i in ter[:: max(1, len(ter) // 400)]:
        nn = tthip.terrain_normal_host(TC.terrains(), TC.atlas(), pos[i], int(hits[i, 1]))
        assert np.abs(out[i, :3] - nn).max() <= 1e-5 and np.abs(out[i, 3:] - nn).max() <= 1e-5, i
    assert np.abs(np.linalg.norm(out[ter, :3], axis=1) - 1).max() < 1e-5
    # triangle hits and misses are resolved as before
    tri_rows = np.nonzero((hits[:, 0] != TID) & (t < TC.FAR))[0]
    want = O.resolve_normals(TC.scene(), ref.copy(), n, 0, TC.FAR, W, H)
    assert len(tri_rows) > 50 and np.abs(out[tri_rows] - want[tri_rows]).max() <= 1e-5
    assert not out[t >= TC.FAR].any()


def test_enqueue_terminates_terrain_hits(eng):
    _, _, _, ref, _, _ = primary()
    n = W * H
    rays = ref.copy()
    got = eng.enqueue_bounce(rays, n, 0, TC.FAR, W, H, frames=3, max_bounce=4)
    want_rays = ref.copy()
    ter = want_rays["hits"][:n, 0] == TID
    want_rays["hits"][:n][ter, 2] = np.float32(TC.FAR).view(np.uint32)  # as a miss: the path ends
    want = O.enqueue_bounce(TC.scene(), want_rays, n, 0, TC.FAR, W, H, frames=3, max_bounce=4)
    assert got == want and 0 < got < n - ter.sum() + 1
    assert np.array_equal(rays[n:n + got], want_rays[n:n + got])
    assert not (rays["hits"][n:n + got, 0] == TID).any()


# ------------------------------------------------------------------ lifecycle
def test_no_terrain_set_is_no_scene_and_changes_nothing():
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    gen, tri, _, ref, _, _ = primary()
    n = W * H
    e = tthip.Engine(0)
    try:
        e.upload(TC.scene())
        bytes0 = e.scene_bytes()
        rays = tri.copy()
        _, st = e.trace_heightmap(rays, n, 0, TC.FAR, W, H, check=False)
        assert st == tthip.TT_ERR_NO_SCENE and "terrain" in e.L.tt_last_error(e.h).decode()
        s = TC.shadow_rays().copy()
        assert e.shadow_heightmap(s, TC.N_SHADOW, 0, TC.SW, TC.SH, check=False) == tthip.TT_ERR_NO_SCENE

        def outputs():
            r = gen.copy()
            info = np.zeros((n, 4), np.uint32)
            e.trace(r, n, 0, TC.FAR, W, H, info=info)
            normals = e.resolve_normals(ref.copy(), n, 0, TC.FAR, W, H)  # (records with mesh 9999999 included)
            b = ref.copy()
            b["hits"][:n][ref["hits"][:n, 0] == TID] = tri["hits"][:n][ref["hits"][:n, 0] == TID]
            cnt = e.enqueue_bounce(b, n, 0, TC.FAR, W, H, frames=1, max_bounce=3)
            return r, info, normals, b, cnt

        before = outputs()
        assert not before[2][ref["hits"][:n, 0] == TID].any()  # no terrain set: such a record resolves to zeros
        assert e.upload_terrains(TC.terrains(), TC.atlas()) == tthip.TT_OK
        assert e.scene_bytes() == bytes0 + TC.atlas().nbytes + TC.terrains().nbytes
        e.upload_terrains(None)  # n = 0 clears the set
        assert e.scene_bytes() == bytes0
        after = outputs()
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        assert e.trace_heightmap(tri.copy(), n, 0, TC.FAR, W, H, check=False)[1] == tthip.TT_ERR_NO_SCENE
        bad = TC.terrains().copy()
        bad[1]["HeightMap"][0] = 1.5
        assert e.upload_terrains(bad, TC.atlas(), check=False) == tthip.TT_ERR_INVALID_ARG
        assert "HeightMap" in e.L.tt_last_error(e.h).decode()
    finally:
        e.close()


def test_borrower_traces_the_lenders_terrains(eng):
    _, tri, tri_info, ref, ref_info, _ = primary()
    n = W * H
    b = tthip.Engine(0)
    try:
        b.share_scene(eng)
        rays, info = tri.copy(), tri_info.copy()
        b.trace_heightmap(rays, n, 0, TC.FAR, W, H, info=info)
        assert np.array_equal(rays, ref) and np.array_equal(info, ref_info)
        # the set belongs to the lender's scene: neither side may replace it while it is shared
        assert eng.upload_terrains(TC.terrains(), TC.atlas(), check=False) == tthip.TT_ERR_INVALID_ARG
        assert b.upload_terrains(TC.terrains(), TC.atlas(), check=False) == tthip.TT_ERR_INVALID_ARG
    finally:
        b.close()
    assert eng.upload_terrains(TC.terrains(), TC.atlas()) == tthip.TT_OK
