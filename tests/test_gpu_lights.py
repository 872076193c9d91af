"""tt_emit_nee on the device against its scalar host reference (tt_emit_nee_host), byte for byte, over the light
scenes L1 / L2 / L3 and every ray set of tests/lights_cases.py, in every call form; the float64 pin of
tests/lights.py on the device's output; the chain into tt_trace_shadow_ex_indirect; and the lights' life with the
scene (sharing, frame slots, groups, re-upload, TLAS-part rewrites)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lights_cases as LC
import oracle_ctypes as O
import terrain_cases as TC
import tthip

pytestmark = pytest.mark.gpu

POISON = 0xCD


@pytest.fixture(scope="module")
def engines():
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    made = {}
    for name, fn in LC.CASES.items():
        case = fn()
        e = tthip.Engine(0)
        e.upload(case.scene)
        e.upload_lights(case.lights)
        made[name] = e
    yield made
    for e in made.values():
        e.close()


_REF = {}


def reference(name, key, flags=0, frame_pixels=0, terrains=False):
    k = (name, key, flags, frame_pixels, terrains)
    if k not in _REF:
        case = LC.CASES[name]()
        rays, n, bounce, w, h = LC.ray_sets(name)[key]
        _REF[k] = tthip.emit_nee_host(case.lights, case.scene, rays, n, bounce, LC.FAR, w, h, frames=LC.FRAMES,
                                      max_bounce=LC.MAX_BOUNCE, frame_pixels=frame_pixels, terrains=terrains, flags=flags)
    return _REF[k]


def poisoned(n, dtype):
    a = np.zeros(max(n, 1), dtype)
    a.view(np.uint8)[:] = POISON
    return a


def dev(a):
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def back(t, dtype):
    return t.cpu().numpy().view(dtype)


def same(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_output(smp, sh, cnt, ref_smp, ref_sh, n):
    assert cnt == len(ref_sh)
    assert same(smp[:n], ref_smp), "samples differ from tt_emit_nee_host"
    assert same(sh[:cnt], ref_sh), "shadow rays differ from tt_emit_nee_host"
    assert (sh[cnt:].view(np.uint8) == POISON).all(), "rows past n_shadow were written"
    miss = ref_smp["light_tri"] < 0
    gone = miss & (ref_smp["steps"] == 0)
    minus1 = np.zeros(1, tthip.LIGHT_SAMPLE_DTYPE)
    minus1["light_tri"] = minus1["mesh_index"] = minus1["agg_tri"] = -1
    assert smp[:n][gone].tobytes() == minus1.tobytes() * int(gone.sum()), "a missed ray's sample is not the -1 record"


@pytest.mark.parametrize("key", ["b0", "b1", "ragged"])
@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_emit_equals_the_host_reference_in_every_form(engines, name, key):
    e = engines[name]
    rays, n, bounce, w, h = LC.ray_sets(name)[key]
    ref_smp, ref_sh = reference(name, key)
    assert n > 0
    kw = dict(frames=LC.FRAMES, max_bounce=LC.MAX_BOUNCE)
    # host pointers
    smp, sh = poisoned(n, tthip.LIGHT_SAMPLE_DTYPE), poisoned(n, tthip.SHADOW_DTYPE)
    cnt = e.emit_nee(rays, n, bounce, LC.FAR, w, h, samples=smp, shadow_rays=sh, **kw)
    check_output(smp, sh, cnt, ref_smp, ref_sh, n)
    # device pointers, synchronous; then asynchronous; then the device-count form with a count below the capacity
    d_rays = dev(rays)
    for form in ("device", "async", "indirect"):
        d_smp, d_sh = dev(poisoned(n, tthip.LIGHT_SAMPLE_DTYPE)), dev(poisoned(n, tthip.SHADOW_DTYPE))
        if form == "device":
            cnt = e.emit_nee(d_rays, n, bounce, LC.FAR, w, h, samples=d_smp, shadow_rays=d_sh, device=True, **kw)
        elif form == "async":
            assert e.emit_nee(d_rays, n, bounce, LC.FAR, w, h, samples=d_smp, shadow_rays=d_sh, device=True,
                              asynchronous=True, **kw) is None
            e.sync()
            cnt = len(ref_sh)
        else:
            d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
            d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            cap = min(w * h, n + 100)  # the capacity exceeds the count: the clamp is the device's
            d_smp, d_sh = dev(poisoned(cap, tthip.LIGHT_SAMPLE_DTYPE)), dev(poisoned(cap, tthip.SHADOW_DTYPE))
            e.emit_nee_indirect(d_rays, d_n, cap, d_cnt, bounce, LC.FAR, w, h, samples=d_smp, shadow_rays=d_sh, **kw)
            e.sync()
            cnt = int(d_cnt.item())
            assert (back(d_smp, tthip.LIGHT_SAMPLE_DTYPE)[n:].view(np.uint8) == POISON).all()
        check_output(back(d_smp, tthip.LIGHT_SAMPLE_DTYPE), back(d_sh, tthip.SHADOW_DTYPE), cnt, ref_smp, ref_sh, n)


def test_negative_t_flips_only_the_sign_and_frame_pixels_are_the_enqueues(engines):
    e = engines["L1"]
    rays, n, bounce, w, h = LC.ray_sets("L1")["ragged"]
    kw = dict(frames=LC.FRAMES, max_bounce=LC.MAX_BOUNCE)
    ref_smp, ref_sh = reference("L1", "ragged")
    smp, sh = poisoned(n, tthip.LIGHT_SAMPLE_DTYPE), poisoned(n, tthip.SHADOW_DTYPE)
    cnt = e.emit_nee(rays, n, bounce, LC.FAR, w, h, samples=smp, shadow_rays=sh, flags=tthip.TT_NEE_NEGATIVE_T, **kw)
    flipped = ref_sh.copy()
    flipped["t"] = -flipped["t"]
    assert (ref_sh["t"] > 0).all()
    check_output(smp, sh, cnt, ref_smp, flipped, n)
    # batched frames: the second copy of the frame carries PixelIndex + W H, frame-local with frame_pixels = W H
    fp = LC.W * LC.H
    fp_smp, fp_sh = reference("L1", "ragged", frame_pixels=fp)
    assert len(fp_sh) != len(ref_sh) or not same(fp_sh, ref_sh), "frame-local pixels draw other random numbers"
    e.set_frame_pixels(fp)
    try:
        smp, sh = poisoned(n, tthip.LIGHT_SAMPLE_DTYPE), poisoned(n, tthip.SHADOW_DTYPE)
        cnt = e.emit_nee(rays, n, bounce, LC.FAR, w, h, samples=smp, shadow_rays=sh, **kw)
    finally:
        e.set_frame_pixels(0)
    check_output(smp, sh, cnt, fp_smp, fp_sh, n)
    assert np.array_equal(sh["PixelIndex"][:cnt], fp_sh["PixelIndex"])


def test_terrain_records_and_misses_emit_nothing():
    case = LC.l1_room()
    rays, n, bounce, w, h = LC.ray_sets("L1")["b0"]
    rays = rays.copy()
    rays["hits"][5:400:7, 0] = tthip.TT_TERRAIN_MESH_ID
    rays["hits"][5:400:7, 1] = 1
    e = tthip.Engine(0)
    try:
        e.upload(case.scene)
        e.upload_terrains(TC.terrains(), TC.atlas())
        e.upload_lights(case.lights)
        ref_smp, ref_sh = tthip.emit_nee_host(case.lights, case.scene, rays, n, bounce, LC.FAR, w, h, frames=LC.FRAMES,
                                              max_bounce=LC.MAX_BOUNCE, terrains=True)
        assert (ref_smp["light_tri"][5:400:7] == -1).all() and (ref_smp["steps"][5:400:7] == 0).all()
        smp, sh = poisoned(n, tthip.LIGHT_SAMPLE_DTYPE), poisoned(n, tthip.SHADOW_DTYPE)
        cnt = e.emit_nee(rays, n, bounce, LC.FAR, w, h, frames=LC.FRAMES, max_bounce=LC.MAX_BOUNCE, samples=smp, shadow_rays=sh)
        check_output(smp, sh, cnt, ref_smp, ref_sh, n)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["L1", "L3"])
def test_float64_pin_on_the_device_output(engines, name):
    import lights

    case = LC.CASES[name]()
    for key in ("b0", "b1"):
        rays, n, bounce, w, h = LC.ray_sets(name)[key]
        smp, sh = poisoned(n, tthip.LIGHT_SAMPLE_DTYPE), poisoned(n, tthip.SHADOW_DTYPE)
        cnt = engines[name].emit_nee(rays, n, bounce, LC.FAR, w, h, frames=LC.FRAMES, max_bounce=LC.MAX_BOUNCE,
                                     samples=smp, shadow_rays=sh)
        off = w * h if bounce % 2 else 0
        got = lights.pin(case, rays[off: off + n], bounce, LC.FAR, LC.FRAMES, LC.MAX_BOUNCE, smp, sh[:cnt])
        ref_smp, ref_sh = reference(name, key)
        want = lights.pin(case, rays[off: off + n], bounce, LC.FAR, LC.FRAMES, LC.MAX_BOUNCE, ref_smp, ref_sh)
        assert got.ok, got.lines()
        assert got.lines() == want.lines()


def test_chain_into_the_indirect_shadow_trace(engines):
    """Generate -> trace -> tt_emit_nee_indirect -> tt_trace_shadow_ex_indirect with no host round trip: the
    visibility rows equal the host reference's rays traced by the oracle's any-hit."""
    case = LC.l1_room()
    e = engines["L1"]
    c2w, ip = LC.camera(case)
    n = LC.W * LC.H
    d_rays = torch.zeros(2 * n * 48, dtype=torch.uint8, device="cuda")
    e.generate(d_rays, c2w, ip, LC.W, LC.H, LC.NEAR, LC.FAR, jitter=1, frames=LC.FRAMES, max_bounce=LC.MAX_BOUNCE, device=True)
    e.trace(d_rays, n, 0, LC.FAR, LC.W, LC.H, device=True)
    host_rays = back(d_rays, tthip.RAY_DTYPE)
    assert same(host_rays[:n], LC.ray_sets("L1")["b0"][0][:n]), "the device's records are the oracle's"
    d_sh = dev(poisoned(n, tthip.SHADOW_DTYPE))
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_vis = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    e.emit_nee_indirect(d_rays, None, n, d_cnt, 0, LC.FAR, LC.W, LC.H, frames=LC.FRAMES, max_bounce=LC.MAX_BOUNCE, shadow_rays=d_sh)
    e.trace_shadow_indirect(d_sh, d_cnt, n, 0, LC.W, LC.H, visibility=d_vis)
    e.sync()
    ref_smp, ref_sh = reference("L1", "b0")
    cnt = int(d_cnt.item())
    assert cnt == len(ref_sh)
    vis = d_vis.cpu().numpy()[:cnt]
    want = ref_sh.copy()
    ovis = np.zeros((cnt, 4), np.float32)
    O.shadow(case.scene, want, cnt, 0, LC.W, LC.H, visibility=ovis)
    assert np.array_equal(vis, ovis)
    assert same(back(d_sh, tthip.SHADOW_DTYPE)[:cnt], want), "occluded rays carry t = 0, as the oracle's"
    # panel A (light triangles 0..1 of the room, open) is seen from the floor below it; panel B hangs over a slab
    tri_of_ray = ref_smp["light_tri"][_emitted_sources(ref_smp, ref_sh)]
    room = case.lights.tris[:4]
    on_a = room["pos0"][:, 0] < 0
    a_ids, b_ids = np.nonzero(on_a)[0], np.nonzero(~on_a)[0]
    from_floor = ref_sh["origin"][:, 1] < 0.01
    assert (vis[np.isin(tri_of_ray, a_ids) & from_floor, 3] == 1).any()
    assert (vis[np.isin(tri_of_ray, b_ids) & from_floor, 3] == 0).all() and (np.isin(tri_of_ray, b_ids) & from_floor).any()


def _emitted_sources(smp, sh):
    """Source ray of every emitted shadow ray: emission keeps source order, and an emitted ray's pixel is its source's."""
    src = np.nonzero(smp["light_tri"] >= 0)[0]
    rays = LC.ray_sets("L1")["b0"][0]
    px = rays["PixelIndex"][src]
    pos = {int(p): int(s) for s, p in zip(src, px)}
    return np.array([pos[int(p)] for p in sh["PixelIndex"]], np.int64)


def test_lights_live_with_the_scene(engines):
    case = LC.l1_room()
    lender = engines["L1"]
    rays, n, bounce, w, h = LC.ray_sets("L1")["b0"]
    ref_smp, ref_sh = reference("L1", "b0")
    kw = dict(frames=LC.FRAMES, max_bounce=LC.MAX_BOUNCE)
    borrower, slot, fresh = tthip.Engine(0), tthip.Engine(0), tthip.Engine(0)
    g = None
    try:
        borrower.share_scene(lender)
        smp, sh = poisoned(n, tthip.LIGHT_SAMPLE_DTYPE), poisoned(n, tthip.SHADOW_DTYPE)
        cnt = borrower.emit_nee(rays, n, bounce, LC.FAR, w, h, samples=smp, shadow_rays=sh, **kw)
        check_output(smp, sh, cnt, ref_smp, ref_sh, n)
        borrower.close()
        # a frame slot and a group member carry no lights
        slot.share_blas(lender, case.scene.tlas_nodes)
        st, _ = slot.emit_nee(rays, n, bounce, LC.FAR, w, h, samples=smp, shadow_rays=sh, check=False, **kw)
        assert st == tthip.TT_ERR_UNSUPPORTED
        L = tthip.hip_lib()
        assert b"frame slot" in L.tt_last_error(slot.h)
        slot.close()
        g = tthip.Group(64, 64, devices=[0, 0], copy=True)
        g.upload(case.scene)
        ctx = g.member_ctx(0)
        assert L.tt_scene_upload_lights(ctx, tthip._ptr(case.lights.nodes), len(case.lights.nodes), tthip._ptr(case.lights.tris),
                                        len(case.lights.tris), tthip._ptr(case.lights.meshes), len(case.lights.meshes)) == tthip.TT_ERR_UNSUPPORTED
        p = tthip.TraceParams(n_rays=n, bounce=0, far_plane=LC.FAR, screen_width=w, screen_height=h, flags=0)
        cnt_c = C.c_uint32()
        assert L.tt_emit_nee(ctx, C.byref(p), tthip._ptr(rays), LC.FRAMES, LC.MAX_BOUNCE, None, tthip._ptr(sh), C.byref(cnt_c)) == tthip.TT_ERR_UNSUPPORTED
        assert b"group" in L.tt_last_error(ctx)
        # no lights before an upload, none after the scene is uploaded again
        fresh.upload(case.scene)
        st, _ = fresh.emit_nee(rays, n, bounce, LC.FAR, w, h, shadow_rays=sh, check=False, **kw)
        assert st == tthip.TT_ERR_NO_SCENE
        fresh.upload_lights(case.lights)
        assert fresh.emit_nee(rays, n, bounce, LC.FAR, w, h, shadow_rays=sh, **kw) == len(ref_sh)
        fresh.upload(case.scene)
        st, _ = fresh.emit_nee(rays, n, bounce, LC.FAR, w, h, shadow_rays=sh, check=False, **kw)
        assert st == tthip.TT_ERR_NO_SCENE
    finally:
        if g is not None:
            g.close()
        for x in (borrower, slot, fresh):
            x.close()


def test_update_light_nodes_after_moving_an_instance():
    case = LC.l1_room()
    rays, n, bounce, w, h = LC.ray_sets("L1")["b0"]
    kw = dict(frames=LC.FRAMES, max_bounce=LC.MAX_BOUNCE)
    moved = list(case.instances)
    l2w = moved[3][2].copy()
    l2w[:3, 3] += (1.5, 0.5, 2.0)
    moved[3] = (moved[3][0], moved[3][1], l2w)
    md = case.scene.meshdata.copy()
    md["W2L"][3] = tthip.unity_colmajor(np.linalg.inv(l2w))
    fresh_lights = tthip.lights_assemble(case.parents, moved, md)
    n_tlas = 2 * len(case.lights.meshes)
    assert same(fresh_lights.nodes[n_tlas:], case.lights.nodes[n_tlas:]) and not same(fresh_lights.nodes[:n_tlas], case.lights.nodes[:n_tlas])
    scene2 = tthip.Scene(case.scene.nodes, case.scene.tris, case.scene.tlas, md, case.scene.materials, tlas_nodes=case.scene.tlas_nodes)
    want_smp, want_sh = tthip.emit_nee_host(fresh_lights, scene2, rays, n, bounce, LC.FAR, w, h, **kw)
    e = tthip.Engine(0)
    try:
        e.upload(case.scene)
        e.upload_lights(case.lights)
        e.update_meshdata(3, md[3:4])
        e.update_light_nodes(0, fresh_lights.nodes[:n_tlas])
        smp, sh = poisoned(n, tthip.LIGHT_SAMPLE_DTYPE), poisoned(n, tthip.SHADOW_DTYPE)
        cnt = e.emit_nee(rays, n, bounce, LC.FAR, w, h, samples=smp, shadow_rays=sh, **kw)
        check_output(smp, sh, cnt, want_smp, want_sh, n)
        bad = fresh_lights.nodes[:n_tlas].copy()
        bad["left"][0] = 1
        assert e.update_light_nodes(0, bad, check=False) == tthip.TT_ERR_INVALID_ARG
        cnt = e.emit_nee(rays, n, bounce, LC.FAR, w, h, samples=smp, shadow_rays=sh, **kw)
        assert cnt == len(want_sh), "a refused rewrite leaves the lights as they were"
    finally:
        e.close()
