"""Every refusal of the launch entry points that valid memory can provoke, by status and tt_last_error text, on
a Cornell box at 8 x 8: the five launch paths (closest hit, any hit, heightmap, shadow heightmap, bounce
enqueue), tt_resolve_normals, tt_generate_primary and the two share calls. The texts are literals: a host may
match on them, so a change of wording or of the order of the checks (csrc/tt_call_host.h, tt_dispatch.hip,
tt_scene_api.hip) has to show up here. No case hands the library unmapped memory: a refused call never reaches
a kernel, and the last test traces on the same contexts to show the refusals left them usable."""
import ctypes as C

import numpy as np
import pytest

import oracle_ctypes as O
import terrain_cases as TC
import tthip

pytestmark = pytest.mark.gpu
W = H = 8
N = W * H
FAR = 1000.0
BAD, NO_SCENE, UNSUP = tthip.TT_ERR_INVALID_ARG, tthip.TT_ERR_NO_SCENE, tthip.TT_ERR_UNSUPPORTED
DEV, STATS, ASYNC = tthip.TT_TRACE_DEVICE_PTRS, tthip.TT_TRACE_STATS, tthip.TT_TRACE_ASYNC

T_NO_SCENE = "no scene uploaded"
T_NO_TERRAIN = "no terrain set uploaded (tt_scene_upload_terrains)"
T_NULL, T_NULL_SH = "null params or rays", "null params or shadow rays"
T_SCREEN0, T_BOUNCE, T_NAN = "zero screen size", "negative bounce", "far_plane is NaN"
T_HOST_RAYS = "TT_TRACE_DEVICE_PTRS set but rays is not device memory"
T_CNT_DEV = "a device-resident ray count needs TT_TRACE_DEVICE_PTRS"
T_CNT_STATS = "TT_TRACE_STATS needs a host ray count"
T_CNT_MEM = "the ray count pointer is not device memory"
T_ALIGN = "GlobalRays / _PrimaryTriangleInfo must be 16-byte aligned"
T_ALIGN_SH = "shadow rays / visibility / NEEPosA must be 16-byte aligned"
T_VIS_CHECK = "TT_SHADOW_VISIBILITY_CHECK has no heightmap form (VisabilityCheckCompute never marches terrains)"


class Ctx:
    """The engines and arrays the cases share (module scope: one upload each)."""

    def __init__(self):
        import torch

        self.torch = torch
        self.scene = tthip.single_object_scene(tthip.Mesh.cornell())
        self.c2w, self.ip = tthip.unity_camera((0, 0, 3.4), (0, 0, -1), (0, 1, 0), 40, W, H, 0.3, FAR)
        self.bare = tthip.Engine(0)                 # no scene, no terrains
        self.eng = tthip.Engine(0)                  # the Cornell box; lends to `bor`
        self.eng.upload(self.scene)
        self.bor = tthip.Engine(0)
        self.bor.share_scene(self.eng)
        self.ter = tthip.Engine(0)                  # the Cornell box on the terrains of terrain_cases
        self.ter.upload(TC.scene())
        self.ter.upload_terrains(TC.terrains(), TC.atlas())
        self.L = self.eng.L
        self.rays = tthip.camera_rays_host(self.c2w, self.ip, W, H, 0.3, FAR)  # 2 W H records
        self.srays = np.zeros(N, tthip.SHADOW_DTYPE)
        self.vis = np.zeros((N, 4), np.float32)
        self.info = np.zeros((N, 4), np.uint32)
        self.count_dev = torch.full((4,), N, dtype=torch.int32, device="cuda:0")
        self.hits_dev = torch.zeros((N + 1, 4), dtype=torch.int32, device="cuda:0")
        self.count_host = np.full(4, N, np.uint32)
        # a 16-byte aligned host block and the address 4 bytes into it
        raw = np.zeros(N * 2 * tthip.RAY_DTYPE.itemsize + 64, np.uint8)
        base = (raw.ctypes.data + 15) & ~15
        self._raw = raw
        self.misaligned = base + 4

    def close(self):
        for e in (self.bor, self.eng, self.ter, self.bare):
            e.close()


@pytest.fixture(scope="module")
def X():
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    x = Ctx()
    yield x
    x.close()


def tp(n=N, bounce=0, far=FAR, w=W, h=H, flags=0):
    return tthip.TraceParams(n_rays=n, bounce=bounce, far_plane=far, screen_width=w, screen_height=h, flags=flags)


def sp(n=N, bounce=0, w=W, h=H, flags=0):
    return tthip.ShadowParams(n_rays=n, bounce=bounce, screen_width=w, screen_height=h, flags=flags)


def expect(e, st, status, text):
    assert st == status, (st, e.L.tt_last_error(e.h).decode())
    assert e.L.tt_last_error(e.h).decode() == text


P = tthip._ptr


# ------------------------------------------------------------------ closest hit
def test_trace_closest_refusals(X):
    L, e, r = X.L, X.eng, P(X.rays)
    s = tthip.Stats()
    call = lambda eng, p, rays=r, info=None, colors=None: L.tt_trace_closest(eng.h, C.byref(p) if p else None, rays, info, colors, C.byref(s))
    assert L.tt_trace_closest(None, C.byref(tp()), r, None, None, None) == BAD
    expect(X.bare, call(X.bare, tp()), NO_SCENE, T_NO_SCENE)
    expect(e, call(e, None), BAD, T_NULL)
    expect(e, call(e, tp(), rays=None), BAD, T_NULL)
    expect(e, call(e, tp(w=0)), BAD, T_SCREEN0)
    expect(e, call(e, tp(h=0)), BAD, T_SCREEN0)
    expect(e, call(e, tp(bounce=-1)), BAD, T_BOUNCE)
    expect(e, call(e, tp(far=float("nan"))), BAD, T_NAN)
    expect(e, call(e, tp(bounce=2), info=P(X.info)), BAD, "GlobalColors required for _PrimaryTriangleInfo at bounce > 0")
    expect(e, call(e, tp(w=65536, h=32768)), BAD, "screen too large")
    expect(e, call(e, tp(n=0xFFFFFFFF, bounce=1)), BAD, "ray range overflows")
    expect(e, call(e, tp(flags=DEV)), BAD, T_HOST_RAYS)
    expect(e, call(e, tp(n=1), rays=X.misaligned), BAD, T_ALIGN)
    expect(e, call(e, tp(n=1), info=X.misaligned), BAD, T_ALIGN)
    # zero rays: TT_OK before the alignment check, stats zeroed
    s.rays = 7
    assert call(e, tp(n=0), rays=X.misaligned) == tthip.TT_OK and s.rays == 0
    # two at once: the order of the checks
    expect(e, call(e, tp(w=0), rays=None), BAD, T_NULL)
    expect(e, call(e, tp(bounce=-1, w=65536, h=32768)), BAD, T_BOUNCE)
    expect(X.bor, call(X.bor, tp(far=float("nan"))), BAD, T_NAN)  # a borrower refuses the same way


def test_trace_closest_indirect_refusals(X):
    L, e, r, cnt = X.L, X.eng, P(X.rays), P(X.count_dev)
    call = lambda p, n=cnt, rays=r: L.tt_trace_closest_indirect(e.h, C.byref(p), n, rays, None, None)
    assert L.tt_trace_closest_indirect(None, C.byref(tp()), cnt, r, None, None) == BAD
    expect(e, call(tp(flags=DEV), n=None), BAD, "null device ray count")
    expect(e, call(tp()), BAD, T_CNT_DEV)
    expect(e, call(tp(flags=STATS)), BAD, T_CNT_DEV)  # (stats + a count without DEVICE_PTRS: the pointer flag first)
    expect(e, call(tp(flags=DEV | STATS)), BAD, T_CNT_STATS)
    expect(e, call(tp(flags=DEV), n=P(X.count_host)), BAD, T_CNT_MEM)
    expect(e, call(tp(flags=DEV)), BAD, T_HOST_RAYS)
    expect(e, call(tp(flags=DEV, h=0)), BAD, T_SCREEN0)


def test_trace_closest_hits_refusals(X):
    L, e, r = X.L, X.eng, P(X.rays)
    hits = X.hits_dev
    call = lambda p, h: L.tt_trace_closest_hits(e.h, C.byref(p), r, None, None, h)
    assert L.tt_trace_closest_hits(None, C.byref(tp()), r, None, None, hits.data_ptr()) == BAD
    expect(e, call(tp(flags=DEV), None), BAD, "null hits_out")
    expect(e, call(tp(), hits.data_ptr()), BAD, "a hit-record stream needs TT_TRACE_DEVICE_PTRS")
    expect(e, call(tp(flags=DEV), P(X.info)), BAD, "hits_out is not device memory")
    expect(e, call(tp(flags=DEV), hits.data_ptr() + 4), BAD, "hits_out must be 16-byte aligned")
    expect(e, call(tp(flags=DEV, w=1 << 14, h=1 << 14, n=(1 << 27) + 1), hits.data_ptr()), BAD,
           "a hit-record stream holds at most 2^27 rays per call")
    expect(e, call(tp(flags=DEV), hits.data_ptr()), BAD, T_HOST_RAYS)


# ------------------------------------------------------------------ any hit
def test_trace_shadow_refusals(X):
    L, e, r, v = X.L, X.eng, P(X.srays), P(X.vis)
    s = tthip.Stats()
    forms = [lambda eng, p, rays=r, vis=v, nee=None: L.tt_trace_shadow(eng.h, C.byref(p) if p else None, rays, vis, None, nee, C.byref(s)),
             lambda eng, p, rays=r, vis=v, nee=None: L.tt_trace_shadow_ex(eng.h, C.byref(p) if p else None, rays, vis, None, nee, None, C.byref(s))]
    assert L.tt_trace_shadow(None, C.byref(sp()), r, v, None, None, None) == BAD
    assert L.tt_trace_shadow_ex(None, C.byref(sp()), r, v, None, None, None, None) == BAD
    for call in forms:
        expect(X.bare, call(X.bare, sp()), NO_SCENE, T_NO_SCENE)
        expect(e, call(e, None), BAD, T_NULL_SH)
        expect(e, call(e, sp(), rays=None), BAD, T_NULL_SH)
        expect(e, call(e, sp(w=0)), BAD, T_SCREEN0)
        expect(e, call(e, sp(bounce=-3)), BAD, T_BOUNCE)
        expect(e, call(e, sp(w=65536, h=32768)), BAD, "screen too large")
        expect(e, call(e, sp(flags=DEV)), BAD, T_HOST_RAYS)
        expect(e, call(e, sp(n=1), rays=X.misaligned), BAD, T_ALIGN_SH)
        expect(e, call(e, sp(n=1), vis=X.misaligned), BAD, T_ALIGN_SH)
        expect(e, call(e, sp(n=1), nee=X.misaligned), BAD, T_ALIGN_SH)
        assert call(e, sp(n=0), rays=X.misaligned) == tthip.TT_OK
        expect(e, call(e, sp(w=0, bounce=-1), rays=None), BAD, T_NULL_SH)


def test_trace_shadow_indirect_refusals(X):
    L, e, r, cnt = X.L, X.eng, P(X.srays), P(X.count_dev)
    call = lambda p, n=cnt: L.tt_trace_shadow_ex_indirect(e.h, C.byref(p), n, r, None, None, None, None)
    assert L.tt_trace_shadow_ex_indirect(None, C.byref(sp()), cnt, r, None, None, None, None) == BAD
    expect(e, call(sp(flags=DEV), n=None), BAD, "null device ray count")
    expect(e, call(sp()), BAD, T_CNT_DEV)
    expect(e, call(sp(flags=DEV | STATS)), BAD, T_CNT_STATS)
    expect(e, call(sp(flags=DEV), n=P(X.count_host)), BAD, T_CNT_MEM)
    expect(e, call(sp(flags=DEV)), BAD, T_HOST_RAYS)


# ------------------------------------------------------------------ heightmap marches
def test_trace_heightmap_refusals(X):
    L, e, r, cnt = X.L, X.ter, P(X.rays), P(X.count_dev)
    s = tthip.Stats()
    call = lambda eng, p, rays=r, info=None: L.tt_trace_heightmap(eng.h, C.byref(p) if p else None, rays, info, C.byref(s))
    ind = lambda p, n=cnt: L.tt_trace_heightmap_indirect(e.h, C.byref(p), n, r, None)
    assert L.tt_trace_heightmap(None, C.byref(tp()), r, None, None) == BAD
    assert L.tt_trace_heightmap_indirect(None, C.byref(tp()), cnt, r, None) == BAD
    expect(X.eng, call(X.eng, tp()), NO_SCENE, T_NO_TERRAIN)  # a scene, but no terrain set
    expect(X.bare, call(X.bare, tp()), NO_SCENE, T_NO_TERRAIN)
    expect(e, call(e, None), BAD, T_NULL)
    expect(e, call(e, tp(w=0)), BAD, T_SCREEN0)
    expect(e, call(e, tp(bounce=-1)), BAD, T_BOUNCE)
    expect(e, call(e, tp(w=65536, h=32768)), BAD, "screen too large")
    expect(e, call(e, tp(n=0xFFFFFFFF, bounce=1)), BAD, "ray range overflows")
    expect(e, call(e, tp(flags=DEV)), BAD, T_HOST_RAYS)
    expect(e, call(e, tp(n=1), rays=X.misaligned), BAD, T_ALIGN)
    expect(e, call(e, tp(n=1), info=X.misaligned), BAD, T_ALIGN)
    assert call(e, tp(n=0), rays=X.misaligned) == tthip.TT_OK
    expect(e, ind(tp(flags=DEV), n=None), BAD, "null device ray count")
    expect(e, ind(tp()), BAD, T_CNT_DEV)
    expect(e, ind(tp(flags=DEV | STATS)), BAD, T_CNT_STATS)
    expect(e, ind(tp(flags=DEV), n=P(X.count_host)), BAD, T_CNT_MEM)
    expect(e, ind(tp(flags=DEV)), BAD, T_HOST_RAYS)


def test_trace_shadow_heightmap_refusals(X):
    L, e, r, v, cnt = X.L, X.ter, P(X.srays), P(X.vis), P(X.count_dev)
    call = lambda eng, p, rays=r, vis=v, nee=None: L.tt_trace_shadow_heightmap(eng.h, C.byref(p) if p else None, rays, vis, None, nee, None)
    ind = lambda p, n=cnt: L.tt_trace_shadow_heightmap_indirect(e.h, C.byref(p), n, r, None, None, None, None)
    assert L.tt_trace_shadow_heightmap(None, C.byref(sp()), r, v, None, None, None) == BAD
    assert L.tt_trace_shadow_heightmap_indirect(None, C.byref(sp()), cnt, r, None, None, None, None) == BAD
    expect(X.eng, call(X.eng, sp()), NO_SCENE, T_NO_TERRAIN)
    expect(e, call(e, None), BAD, T_NULL_SH)
    expect(e, call(e, sp(h=0)), BAD, T_SCREEN0)
    expect(e, call(e, sp(bounce=-1)), BAD, T_BOUNCE)
    expect(e, call(e, sp(flags=tthip.TT_SHADOW_VISIBILITY_CHECK)), BAD, T_VIS_CHECK)
    expect(e, call(e, sp(flags=tthip.TT_SHADOW_VISIBILITY_CHECK, w=65536, h=32768)), BAD, T_VIS_CHECK)
    expect(e, call(e, sp(w=65536, h=32768)), BAD, "screen too large")
    expect(e, call(e, sp(flags=DEV)), BAD, T_HOST_RAYS)
    expect(e, call(e, sp(n=1), rays=X.misaligned), BAD, T_ALIGN_SH)
    expect(e, call(e, sp(n=1), vis=X.misaligned), BAD, T_ALIGN_SH)
    expect(e, call(e, sp(n=1), nee=X.misaligned), BAD, T_ALIGN_SH)
    assert call(e, sp(n=0), rays=X.misaligned) == tthip.TT_OK
    expect(e, ind(sp(flags=DEV), n=None), BAD, "null device ray count")
    expect(e, ind(sp()), BAD, T_CNT_DEV)
    expect(e, ind(sp(flags=DEV), n=P(X.count_host)), BAD, T_CNT_MEM)
    expect(e, ind(sp(flags=DEV | STATS)), BAD, T_HOST_RAYS)  # (no stats form: the flag is not what refuses this call)


# ------------------------------------------------------------------ bounce enqueue
def test_enqueue_refusals(X):
    L, e, r = X.L, X.eng, P(X.rays)
    n = C.c_uint32()
    call = lambda eng, p, rays=r, out=C.byref(n): L.tt_enqueue_diffuse_bounce(eng.h, C.byref(p) if p else None, rays, 0, 3, out)
    ind = lambda p, n_in, n_out: L.tt_enqueue_diffuse_bounce_indirect(e.h, C.byref(p), n_in, r, 0, 3, n_out)
    assert L.tt_enqueue_diffuse_bounce(None, C.byref(tp()), r, 0, 3, C.byref(n)) == BAD
    assert L.tt_enqueue_diffuse_bounce_indirect(None, C.byref(tp()), None, r, 0, 3, P(X.count_dev)) == BAD
    expect(e, call(e, tp(), out=None), BAD, "null argument")
    expect(X.bare, call(X.bare, tp()), NO_SCENE, T_NO_SCENE)
    expect(e, call(e, None), BAD, "null argument")
    expect(e, call(e, tp(), rays=None), BAD, "null argument")
    expect(e, call(e, tp(w=0)), BAD, "bad ray count / screen")
    expect(e, call(e, tp(n=N + 1)), BAD, "bad ray count / screen")
    expect(e, call(e, tp(w=65536, h=32768)), BAD, "bad ray count / screen")
    expect(e, ind(tp(flags=DEV), None, None), BAD, "null device survivor count")
    expect(e, ind(tp(), None, P(X.count_dev)), BAD, "device-resident ray counts need TT_TRACE_DEVICE_PTRS")
    expect(e, ind(tp(flags=DEV), None, P(X.count_host)), BAD, "a ray count pointer is not device memory")
    expect(e, ind(tp(flags=DEV), P(X.count_host), P(X.count_dev)), BAD, "a ray count pointer is not device memory")


# ------------------------------------------------------------------ resolve, generate
def test_resolve_and_generate_refusals(X):
    L, e, r = X.L, X.eng, P(X.rays)
    out = np.zeros((N, 6), np.float32)
    assert L.tt_resolve_normals(None, C.byref(tp()), r, P(out)) == BAD
    expect(X.bare, L.tt_resolve_normals(X.bare.h, C.byref(tp()), r, P(out)), NO_SCENE, T_NO_SCENE)
    expect(e, L.tt_resolve_normals(e.h, None, r, P(out)), BAD, "null argument")
    expect(e, L.tt_resolve_normals(e.h, C.byref(tp()), None, P(out)), BAD, "null argument")
    expect(e, L.tt_resolve_normals(e.h, C.byref(tp()), r, None), BAD, "null argument")

    def cam(w=W, h=H, flags=0):
        c = tthip.Camera()
        c.cam_to_world[:] = tthip.unity_colmajor(X.c2w)
        c.cam_inv_proj[:] = tthip.unity_colmajor(X.ip)
        c.near_plane, c.far_plane, c.width, c.height, c.max_bounce, c.flags = 0.3, FAR, w, h, 1, flags
        return c

    assert L.tt_generate_primary(None, C.byref(cam()), r) == BAD
    expect(e, L.tt_generate_primary(e.h, None, r), BAD, "bad camera or rays")
    expect(e, L.tt_generate_primary(e.h, C.byref(cam()), None), BAD, "bad camera or rays")
    expect(e, L.tt_generate_primary(e.h, C.byref(cam(w=0)), r), BAD, "bad camera or rays")
    expect(e, L.tt_generate_primary(e.h, C.byref(cam(w=65536, h=32768)), r), BAD, "screen too large")
    expect(e, L.tt_generate_primary(e.h, C.byref(cam(flags=DEV)), r), BAD, T_HOST_RAYS)
    expect(e, L.tt_generate_primary(e.h, C.byref(cam(flags=DEV | ASYNC)), r), BAD, T_HOST_RAYS)


# ------------------------------------------------------------------ sharing
def test_share_refusals(X):
    L, eng, bor, ter, bare = X.L, X.eng, X.bor, X.ter, X.bare
    for share in (lambda d, s: L.tt_ctx_share_scene(d, s), lambda d, s: L.tt_ctx_share_blas(d, s, 1)):
        assert share(None, eng.h) == BAD and share(bare.h, None) == BAD
        expect(bare, share(bare.h, bare.h), BAD, "a context cannot share its own scene")
        expect(ter, share(ter.h, bare.h), NO_SCENE, "the source context has no scene")
        expect(bare, share(bare.h, bor.h), BAD, "the source context shares another context's scene")
        expect(eng, share(eng.h, ter.h), BAD, "other contexts share this context's scene")  # a lender with borrowers
        # two at once: self before the missing scene, the missing scene before the lender's borrowers
        expect(bare, share(bare.h, bare.h), BAD, "a context cannot share its own scene")
        expect(eng, share(eng.h, bare.h), NO_SCENE, "the source context has no scene")
    st = L.tt_ctx_share_blas(bare.h, eng.h, 0)
    msg = L.tt_last_error(bare.h).decode()
    assert st == BAD and msg.startswith("tt_ctx_share_blas: n_tlas_nodes 0 outside (0, ") and msg.endswith("] (the TLAS region)")
    # the refused calls changed nothing: `bor` still borrows, `bare` still has no scene
    expect(bare, L.tt_trace_closest(bare.h, C.byref(tp()), P(X.rays), None, None, None), NO_SCENE, T_NO_SCENE)
    expect(eng, L.tt_scene_upload_alpha_atlas(eng.h, P(np.zeros((4, 4), np.uint8)), 4, 4), BAD,
           "other contexts share this scene: destroy them (or re-share) first")


# ------------------------------------------------------------------ the context is still usable
@pytest.mark.parametrize("who", ["eng", "bor"])
def test_a_valid_trace_after_the_refusals_matches_the_oracle(X, who):
    e = getattr(X, who)
    rays = tthip.camera_rays_host(X.c2w, X.ip, W, H, 0.3, FAR)
    ref = rays.copy()
    e.trace(rays, N, 0, FAR, W, H)
    st, _ = O.trace(X.scene, ref, N, 0, FAR, W, H)
    assert st == 0
    assert np.array_equal(rays["hits"], ref["hits"])
    assert int((rays["hits"][:N, 1] != 0xFFFFFFFF).sum()) > 0
