"""The restart of finished lanes in the leaf-TLAS closest-hit kernels (tt_trace_leaf_kernel,
csrc/tt_trace_leaf.h): a lane whose ray finishes while the wave's pool holds prepared rays takes the next one in the same
advance block, parks the finished ray's result in the pool slot it has just consumed, and the wave writes the parked
records at full width before the next chunk setup, before the cooperative drain and at its exit. Every ray's hit
record, its _PrimaryTriangleInfo texel and its entry of the compact stream must be written exactly once.

Every case runs four times: in this process (the leaf-TLAS kernels on as many waves as the launch has chunks: a
wave's first fill takes its whole chunk, so lanes restart only in waves that come back for a second chunk before
the others have started, and in the 320x200 cases, whose context is held to 256 waves), on the oracle, in a child
process with TT_LEAF_KERNEL=0 (the generic kernels) and in a child process with TT_CHUNKS_PER_WAVE=16 (the leaf-TLAS
kernels on a sixteenth of the waves: every wave runs several chunks, takes 16 rays of each at the refill, restarts
lanes on the other 48 and writes the parked records before the next setup; with 600 rays one wave runs all ten
chunks, the last one partial). Every output byte -- RayData with its hit records, both _PrimaryTriangleInfo forms,
the compact hit stream -- must be equal in all four. Records and texels start from a sentinel, so a record that was
skipped or written from a stale slot shows. (A wave cannot reach the drain or its exit with results parked: the
queue is only seen dry by a refill, which writes the parked records first and takes what the pool still holds; the
writes at those two places are a safeguard that no launch exercises.)

Scenes, one instance each: a 3,000-triangle soup; a ground grid under rays of which about half head away from the
root's box (they start with an empty group and finish in the next advance, so restarts chain); the Cornell box with
rays from inside (a dozen triangles: many lanes finish in one advance and the pool empties in the middle of one). Ray
counts 1, 63, the chunk edges 64, 65, 127, 128, 129, then 600 and 4,097. INFO 0, 1 and 2 at bounce 0 and 1 with Data.w
over -1, the bounce index, 0 and 2 and PixelIndex values past the frame; device counts 0, 1, 65 and 600; a two-frame
batched screen; swizzled full frames; a 320x200 frame on one block per CU; a ray that exhausts the Reps bound and one
that overflows the stack among rays that miss (they park nothing and write nothing). A last child runs the library
built with TT_TEST_PARK_SWAP (two parked words swapped), at TT_CHUNKS_PER_WAVE=16 so that lanes are sure to restart,
and must differ from the oracle: the comparison can fail.

Run as a script (`python test_gpu_leaf_restart.py out.npz [case ...]`) it is such a child: the GPU outputs of the
named cases (default: all) go to the .npz.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the child process: the paths tests/conftest.py sets for pytest
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(_here), "truetrace-unity-pathtracer_amd", "python"))
    sys.path.insert(0, _here)

import handbuilt as hb
import kat_cases as K
import oracle_ctypes as O
import tthip
from parity_util import CPU_THREADS, FAR

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
GENERIC, LEAF = tthip.TT_TRACE_FORM_GENERIC, tthip.TT_TRACE_FORM_LEAF
NEAR = 0.05
COUNTS = (1, 63, 64, 65, 127, 128, 129, 600, 4097)
SCENES = ("soup", "grid", "cornell")
W, H = 83, 50  # 4,150 texels for up to 4,097 rays; 83 is no multiple of 8: no tile swizzle
CHILD_TIMEOUT = 240
PARKSWAP_LIB = os.path.join(tthip.LIB_DIR, "test", "libtruetrace_hip_parkswap.so")
WITH_ORACLE = __name__ != "__main__"  # a child only produces the GPU's bytes

_ENGINE = None
_CACHE = {}


def _engine():
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = tthip.Engine(0)
    return _ENGINE


def _l2w():
    a, b = np.deg2rad(33.0), np.deg2rad(-21.0)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ np.diag([1.25, -0.8, 1.1])
    m[:3, 3] = (0.3, -0.2, 0.4)
    return m


def _scene(name):
    if ("scene", name) not in _CACHE:
        if name == "soup":
            sc = tthip.single_object_scene(tthip.Mesh.soup(11, 3000, 1.0, 0.12), _l2w())
        elif name == "grid":
            sc = tthip.single_object_scene(tthip.Mesh.ground(-2.0, 2.0, -2.0, 2.0, 24, 24))
        else:
            sc = tthip.single_object_scene(tthip.Mesh.cornell())
        assert tthip.tlas_root_form(sc.nodes[:1]) == tthip.TT_ROOT_ONE_INSTANCE
        _CACHE["scene", name] = sc
    return _CACHE["scene", name]


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rays(name, n):
    """n rays of the scene (a prefix of one seeded list of 4,097), PixelIndex = ray index."""
    if ("rays", name) not in _CACHE:
        m = COUNTS[-1]
        rng = np.random.default_rng({"soup": 5, "grid": 6, "cornell": 7}[name])
        rays = np.zeros(m, tthip.RAY_DTYPE)
        if name == "soup":  # from the eye into the soup's box, about a third past it
            o = np.tile(np.array([0.4, 0.1, 3.6]), (m, 1))
            d = _unit(rng.uniform([-0.55, -0.45, -1.0], [0.55, 0.45, -1.0], (m, 3)))
        elif name == "grid":  # from above the grid: down onto it, or (about half, at random) up and away
            o = rng.uniform([-1.9, 0.5, -1.9], [1.9, 1.5, 1.9], (m, 3))
            d = _unit(rng.uniform([-0.3, -1.0, -0.3], [0.3, -0.6, 0.3], (m, 3)))
            d[rng.random(m) < 0.5, 1] *= -1.0
        else:  # from inside the box in every direction
            o = rng.uniform(-0.2, 0.2, (m, 3))
            d = _unit(rng.normal(size=(m, 3)))
        rays["origin"], rays["direction"] = o, d
        rays["PixelIndex"] = np.arange(m)
        _CACHE["rays", name] = rays
    out = np.zeros(2 * W * H, tthip.RAY_DTYPE)
    out[:n] = _CACHE["rays", name][:n]
    return out


def _sentinel(rays, first, n):
    rays["hits"][first:first + n] = SENT
    return rays


def _as_bounce(rays, n, wh):
    """The first n rays as a bounce-1 list: at ray offset wh."""
    out = np.zeros(2 * max(wh, n), tthip.RAY_DTYPE)
    out[wh:wh + n] = rays[:n]
    return out


def _colors(wh, bounce):
    colors = np.zeros(wh, tthip.COL_DTYPE)
    colors["Data"][:, 3] = np.array([-1.0, float(bounce), 0.0, 2.0], np.float32)[np.arange(wh) % 4]
    return colors


def _hit_mask(want, first, n):
    return want["rays"].view(tthip.RAY_DTYPE)["hits"][first:first + n, 1] != 0xFFFFFFFF


def _pair(eng, sc, rays, n, bounce, w, h, info=True, colors=None, flags=0, stream=False, status=0):
    """One launch on the GPU and (in the test process) on the oracle from the same inputs: (got, want, form).
    stream: tt_trace_closest_hits on device buffers, with the compact hit stream. status: what the call returns."""
    first = w * h if bounce else 0
    rg, rc = rays.copy(), rays.copy()
    ig = np.full((w * h, 4), SENT, np.uint32) if info else None
    ic = np.full((w * h, 4), SENT, np.uint32) if info else None
    got = {}
    if stream:
        import torch

        dev = torch.device("cuda:0")
        buf = torch.from_numpy(rg.view(np.uint8)).to(dev)
        it = torch.from_numpy(ig.view(np.int32)).to(dev) if info else None
        ct = torch.from_numpy(colors.view(np.uint8)).to(dev) if colors is not None else None
        hs = torch.from_numpy(np.full((n, 4), SENT, np.uint32).view(np.int32)).to(dev)
        st = eng.trace(buf, n, bounce, FAR, w, h, info=it, colors=ct, flags=flags, device=True, hits_out=hs, check=False)[1]
        form = eng.last_trace_form()
        torch.cuda.synchronize()
        got["rays"], got["hits_out"] = buf.cpu().numpy(), hs.cpu().numpy().view(np.uint32)
        if info:
            got["info"] = it.cpu().numpy().view(np.uint32)
    else:
        st = eng.trace(rg, n, bounce, FAR, w, h, info=ig, colors=colors, flags=flags, check=False)[1]
        form = eng.last_trace_form()
        got["rays"] = rg.view(np.uint8)
        if info:
            got["info"] = ig
    assert st == status, eng.L.tt_last_error(eng.h).decode()
    want = None
    if WITH_ORACLE:
        assert O.trace(sc, rc, n, bounce, FAR, w, h, info=ic, colors=colors, flags=flags, nthreads=CPU_THREADS)[0] == status
        want = {"rays": rc.view(np.uint8)}
        if info:
            want["info"] = ic
        if stream:
            want["hits_out"] = rc["hits"][first:first + n].copy()
    return got, want, form


# ------------------------------------------------------------------ cases: () -> (got, want, form)
def _case_count(name, n):
    def run():
        eng, sc = _engine(), _scene(name)
        eng.upload(sc)
        got, want, form = _pair(eng, sc, _sentinel(_rays(name, n), 0, n), n, 0, W, H)
        if want is not None and n >= 63:
            hit = _hit_mask(want, 0, n)
            assert hit.any() and not hit.all()  # hit records and miss records
        return got, want, form
    run.__doc__ = f"The first {n} rays of the {name} scene, bounce 0, INFO 1."
    return run


def _case_info(name, n, bounce, info, flags, stream):
    def run():
        eng, sc = _engine(), _scene(name)
        eng.upload(sc)
        rays = _rays(name, n)
        # PixelIndex past the frame: no texel, and (INFO 2) no read of GlobalColors
        rays["PixelIndex"][5:n:37] = W * H + 3
        rays["PixelIndex"][11:n:53] = 0xFFFFFFF0
        if bounce:
            rays = _as_bounce(rays, n, W * H)
        colors = _colors(W * H, bounce) if info and bounce else None
        got, want, form = _pair(eng, sc, _sentinel(rays, bounce * W * H, n), n, bounce, W, H, info=info, colors=colors,
                                flags=flags, stream=stream)
        if want is not None and info:
            written = (want["info"] != SENT).any(axis=1)
            assert written.any() and not written.all()
        return got, want, form
    run.__doc__ = (f"{n} rays of the {name} scene at bounce {bounce}, INFO {(2 if bounce else 1) if info else 0}, flags "
                   f"{flags}{', with the compact stream' if stream else ''}; Data.w over -1, the bounce index, 0, 2; "
                   "PixelIndex values past the frame.")
    return run


def _frame(w, h, frames=2):
    if ("frame", w, h, frames) not in _CACHE:
        c2w, ip = tthip.unity_camera((0.4, 0.1, 3.6), (-0.03, -0.02, -1), (0, 1, 0), 50, w, h, NEAR, FAR)
        _CACHE["frame", w, h, frames] = O.generate(c2w, ip, w, h, NEAR, FAR, jitter=1, frames=frames, max_bounce=2)
    return _CACHE["frame", w, h, frames].copy()


def _case_frame(w, h, info):
    def run():
        eng, sc = _engine(), _scene("soup")
        eng.upload(sc)
        return _pair(eng, sc, _sentinel(_frame(w, h), 0, w * h), w * h, 0, w, h, info=info)
    run.__doc__ = f"The full {w}x{h} frame on the soup (8x8 tile swizzle), INFO {1 if info else 0}."
    return run


def _case_indirect(count):
    w, h = 30, 20  # capacity 600

    def run():
        import torch

        eng, sc = _engine(), _scene("cornell")
        eng.upload(sc)
        dev = torch.device("cuda:0")
        rays = np.zeros(2 * w * h, tthip.RAY_DTYPE)
        rays[:w * h] = _rays("cornell", w * h)[:w * h]
        _sentinel(rays, 0, w * h)
        buf = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
        info = torch.from_numpy(np.full((w * h, 4), SENT, np.uint32).view(np.int32)).to(dev)
        n_dev = torch.tensor([count], dtype=torch.int32, device=dev)
        eng.trace_indirect(buf, n_dev, w * h, 0, FAR, w, h, info=info)
        form = eng.last_trace_form()
        torch.cuda.synchronize()
        got = {"rays": buf.cpu().numpy(), "info": info.cpu().numpy().view(np.uint32)}
        want = None
        if WITH_ORACLE:
            rc, ic = rays.copy(), np.full((w * h, 4), SENT, np.uint32)
            if count:
                assert O.trace(sc, rc, count, 0, FAR, w, h, info=ic, nthreads=CPU_THREADS)[0] == 0
            want = {"rays": rc.view(np.uint8), "info": ic}
        return got, want, form
    run.__doc__ = f"tt_trace_closest_indirect with a device count of {count} (capacity 600), Cornell."
    return run


def case_batched_two_frames():
    """Two 24x16 frames as one 24x32 screen (tt_ctx_set_frame_pixels): the swizzled primary launch, the enqueue, and
    the bounce-1 launch (INFO 2) on the compacted list."""
    w, h, B = 24, 16, 2
    wh = w * h
    sc = _scene("soup")
    eng = tthip.Engine(0)
    try:
        eng.upload(sc)
        eng.set_frame_pixels(wh)
        rays = np.zeros(2 * B * wh, tthip.RAY_DTYPE)
        for j in range(B):
            rays[j * wh:(j + 1) * wh] = _frame(w, h, frames=3 + j)[:wh]
            rays["PixelIndex"][j * wh:(j + 1) * wh] += np.uint32(j * wh)
        g0, w0, form = _pair(eng, sc, _sentinel(rays, 0, B * wh), B * wh, 0, w, B * h)
        rb = g0["rays"].view(tthip.RAY_DTYPE).copy()
        nb = eng.enqueue_bounce(rb, B * wh, 0, FAR, w, B * h, frames=3, max_bounce=2)
        assert 64 < nb <= B * wh
        g1, w1, form1 = _pair(eng, sc, _sentinel(rb, B * wh, nb), nb, 1, w, B * h, colors=_colors(B * wh, 1))
        assert form == form1
        got = {"rays": g0["rays"], "info": g0["info"], "rays1": g1["rays"], "info1": g1["info"]}
        want = None
        if w0 is not None:
            want = {"rays": w0["rays"], "info": w0["info"], "rays1": w1["rays"], "info1": w1["info"]}
        return got, want, form
    finally:
        eng.close()


def _case_many_chunks(bounce):
    def run():
        w, h = 320, 200  # 1,000 chunks over the 256 waves of a grid of one block per CU
        sc = _scene("soup")
        old = os.environ.get("TT_BLOCKS_PER_CU")
        os.environ["TT_BLOCKS_PER_CU"] = "1"  # (read when the context is created)
        try:
            eng = tthip.Engine(0)
        finally:
            if old is None:
                del os.environ["TT_BLOCKS_PER_CU"]
            else:
                os.environ["TT_BLOCKS_PER_CU"] = old
        try:
            eng.upload(sc)
            rays = _frame(w, h)
            if bounce == 0:
                return _pair(eng, sc, _sentinel(rays, 0, w * h), w * h, 0, w, h)
            n = w * h - 37  # (a partial last chunk; the primary rays again, as a bounce-1 list)
            return _pair(eng, sc, _sentinel(_as_bounce(rays, n, w * h), w * h, n), n, 1, w, h, colors=_colors(w * h, 1))
        finally:
            eng.close()
    run.__doc__ = (f"A 320x200 frame on the soup, bounce {bounce}, on a grid of one block per CU: several chunks per "
                   "wave in this process too, parked records written before each setup.")
    return run


def _case_no_record(kind):
    def run():
        if ("kat", kind) not in _CACHE:
            _CACHE["kat", kind] = K.case_reps_exhausted()[1] if kind == "reps" else K.stack_overflow_scene(17)[0]
        sc = _CACHE["kat", kind]
        assert tthip.tlas_root_form(sc.nodes[:1]) == tthip.TT_ROOT_ONE_INSTANCE
        eng = _engine()
        eng.upload(sc)
        n = 200
        special = (0, 7, 63, 64, 130, 199)  # these go down the chain; the others miss at the root and finish at once
        o, d = [(0.25, 0.25, 1000.0)] * n, [(0.0, 0.0, 1.0)] * n
        for i in special:
            o[i], d[i] = (0.25, 0.25, 1.0), (0.0, 0.0, -1.0)
        rays = hb.rays_buffer(o, d, FAR)
        rays["PixelIndex"][:n] = np.arange(n)
        rays["hits"][:n] = [7, 8, 9, 10]
        # (the call reports the overflow; the records are what the oracle leaves)
        got, want, form = _pair(eng, sc, rays, n, 0, n, 1, stream=True,
                                status=tthip.TT_ERR_STACK_OVERFLOW if kind == "overflow" else 0)
        if want is not None:
            hits = want["rays"].view(tthip.RAY_DTYPE)["hits"][:n]
            assert all(hits[i].tolist() == [7, 8, 9, 10] for i in special), "the oracle writes nothing for these"
            assert all(hits[i].tolist() != [7, 8, 9, 10] for i in range(n) if i not in special)
        return got, want, form
    run.__doc__ = (f"Six rays that end without a record ({kind}) among 194 that miss at the root: they park nothing, "
                   "their records keep the input bytes, the compact stream carries them, the neighbours' are intact.")
    return run


CASES = {
    **{f"{s}_count{n}": _case_count(s, n) for s in SCENES for n in COUNTS},
    **{f"{s}_bounce{b}_info0": _case_info(s, 600, b, False, 0, False) for s in SCENES for b in (0, 1)},
    **{f"{s}_bounce0_info1_pix": _case_info(s, 600, 0, True, 0, False) for s in SCENES},
    **{f"{s}_bounce1_info2_{name}": _case_info(s, 600, 1, True, f, False) for s in SCENES
       for name, f in (("plain", 0), ("asvgf", tthip.TT_TRACE_USE_ASVGF), ("restirgi", tthip.TT_TRACE_USE_RESTIRGI))},
    "soup_bounce1_info2_4097": _case_info("soup", 4097, 1, True, 0, False),
    "cornell_bounce1_info2_129_stream": _case_info("cornell", 129, 1, True, 0, True),
    "grid_bounce0_info1_4097_stream": _case_info("grid", 4097, 0, True, 0, True),
    **{f"frame_{w}x{h}_info{int(i)}": _case_frame(w, h, i) for w, h in ((24, 16), (64, 40)) for i in (True, False)},
    **{f"indirect_{c}": _case_indirect(c) for c in (0, 1, 65, 600)},
    "batched_two_frames": case_batched_two_frames,
    "many_chunks_bounce0": _case_many_chunks(0),
    "many_chunks_bounce1": _case_many_chunks(1),
    "no_record_reps": _case_no_record("reps"),
    "no_record_overflow": _case_no_record("overflow"),
}
CONTROL = "cornell_count600"  # the case the TT_TEST_PARK_SWAP child runs


def _run(path, names):
    out = {}
    for name in names:
        got, _, form = CASES[name]()
        for k, v in got.items():
            out[f"{name}/{k}"] = np.ascontiguousarray(v)
        out[f"{name}/form"] = np.uint32(form)
    np.savez(path, **out)


def _child(tmp, tag, env, names=()):
    path = str(tmp / f"{tag}.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path, *names], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(path)


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """Every case's outputs from two fresh processes: the generic kernels, and the leaf-TLAS kernels on a sixteenth
    of the waves."""
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    assert os.environ.get("TT_LEAF_KERNEL", "1") != "0", "this process must run with the leaf-TLAS kernels enabled"
    tmp = tmp_path_factory.mktemp("leaf_restart")
    yield {"generic": _child(tmp, "generic", {"TT_LEAF_KERNEL": "0"}),
           "dense": _child(tmp, "dense", {"TT_CHUNKS_PER_WAVE": "16"})}
    global _ENGINE
    if _ENGINE is not None:
        _ENGINE.close()
        _ENGINE = None


@pytest.mark.parametrize("name", list(CASES))
def test_leaf_restart_case(children, name):
    got, want, form = CASES[name]()
    assert form == LEAF, f"{name}: took form {form}, expected the leaf-TLAS kernels"
    assert int(children["generic"][f"{name}/form"]) == GENERIC, "TT_LEAF_KERNEL=0 forces the generic kernels"
    assert int(children["dense"][f"{name}/form"]) == LEAF
    for k in want:
        g = np.ascontiguousarray(got[k]).view(np.uint8)
        assert np.array_equal(g, np.ascontiguousarray(want[k]).view(np.uint8)), f"{name}: {k} differs from the oracle"
        for tag, run in children.items():
            assert np.array_equal(g, run[f"{name}/{k}"].view(np.uint8)), f"{name}: {k} differs from the {tag} child"


def test_a_swapped_parked_word_shows(tmp_path):
    """The control: the library built with TT_TEST_PARK_SWAP parks u and v swapped. On one wave that runs all ten
    chunks of the case its records must differ from the oracle's, and only in the records of rays that hit (u != v)."""
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    assert os.path.exists(PARKSWAP_LIB), "build() makes lib/test/libtruetrace_hip_parkswap.so"
    run = _child(tmp_path, "parkswap", {"TT_HIP_LIB": PARKSWAP_LIB, "TT_CHUNKS_PER_WAVE": "16"}, (CONTROL,))
    assert int(run[f"{CONTROL}/form"]) == LEAF
    _, want, _ = CASES[CONTROL]()
    got = run[f"{CONTROL}/rays"].view(tthip.RAY_DTYPE)
    ref = want["rays"].view(tthip.RAY_DTYPE)
    differs = (got["hits"] != ref["hits"]).any(axis=1)
    assert differs.any(), "the swapped word went unnoticed: no record was parked, or the comparison cannot fail"
    assert (ref["hits"][differs, 1] != 0xFFFFFFFF).all()
    assert np.array_equal(got["hits"][:, :3], ref["hits"][:, :3])  # mesh, triangle and t are parked where they belong


if __name__ == "__main__":
    _run(sys.argv[1], sys.argv[2:] or list(CASES))
