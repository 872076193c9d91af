"""The prepared-ray pool of the leaf-TLAS closest-hit kernels (tt_trace_leaf_kernel, csrc/tt_trace.hip): the rays of a
dequeued 64-ray chunk are set up by the whole wave into a per-wave pool in LDS, an idle lane's refill reads its
record from there, and the LDS part of the traversal stack is TT_LEAF_LDS_STACK (6) entries deep.

Every case runs in this process (the leaf-TLAS kernels; tt_trace_last_form is checked) and in a fresh child process
started with TT_LEAF_KERNEL=0 (the generic kernels, which have no pool and a 12-entry LDS stack). Every output byte
-- RayData with its hit records, both _PrimaryTriangleInfo forms, the compact hit stream -- must equal the oracle's
and the child's. Output buffers start from a sentinel fill.

The shapes are the smallest at which the pool can go wrong: ray counts around one chunk (1, 63, 64, 65, 129) and
8 * 64 * 3 + 5 (three chunks per scheduler segment and a partial last one: stealing across segments); full frames
with the 8x8 tile swizzle (64x40) and without (60x33); rays that all miss the root's box, and alternating hit /
miss; INFO 0, 1 and 2 with Data.w gating texels; device counts 0, 1, 65 and the capacity; a hits_out stream; three
asynchronous launches back to back (the control-block ping-pong); a 320x200 frame on a context held to one block per
CU, so that every wave dequeues several chunks and hands leftover slots out beside a new chunk; and the deep-stack
chain of test_gpu_deep_stack.py, whose rays go past the leaf form's LDS depth in the scalar loop and in the drain
(chains of depth 6, 7 and 16: the last LDS entry, the first spilled one, the full stack).

Run as a script (`python test_gpu_leaf_refill.py out.npz`) it is that child: every case's GPU outputs go to the .npz.
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
SEGMENTS = 8 * 64 * 3 + 5
COUNTS = (1, 63, 64, 65, 129, SEGMENTS)
FRAMES = {"64x40": (64, 40), "60x33": (60, 33)}  # the 8x8 tile swizzle on / off

_ENGINE = None
_CACHE = {}


def _engine():
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = tthip.Engine(0)
    return _ENGINE


def _scene():
    """One instance (rotated, mirrored, translated) of a 3,000-triangle soup: the TLAS root is one leaf."""
    if "scene" not in _CACHE:
        a, b = np.deg2rad(33.0), np.deg2rad(-21.0)
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        m = np.eye(4)
        m[:3, :3] = ry @ rx @ np.diag([1.25, -0.8, 1.1])
        m[:3, 3] = (0.3, -0.2, 0.4)
        sc = tthip.single_object_scene(tthip.Mesh.soup(11, 3000, 1.0, 0.12), m)
        assert tthip.tlas_root_form(sc.nodes[:1]) == tthip.TT_ROOT_ONE_INSTANCE
        _CACHE["scene"] = sc
    return _CACHE["scene"]


def _frame(w, h):
    """The jittered primary rays of a w x h frame (the oracle's Generate), computed once per size."""
    if (w, h) not in _CACHE:
        c2w, ip = tthip.unity_camera((0.4, 0.1, 3.6), (-0.03, -0.02, -1), (0, 1, 0), 50, w, h, NEAR, FAR)
        _CACHE[(w, h)] = O.generate(c2w, ip, w, h, NEAR, FAR, jitter=1, frames=2, max_bounce=2)
    return _CACHE[(w, h)].copy()


def _sentinel(rays, first, n):
    rays["hits"][first:first + n] = SENT
    return rays


def _miss(rays, idx):
    """The rays at idx start far outside the root's box and head away from it."""
    rays["origin"][idx] = (60.0, 60.0, 60.0)
    rays["direction"][idx] = (0.0, 1.0, 0.0)


def _pair(eng, sc, rays, n, bounce, w, h, info=True, colors=None, flags=0):
    """One launch on the GPU and on the oracle from the same inputs: (got, want, form)."""
    rg, rc = rays.copy(), rays.copy()
    ig = np.full((w * h, 4), SENT, np.uint32) if info else None
    ic = np.full((w * h, 4), SENT, np.uint32) if info else None
    eng.trace(rg, n, bounce, FAR, w, h, info=ig, colors=colors, flags=flags)
    form = eng.last_trace_form()
    assert O.trace(sc, rc, n, bounce, FAR, w, h, info=ic, colors=colors, flags=flags, nthreads=CPU_THREADS)[0] == 0
    got, want = {"rays": rg.view(np.uint8)}, {"rays": rc.view(np.uint8)}
    if info:
        got["info"], want["info"] = ig, ic
    return got, want, form


def _hit_mask(want, first, n):
    return want["rays"].view(tthip.RAY_DTYPE)["hits"][first:first + n, 1] != 0xFFFFFFFF


# ------------------------------------------------------------------ cases: () -> (got, want, form)
def _case_frame(size, info):
    w, h = FRAMES[size]

    def run():
        eng, sc = _engine(), _scene()
        eng.upload(sc)
        got, want, form = _pair(eng, sc, _sentinel(_frame(w, h), 0, w * h), w * h, 0, w, h, info=info)
        hit = _hit_mask(want, 0, w * h)
        assert hit.any() and not hit.all()
        return got, want, form
    run.__doc__ = f"The full {size} frame, INFO {1 if info else 0}."
    return run


def _case_count(n, mix):
    w, h = FRAMES["64x40"]

    def run():
        eng, sc = _engine(), _scene()
        eng.upload(sc)
        rays = np.zeros(2 * max(n, w * h), tthip.RAY_DTYPE)
        rays[:n] = _frame(w, h)[:w * h][np.linspace(0, w * h - 1, n).astype(np.int64)]  # spread over the frame
        rays["PixelIndex"][:n] = np.arange(n) % (w * h)
        if mix == "miss":
            _miss(rays, np.arange(n))
        elif mix == "alt":
            _miss(rays, np.arange(0, n, 2))
        got, want, form = _pair(eng, sc, _sentinel(rays, 0, n), n, 0, w, h)
        hit = _hit_mask(want, 0, n)
        if mix == "miss":
            assert not hit.any()
        elif mix == "alt":
            assert not hit[0::2].any() and (n < 64 or hit[1::2].any())
        return got, want, form
    run.__doc__ = f"{n} rays, INFO 1; mix: {mix} (frame: spread over the frame, miss: all miss the root, alt: every other one)."
    return run


def _bounce_inputs(eng, sc, w, h):
    rays = _frame(w, h)
    eng.trace(rays, w * h, 0, FAR, w, h)
    nb = eng.enqueue_bounce(rays, w * h, 0, FAR, w, h, frames=2, max_bounce=2)
    assert 64 < nb <= w * h
    colors = np.zeros(w * h, tthip.COL_DTYPE)
    colors["Data"][:, 3] = np.array([-1.0, 1.0, 0.0, 2.0], np.float32)[np.arange(w * h) % 4]
    return rays, nb, colors


def _case_bounce(size, flags):
    w, h = FRAMES[size]

    def run():
        eng, sc = _engine(), _scene()
        eng.upload(sc)
        rays, nb, colors = _bounce_inputs(eng, sc, w, h)
        got, want, form = _pair(eng, sc, _sentinel(rays, w * h, nb), nb, 1, w, h, colors=colors, flags=flags)
        hit = _hit_mask(want, w * h, nb)
        assert hit.any() and not hit.all()  # the miss form o + d t and the hit forms
        written = (want["info"] != SENT).any(axis=1)
        assert written.any() and not written.all()  # Data.w gates some texels
        return got, want, form
    run.__doc__ = f"Bounce 1 of the {size} frame from the enqueue (INFO 2), Data.w over -1, 1, 0, 2; flags {flags}."
    return run


def _case_indirect(count):
    w, h = FRAMES["64x40"]

    def run():
        import torch

        eng, sc = _engine(), _scene()
        eng.upload(sc)
        dev = torch.device("cuda:0")
        rays = _sentinel(_frame(w, h), 0, w * h)
        buf = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
        info = torch.from_numpy(np.full((w * h, 4), SENT, np.uint32).view(np.int32)).to(dev)
        n_dev = torch.tensor([count], dtype=torch.int32, device=dev)
        eng.trace_indirect(buf, n_dev, w * h, 0, FAR, w, h, info=info)
        form = eng.last_trace_form()
        torch.cuda.synchronize()
        rc, ic = rays.copy(), np.full((w * h, 4), SENT, np.uint32)
        if count:
            assert O.trace(sc, rc, count, 0, FAR, w, h, info=ic, nthreads=CPU_THREADS)[0] == 0
        got = {"rays": buf.cpu().numpy(), "info": info.cpu().numpy().view(np.uint32)}
        return got, {"rays": rc.view(np.uint8), "info": ic}, form
    run.__doc__ = f"tt_trace_closest_indirect with a device count of {count} (capacity 64 * 40)."
    return run


def case_compact_stream():
    """tt_trace_closest_hits on the bounce-1 list: hits_out and a non-zero ray_offset."""
    import torch

    w, h = FRAMES["64x40"]
    eng, sc = _engine(), _scene()
    eng.upload(sc)
    dev = torch.device("cuda:0")
    rays, nb, _ = _bounce_inputs(eng, sc, w, h)
    _sentinel(rays, w * h, nb)
    buf = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
    hs = torch.from_numpy(np.full((nb, 4), SENT, np.uint32).view(np.int32)).to(dev)
    eng.trace(buf, nb, 1, FAR, w, h, device=True, hits_out=hs)
    form = eng.last_trace_form()
    torch.cuda.synchronize()
    rc = rays.copy()
    assert O.trace(sc, rc, nb, 1, FAR, w, h, nthreads=CPU_THREADS)[0] == 0
    got = {"rays": buf.cpu().numpy(), "hits_out": hs.cpu().numpy().view(np.uint32)}
    return got, {"rays": rc.view(np.uint8), "hits_out": rc["hits"][w * h:w * h + nb].copy()}, form


def case_three_async_launches():
    """Three asynchronous launches back to back on one context (each zeroes the next one's control block): the
    full 64x40 frame, then 129 and 65 rays of the 60x33 one."""
    import torch

    eng, sc = _engine(), _scene()
    eng.upload(sc)
    dev = torch.device("cuda:0")
    plan = [(FRAMES["64x40"], 64 * 40), (FRAMES["60x33"], 129), (FRAMES["60x33"], 65)]
    ins = [_sentinel(_frame(w, h), 0, n) for (w, h), n in plan]
    bufs = [torch.from_numpy(r.view(np.uint8).copy()).to(dev) for r in ins]
    infos = [torch.from_numpy(np.full((w * h, 4), SENT, np.uint32).view(np.int32)).to(dev) for (w, h), _ in plan]
    forms = []
    for ((w, h), n), buf, info in zip(plan, bufs, infos):
        eng.trace(buf, n, 0, FAR, w, h, info=info, device=True, asynchronous=True)
        forms.append(eng.last_trace_form())
    torch.cuda.synchronize()
    got, want = {}, {}
    for k, (((w, h), n), r) in enumerate(zip(plan, ins)):
        ic = np.full((w * h, 4), SENT, np.uint32)
        assert O.trace(sc, r, n, 0, FAR, w, h, info=ic, nthreads=CPU_THREADS)[0] == 0
        got[f"rays{k}"], got[f"info{k}"] = bufs[k].cpu().numpy(), infos[k].cpu().numpy().view(np.uint32)
        want[f"rays{k}"], want[f"info{k}"] = r.view(np.uint8), ic
    assert len(set(forms)) == 1
    return got, want, forms[0]


def _case_many_chunks(bounce):
    def run():
        w, h = 320, 200  # 1,000 chunks over the 256 waves of a grid of one block per CU
        sc = _scene()
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
            if bounce == 0:
                return _pair(eng, sc, _sentinel(_frame(w, h), 0, w * h), w * h, 0, w, h)
            rays, nb, colors = _bounce_inputs(eng, sc, w, h)
            return _pair(eng, sc, _sentinel(rays, w * h, nb), nb, 1, w, h, colors=colors)
        finally:
            eng.close()
    run.__doc__ = f"A 320x200 frame, bounce {bounce}, on a grid of one block per CU: several chunks per wave."
    return run


def _chain_rays(shape):
    """test_gpu_deep_stack.py's shapes: whole waves on the chain's ray; `away` rays miss at the root."""
    n = 96 if shape == "second_wave_of_32" else 64
    o, d = [(0.25, 0.25, 1.0)] * n, [(0.0, 0.0, -1.0)] * n
    if shape == "odd_lanes_live":  # the live rays regroup onto other lanes' stack columns in the drain
        o[0::2], d[0::2] = [(0.25, 0.25, 1000.0)] * (n // 2), [(0.0, 0.0, 1.0)] * (n // 2)
    r = hb.rays_buffer(o, d, FAR)
    r["hits"][:n] = [7, 8, 9, 10]
    return n, r


def _case_chain(depth, shape):
    def run():
        eng = _engine()
        if ("chain", depth) not in _CACHE:
            _CACHE[("chain", depth)] = K.stack_overflow_scene(depth)[0]
        sc = _CACHE[("chain", depth)]
        eng.upload(sc)
        n, rays = _chain_rays(shape)
        probe = rays.copy()
        st, cnt = O.trace(sc, probe, n, 0, FAR, n, 1, counts=True)
        assert st == 0 and int(cnt["max_stack"].max()) == depth
        got, want, form = _pair(eng, sc, rays, n, 0, n, 1)
        hit = _hit_mask(want, 0, n)
        assert hit[1::2].all() and (hit[0::2].all() if shape != "odd_lanes_live" else not hit[0::2].any())
        return got, want, form
    run.__doc__ = f"A chain that pushes {depth} stack entries (the leaf form keeps 6 in LDS), {shape}."
    return run


CASES = {
    **{f"frame_{s}_info{int(i)}": _case_frame(s, i) for s in FRAMES for i in (True, False)},
    **{f"count_{n}_{m}": _case_count(n, m) for n in COUNTS for m in ("frame", "miss", "alt")},
    **{f"bounce_{s}_{name}": _case_bounce(s, f) for s in FRAMES
       for name, f in (("plain", 0), ("asvgf", tthip.TT_TRACE_USE_ASVGF), ("restirgi", tthip.TT_TRACE_USE_RESTIRGI))},
    **{f"indirect_{c}": _case_indirect(c) for c in (0, 1, 65, 64 * 40)},
    "compact_stream": case_compact_stream,
    "three_async_launches": case_three_async_launches,
    "many_chunks_bounce0": _case_many_chunks(0),
    "many_chunks_bounce1": _case_many_chunks(1),
    **{f"chain{d}_{s}": _case_chain(d, s) for d in (6, 7, 16)
       for s in ("full_wave", "odd_lanes_live", "second_wave_of_32")},
}


def _run_all(path):
    out = {}
    for name, fn in CASES.items():
        got, _, form = fn()
        for k, v in got.items():
            out[f"{name}/{k}"] = np.ascontiguousarray(v)
        out[f"{name}/form"] = np.uint32(form)
    np.savez(path, **out)


@pytest.fixture(scope="module")
def generic_run(tmp_path_factory):
    """Every case's outputs from a fresh process with TT_LEAF_KERNEL=0 (the generic kernels)."""
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    assert os.environ.get("TT_LEAF_KERNEL", "1") != "0", "this process must run with the leaf-TLAS kernels enabled"
    path = str(tmp_path_factory.mktemp("leaf_refill") / "generic.npz")
    env = dict(os.environ, TT_LEAF_KERNEL="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    yield np.load(path)
    global _ENGINE
    if _ENGINE is not None:
        _ENGINE.close()
        _ENGINE = None


@pytest.mark.parametrize("name", list(CASES))
def test_leaf_refill_case(generic_run, name):
    got, want, form = CASES[name]()
    assert form == LEAF, f"{name}: took form {form}, expected the leaf-TLAS kernels"
    assert int(generic_run[f"{name}/form"]) == GENERIC, "TT_LEAF_KERNEL=0 forces the generic kernels"
    for k in want:
        g = np.ascontiguousarray(got[k]).view(np.uint8)
        assert np.array_equal(g, np.ascontiguousarray(want[k]).view(np.uint8)), f"{name}: {k} differs from the oracle"
        assert np.array_equal(g, generic_run[f"{name}/{k}"].view(np.uint8)), f"{name}: {k} differs from the generic kernel"


if __name__ == "__main__":
    _run_all(sys.argv[1])
