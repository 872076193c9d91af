"""The leaf-TLAS form of the closest-hit kernel (tt_trace_leaf_kernel, csrc/tt_trace.hip) against the oracle and
against the generic kernel, byte for byte.

A scene whose TLAS root is one leaf holding one instance takes the leaf-TLAS kernels for launches without
stats, the material check or the adaptive order (tt_trace_last_form says which form a launch took). Every case
below runs once in this process and once in a fresh child process started with TT_LEAF_KERNEL=0 (the knob is
read once per process), which forces the generic kernels; RayData, _PrimaryTriangleInfo and the compact hit
stream must equal the oracle's and the child's bytes. Output buffers start from a sentinel fill. The scene is
a 300-triangle soup under a W2L with a rotation, a translation and a negative scale on one axis.

Run as a script (`python test_gpu_leaf_kernel.py out.npz`) it is that child: every case's GPU outputs go to
the .npz.
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

import kat_cases as K
import oracle_ctypes as O
import tthip
from parity_util import CPU_THREADS, FAR

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
GENERIC, LEAF = tthip.TT_TRACE_FORM_GENERIC, tthip.TT_TRACE_FORM_LEAF
W, H = 72, 40
WH = W * H
NEAR = 0.05

_ENGINE = None


def _engine():
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = tthip.Engine(0)
    return _ENGINE


def _l2w(shift=0.0):
    """localToWorld: rotations about y and x, a mirrored y axis (negative scale), a translation."""
    a, b = np.deg2rad(33.0), np.deg2rad(-21.0)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ np.diag([1.25, -0.8, 1.1])
    m[:3, 3] = (0.3 + shift, -0.2, 0.4)
    return m


_SCENE = None


def _scene():
    global _SCENE
    if _SCENE is None:
        _SCENE = tthip.single_object_scene(tthip.Mesh.soup(11, 300, 1.0, 0.35), _l2w())
        assert tthip.tlas_root_form(_SCENE.nodes[:1]) == tthip.TT_ROOT_ONE_INSTANCE
        assert not np.allclose(_SCENE.meshdata["W2L"][0].reshape(4, 4), np.eye(4))
    return _SCENE


def _frame(w, h, jitter=1):
    c2w, ip = tthip.unity_camera((0.4, 0.1, 3.6), (-0.03, -0.02, -1), (0, 1, 0), 50, w, h, NEAR, FAR)
    return O.generate(c2w, ip, w, h, NEAR, FAR, jitter=jitter, frames=2, max_bounce=2)


def _sentinel(rays, first, n):
    rays["hits"][first:first + n] = SENT
    return rays


def _pair(eng, sc, rays, n, bounce, w, h, info=True, colors=None, flags=0, stats=False):
    """One launch on the GPU and on the oracle from the same inputs: (got, want, form)."""
    rg, rc = rays.copy(), rays.copy()
    ig = np.full((w * h, 4), SENT, np.uint32) if info else None
    ic = np.full((w * h, 4), SENT, np.uint32) if info else None
    eng.trace(rg, n, bounce, FAR, w, h, info=ig, colors=colors, flags=flags, stats=stats)
    form = eng.last_trace_form()
    assert O.trace(sc, rc, n, bounce, FAR, w, h, info=ic, colors=colors, flags=flags, nthreads=CPU_THREADS)[0] == 0
    got, want = {"rays": rg.view(np.uint8)}, {"rays": rc.view(np.uint8)}
    if info:
        got["info"], want["info"] = ig, ic
    return got, want, form


# ------------------------------------------------------------------ cases: () -> (got, want, form, expected form)
def case_frame_72x40_info1():
    """Full frame, 8x8 tile swizzle on (72 and 40 are multiples of 8), 2,880 rays, INFO 1."""
    eng, sc = _engine(), _scene()
    eng.upload(sc)
    return (*_pair(eng, sc, _sentinel(_frame(W, H), 0, WH), WH, 0, W, H), LEAF)


def case_frame_67x41_info0():
    """Full frame without the swizzle (67 x 41), a ragged last 64-ray chunk, no _PrimaryTriangleInfo."""
    eng, sc = _engine(), _scene()
    eng.upload(sc)
    return (*_pair(eng, sc, _sentinel(_frame(67, 41), 0, 67 * 41), 67 * 41, 0, 67, 41, info=False), LEAF)


def _case_count(n):
    def run():
        eng, sc = _engine(), _scene()
        eng.upload(sc)
        rays = _frame(W, H)
        rays[:n] = rays[:WH][np.linspace(0, WH - 1, n).astype(np.int64)]  # spread over the frame: hits and misses
        return (*_pair(eng, sc, _sentinel(rays, 0, n), n, 0, W, H), LEAF)
    run.__doc__ = f"{n} rays (a partial / exact / just-over wave), INFO 1."
    return run


def _bounce_inputs(eng, sc):
    rays = _frame(W, H)
    eng.trace(rays, WH, 0, FAR, W, H)
    nb = eng.enqueue_bounce(rays, WH, 0, FAR, W, H, frames=2, max_bounce=2)
    assert 64 < nb <= WH
    colors = np.zeros(WH, tthip.COL_DTYPE)
    colors["Data"][:, 3] = np.array([-1.0, 1.0, 0.0, 2.0], np.float32)[np.arange(WH) % 4]
    return rays, nb, colors


def _case_bounce(flags):
    def run():
        eng, sc = _engine(), _scene()
        eng.upload(sc)
        rays, nb, colors = _bounce_inputs(eng, sc)
        got, want, form = _pair(eng, sc, _sentinel(rays, WH, nb), nb, 1, W, H, colors=colors, flags=flags)
        t = want["rays"].view(tthip.RAY_DTYPE)["hits"][WH:WH + nb, 2].view(np.float32)
        assert (t == np.float32(FAR)).any() and (t != np.float32(FAR)).any()  # the miss form o + d t and the hit forms
        return got, want, form, LEAF
    run.__doc__ = "Bounce 1 from the enqueue (INFO 2), GlobalColors.Data.w over -1, 1, 0, 2: the re-read world ray."
    return run


def case_edge_rays():
    """Rays that miss the root box, start inside it, and carry +-0, a denormal, an infinity (and the other
    hostile values of test_gpu_parity.degenerate_rays) in a direction component."""
    from test_gpu_parity import degenerate_rays

    eng, sc = _engine(), _scene()
    eng.upload(sc)
    n = 256
    rays = degenerate_rays(n, 21)
    d = np.array([0.6, 0.0, -0.8], np.float32)
    fixed = [((50.0, 50.0, 50.0), (0.0, 1.0, 0.0)), ((50.0, 0.0, 0.0), (1.0, 0.0, 0.0)),   # miss the root box
             ((0.3, -0.2, 0.4), d), ((0.3, -0.2, 0.4), -d),                               # start inside it
             ((0.3, -0.2, 3.0), (0.0, 0.0, -1.0)), ((0.3, -0.2, 3.0), (-0.0, 0.0, -1.0)),  # +0 / -0
             ((0.3, -0.2, 3.0), (1e-40, 0.0, -1.0)), ((0.3, -0.2, 3.0), (np.inf, 0.0, -1.0))]  # denormal / infinity
    for i, (o, dd) in enumerate(fixed):
        rays["origin"][i], rays["direction"][i] = o, dd
    return (*_pair(eng, sc, _sentinel(rays, 0, n), n, 0, n, 1), LEAF)


def _case_indirect(count):
    def run():
        import torch

        eng, sc = _engine(), _scene()
        eng.upload(sc)
        dev = torch.device("cuda:0")
        rays = _sentinel(_frame(W, H), 0, WH)
        buf = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
        info = torch.from_numpy(np.full((WH, 4), SENT, np.uint32).view(np.int32)).to(dev)
        n_dev = torch.tensor([count], dtype=torch.int32, device=dev)
        eng.trace_indirect(buf, n_dev, WH, 0, FAR, W, H, info=info)
        form = eng.last_trace_form()
        torch.cuda.synchronize()
        rc, ic = rays.copy(), np.full((WH, 4), SENT, np.uint32)
        if count:
            assert O.trace(sc, rc, count, 0, FAR, W, H, info=ic, nthreads=CPU_THREADS)[0] == 0
        got = {"rays": buf.cpu().numpy(), "info": info.cpu().numpy().view(np.uint32)}
        return got, {"rays": rc.view(np.uint8), "info": ic}, form, LEAF
    run.__doc__ = f"tt_trace_closest_indirect with a device count of {count} (capacity W*H)."
    return run


def case_compact_stream():
    """tt_trace_closest_hits on the bounce-1 list: hits_out and a non-zero ray_offset (W*H on odd bounces)."""
    import torch

    eng, sc = _engine(), _scene()
    eng.upload(sc)
    dev = torch.device("cuda:0")
    rays, nb, colors = _bounce_inputs(eng, sc)
    _sentinel(rays, WH, nb)
    buf = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
    hs = torch.from_numpy(np.full((nb, 4), SENT, np.uint32).view(np.int32)).to(dev)
    eng.trace(buf, nb, 1, FAR, W, H, device=True, hits_out=hs)
    form = eng.last_trace_form()
    torch.cuda.synchronize()
    rc = rays.copy()
    assert O.trace(sc, rc, nb, 1, FAR, W, H, nthreads=CPU_THREADS)[0] == 0
    got = {"rays": buf.cpu().numpy(), "hits_out": hs.cpu().numpy().view(np.uint32)}
    return got, {"rays": rc.view(np.uint8), "hits_out": rc["hits"][WH:WH + nb].copy()}, form, LEAF


def case_overlay_context():
    """A frame slot (tt_ctx_share_blas, tlas_base != 0) over a lender's scene traces identically."""
    sc = _scene()
    lender, slot = tthip.Engine(0), tthip.Engine(0)
    try:
        lender.upload(sc)
        slot.share_blas(lender, sc.tlas_nodes)
        return (*_pair(slot, sc, _sentinel(_frame(W, H), 0, WH), WH, 0, W, H), LEAF)
    finally:
        lender.close()


def case_update_meshdata():
    """tt_scene_update_meshdata between two launches: the second follows the new W2L (the kernel reads the
    instance's record from device memory at every launch)."""
    eng, sc = _engine(), _scene()
    eng.upload(sc)
    rays = _sentinel(_frame(W, H), 0, WH)
    g1, w1, f1 = _pair(eng, sc, rays, WH, 0, W, H)
    md = sc.meshdata.copy()
    md["W2L"][0] = tthip.unity_colmajor(np.linalg.inv(_l2w(shift=0.45)))
    eng.update_meshdata(0, md)
    sc2 = tthip.Scene(sc.nodes, sc.tris, sc.tlas, md, sc.materials, tlas_nodes=sc.tlas_nodes)
    g2, w2, f2 = _pair(eng, sc2, rays, WH, 0, W, H)
    assert f1 == f2
    assert not np.array_equal(w1["rays"], w2["rays"]), "the moved instance changes the frame"
    return ({"rays": g1["rays"], "info": g1["info"], "rays2": g2["rays"], "info2": g2["info"]},
            {"rays": w1["rays"], "info": w1["info"], "rays2": w2["rays"], "info2": w2["info"]}, f2, LEAF)


def case_drain_entry():
    """One wave's worth of rays of which 24 are long (they cross the soup) and 40 miss the root box: the queue
    is dry after the first refill, so the wave enters the cooperative drain with live rays."""
    eng, sc = _engine(), _scene()
    eng.upload(sc)
    frame = _frame(W, H)
    probe = frame.copy()
    assert O.trace(sc, probe, WH, 0, FAR, W, H, nthreads=CPU_THREADS)[0] == 0
    hitting = np.nonzero(probe["hits"][:WH, 1] != 0xFFFFFFFF)[0]
    assert len(hitting) >= 24
    rays = np.zeros(2 * 64, tthip.RAY_DTYPE)
    rays[:24] = frame[hitting[np.linspace(0, len(hitting) - 1, 24).astype(np.int64)]]
    rays["origin"][24:64] = (60.0, 60.0, 60.0)
    rays["direction"][24:64] = (0.0, 1.0, 0.0)
    rays["PixelIndex"][:64] = np.arange(64)
    got, want, form = _pair(eng, sc, _sentinel(rays, 0, 64), 64, 0, 64, 1)
    hit = want["rays"].view(tthip.RAY_DTYPE)["hits"][:64, 1] != 0xFFFFFFFF
    assert hit[:24].all() and not hit[24:].any()
    return got, want, form, LEAF


# fallbacks: each takes the generic kernel and still matches the oracle
def case_fb_two_instances():
    """A root leaf holding two instances (kat_cases.case_two_instances): TT_ROOT_ONE_LEAF, the generic kernel."""
    _, sc, rays, n, _ = K.case_two_instances()
    assert tthip.tlas_root_form(sc.nodes[:1]) == tthip.TT_ROOT_ONE_LEAF
    eng = _engine()
    eng.upload(sc)
    return (*_pair(eng, sc, _sentinel(rays, 0, n), n, 0, n, 1), GENERIC)


def case_fb_two_leaves():
    """The same two instances in two leaves of node 0."""
    _, sc, rays, n, _ = K.case_two_instances()
    nodes = sc.nodes.copy()
    import handbuilt as hb
    nodes[0] = hb.make_node((-8.0, -8.0, -8.0), (K.E6 + 3,) * 3, 0, 0,
                            [(0, "leaf", (64, 64, 56), (128, 128, 72), (0, 1)),
                             (1, "leaf", (64, 64, 56), (128, 128, 72), (1, 1))])
    sc = tthip.Scene(nodes, sc.tris, sc.tlas, sc.meshdata, sc.materials, tlas_nodes=1)
    assert tthip.tlas_root_form(sc.nodes[:1]) == tthip.TT_ROOT_GENERIC
    eng = _engine()
    eng.upload(sc)
    return (*_pair(eng, sc, _sentinel(rays, 0, n), n, 0, n, 1), GENERIC)


def case_fb_after_refit():
    """After a device tt_tlas_refit the host no longer knows node 0: the generic kernel until the next update."""
    eng, sc = _engine(), _scene()
    eng.upload(sc)
    boxes = np.ascontiguousarray(sc.meta["mesh_aabbs"], np.float32)
    eng.tlas_refit(sc.tlas_nodes, boxes)
    st, nodes = O.tlas_refit(sc, boxes)
    assert st == 0
    sc2 = tthip.Scene(nodes, sc.tris, sc.tlas, sc.meshdata, sc.materials, tlas_nodes=sc.tlas_nodes)
    return (*_pair(eng, sc2, _sentinel(_frame(W, H), 0, WH), WH, 0, W, H), GENERIC)


def case_fb_stats():
    """TT_TRACE_STATS."""
    eng, sc = _engine(), _scene()
    eng.upload(sc)
    return (*_pair(eng, sc, _sentinel(_frame(W, H), 0, WH), WH, 0, W, H, stats=True), GENERIC)


def case_fb_cutout():
    """A scene with one Cutout material needs the material check (kat_cases.case_cutout)."""
    _, sc, rays, n, _ = K.case_cutout()
    assert tthip.tlas_root_form(sc.nodes[:1]) == tthip.TT_ROOT_ONE_INSTANCE
    eng = _engine()
    eng.upload(sc)
    return (*_pair(eng, sc, _sentinel(rays, 0, n), n, 0, n, 1), GENERIC)


def case_fb_adaptive_order():
    """TT_TRACE_ADAPTIVE_ORDER."""
    eng, sc = _engine(), _scene()
    eng.upload(sc)
    return (*_pair(eng, sc, _sentinel(_frame(W, H), 0, WH), WH, 0, W, H, flags=tthip.TT_TRACE_ADAPTIVE_ORDER), GENERIC)


CASES = {
    "frame_72x40_info1": case_frame_72x40_info1,
    "frame_67x41_info0": case_frame_67x41_info0,
    **{f"count_{n}": _case_count(n) for n in (1, 63, 64, 65, 129)},
    "bounce_plain": _case_bounce(0),
    "bounce_asvgf": _case_bounce(tthip.TT_TRACE_USE_ASVGF),
    "bounce_restirgi": _case_bounce(tthip.TT_TRACE_USE_RESTIRGI),
    "edge_rays": case_edge_rays,
    **{f"indirect_{c}": _case_indirect(c) for c in (0, 1, 64, WH)},
    "compact_stream": case_compact_stream,
    "overlay_context": case_overlay_context,
    "update_meshdata": case_update_meshdata,
    "drain_entry": case_drain_entry,
    "fb_two_instances": case_fb_two_instances,
    "fb_two_leaves": case_fb_two_leaves,
    "fb_after_refit": case_fb_after_refit,
    "fb_stats": case_fb_stats,
    "fb_cutout": case_fb_cutout,
    "fb_adaptive_order": case_fb_adaptive_order,
}


def _run_all(path):
    out = {}
    for name, fn in CASES.items():
        got, _, form, _ = fn()
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
    path = str(tmp_path_factory.mktemp("leaf") / "generic.npz")
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
def test_leaf_kernel_case(generic_run, name):
    got, want, form, expected = CASES[name]()
    assert form == expected, f"{name}: took form {form}, expected {expected}"
    assert int(generic_run[f"{name}/form"]) == GENERIC, "TT_LEAF_KERNEL=0 forces the generic kernels"
    for k in want:
        g = np.ascontiguousarray(got[k]).view(np.uint8)
        assert np.array_equal(g, np.ascontiguousarray(want[k]).view(np.uint8)), f"{name}: {k} differs from the oracle"
        assert np.array_equal(g, generic_run[f"{name}/{k}"].view(np.uint8)), f"{name}: {k} differs from the generic kernel"


if __name__ == "__main__":
    _run_all(sys.argv[1])
