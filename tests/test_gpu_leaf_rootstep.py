"""The BLAS root's node step of the leaf-TLAS closest-hit kernels (tt_trace_leaf_kernel,
csrc/tt_trace_leaf.h): the chunk setup steps the instance's BLAS root for all 64 rays at once, from wave-uniform loads
of the node, and the prepared-ray pool carries the step's hit mask, so a refilled lane starts after it -- with inner
children to visit, with leaf triangles pending, or with an empty group.

Every case runs in this process (the leaf-TLAS kernels; tt_trace_last_form is checked) and in a fresh child process
started with TT_LEAF_KERNEL=0 (the generic kernels, which step the BLAS root in the loop). Every output byte --
RayData with its hit records, both _PrimaryTriangleInfo forms, the compact hit stream -- must equal the oracle's and
the child's. Every record starts from a sentinel.

The scenes are one instance (rotated, mirrored, translated) of a mesh of 1, 3, 8 or 40 triangles: up to 8 the BLAS
root has only leaf children, so a lane starts in the triangle phase; the 40-triangle root mixes inner children and
a leaf. The 200 rays of a mesh are of three kinds (the oracle's counts say which, _kinds): they miss the TLAS root's
box, hit it but no child of the BLAS root, or hit a child; a quarter run along an axis with +0 / -0 in the other
components, a quarter are test_gpu_parity.degenerate_rays (zero, denormal, infinite and NaN components), so inf / NaN
slabs go through the setup's step. Ray counts 1, 63, 64, 65, 129 and 200; a swizzled 24x16 frame; device counts 0, 1,
65 and the capacity; INFO 0, 1 and 2 at bounce 0 and 1 with Data.w over -1, the bounce index, 0 and 2 and the
TT_TRACE_USE_ASVGF / USE_RESTIRGI flags; a hits_out stream; a 320x200 frame on a context held to one block per CU
(several chunks per wave: pool slots left from the previous chunk); kat_cases.case_reps_exhausted and
case_chain_within_bound (the Reps bound ends the same ray at the same step); and tt_scene_update_nodes rewriting the
BLAS root between two launches on one context.

Run as a script (`python test_gpu_leaf_rootstep.py out.npz`) it is that child: every case's GPU outputs go to the .npz.
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
NEAR = 0.05
MESHES = (1, 3, 8, 40)
COUNTS = (1, 63, 64, 65, 129, 200)
N = 200
W, H = 25, 8          # N pixels, no 8x8 tile swizzle
FW, FH = 24, 16       # six 8x8 tiles: the swizzled full frame
EYE = np.array([0.4, 0.1, 3.6])

_ENGINE = None
_CACHE = {}


def _engine():
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = tthip.Engine(0)
    return _ENGINE


def _l2w():
    """localToWorld: rotations about y and x, a mirrored y axis (negative scale), a translation."""
    a, b = np.deg2rad(33.0), np.deg2rad(-21.0)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ np.diag([1.25, -0.8, 1.1])
    m[:3, 3] = (0.3, -0.2, 0.4)
    return m


def _blas_root(sc):
    return int(sc.meshdata["mesh_data_bvh_offsets"][0]) & 0x7FFFFFFF


def _root_children(sc):
    """(inner, leaf) child counts of the instance's BLAS root, from its meta bytes."""
    meta = np.ascontiguousarray(sc.nodes[_blas_root(sc)]["meta"]).view(np.uint8)
    inner = ((meta & (meta << 1) & 0x10) != 0) & ((meta >> 5) != 0)
    return int(inner.sum()), int((((meta >> 5) != 0) & ~inner).sum())


def _scene(nt):
    if ("scene", nt) not in _CACHE:
        sc = tthip.single_object_scene(tthip.Mesh.soup(11, nt, 1.0, 0.35), _l2w())
        assert tthip.tlas_root_form(sc.nodes[:1]) == tthip.TT_ROOT_ONE_INSTANCE
        inner, leaf = _root_children(sc)
        assert leaf >= 1 and (inner == 0 if nt <= 8 else inner >= 1), (nt, inner, leaf)
        _CACHE["scene", nt] = sc
    return _CACHE["scene", nt]


def _world_tris(sc):
    """World-space vertices of the scene's triangles, (n, 3, 3)."""
    m = _l2w()
    p0 = sc.tris["pos0"].astype(np.float64)
    v = np.stack([p0, p0 + sc.tris["posedge1"], p0 + sc.tris["posedge2"]], axis=1)
    return v @ m[:3, :3].T + m[:3, 3]


def _rays(nt):
    """The mesh's N rays, PixelIndex = ray index. By i % 4: 0 from the eye at a triangle's centroid; 1 along an
    axis through a centroid, +0 / -0 in the other two components; 2 degenerate_rays; 3 alternately far outside the
    TLAS root's box heading away, and from the eye at a point just inside a corner of that box (the instance is
    rotated, so the BLAS root's children are not there)."""
    if ("rays", nt) not in _CACHE:
        from test_gpu_parity import degenerate_rays

        sc = _scene(nt)
        v = _world_tris(sc)
        cen = v.mean(axis=1)
        lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
        rays = degenerate_rays(N, 100 + nt)
        corner = 0
        for i in range(N):
            c = cen[(i // 4) % len(cen)]
            if i % 4 == 0:
                rays["origin"][i], rays["direction"][i] = EYE, (c - EYE) / np.linalg.norm(c - EYE)
            elif i % 4 == 1:
                axis, k = (i // 4) % 3, i // 12
                d = np.array([0.0, -0.0, 0.0, -0.0], np.float32)[[k % 4, (k + 1) % 4, (k + 2) % 4]]
                d[axis] = -1.0 if k % 2 else 1.0
                o = c.copy()
                o[axis] -= 2.0 * d[axis]
                rays["origin"][i], rays["direction"][i] = o, d
            elif i % 4 == 3 and i % 8 == 3:
                rays["origin"][i], rays["direction"][i] = (60.0, 60.0, 60.0), (0.0, 1.0, 0.0)
            elif i % 4 == 3:
                t = np.array([(corner >> a) & 1 for a in range(3)]) * 0.94 + 0.03
                p = lo + t * (hi - lo)
                corner += 1
                rays["origin"][i], rays["direction"][i] = EYE, (p - EYE) / np.linalg.norm(p - EYE)
        _CACHE["rays", nt] = rays
    return _CACHE["rays", nt].copy()


def _kinds(sc, rays, n):
    """Per ray, from the oracle's counts: 0 missed the TLAS root's box, 1 hit it but no child of the BLAS root,
    2 hit a child of the BLAS root."""
    probe = rays.copy()
    st, cnt = O.trace(sc, probe, n, 0, FAR, n, 1, counts=True)
    assert st == 0
    below = (cnt["node_visits"] > 2) | (cnt["tri_tests"] > 0)
    return np.where(cnt["blas_entries"] == 0, 0, np.where(below, 2, 1))


def _sentinel(rays, first, n):
    rays["hits"][first:first + n] = SENT
    return rays


def _as_bounce(rays, n, wh):
    """The first n rays as a bounce-1 list: at ray offset W*H."""
    out = np.zeros(2 * max(wh, n), tthip.RAY_DTYPE)
    out[wh:wh + n] = rays[:n]
    return out


def _colors(wh, bounce):
    colors = np.zeros(wh, tthip.COL_DTYPE)
    colors["Data"][:, 3] = np.array([-1.0, float(bounce), 0.0, 2.0], np.float32)[np.arange(wh) % 4]
    return colors


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


# ------------------------------------------------------------------ cases: () -> (got, want, form)
def _case_count(nt, n):
    def run():
        eng, sc = _engine(), _scene(nt)
        eng.upload(sc)
        rays = _rays(nt)
        kinds = _kinds(sc, rays, N)
        assert all((kinds == k).sum() >= 8 for k in (0, 1, 2)), np.bincount(kinds, minlength=3)
        assert kinds[0] == 2  # (the one ray of count 1 goes past the setup's step into the triangle phase)
        return _pair(eng, sc, _sentinel(rays, 0, n), n, 0, W, H)
    run.__doc__ = f"The first {n} of the {nt}-triangle mesh's rays, bounce 0, INFO 1."
    return run


def _case_info(nt, bounce, info, flags):
    def run():
        eng, sc = _engine(), _scene(nt)
        eng.upload(sc)
        rays = _rays(nt)
        if bounce:
            rays = _as_bounce(rays, N, W * H)
        colors = _colors(W * H, bounce) if info and bounce else None
        got, want, form = _pair(eng, sc, _sentinel(rays, bounce * W * H, N), N, bounce, W, H, info=info, colors=colors,
                                flags=flags)
        if info and bounce:
            written = (want["info"] != SENT).any(axis=1)
            assert written.any() and not written.all()  # Data.w gates some texels
        return got, want, form
    run.__doc__ = (f"{N} rays of the {nt}-triangle mesh at bounce {bounce}, INFO {(2 if bounce else 1) if info else 0}, "
                   f"flags {flags}; Data.w over -1, the bounce index, 0, 2.")
    return run


def _frame(w, h):
    if ("frame", w, h) not in _CACHE:
        c2w, ip = tthip.unity_camera(tuple(EYE), (-0.03, -0.02, -1), (0, 1, 0), 50, w, h, NEAR, FAR)
        _CACHE["frame", w, h] = O.generate(c2w, ip, w, h, NEAR, FAR, jitter=1, frames=2, max_bounce=2)
    return _CACHE["frame", w, h].copy()


def _case_frame(nt):
    def run():
        eng, sc = _engine(), _scene(nt)
        eng.upload(sc)
        return _pair(eng, sc, _sentinel(_frame(FW, FH), 0, FW * FH), FW * FH, 0, FW, FH)
    run.__doc__ = f"The full {FW}x{FH} frame (8x8 tile swizzle) on the {nt}-triangle mesh, INFO 1."
    return run


def _case_indirect(count):
    def run():
        import torch

        eng, sc = _engine(), _scene(40)
        eng.upload(sc)
        dev = torch.device("cuda:0")
        rays = _sentinel(_frame(FW, FH), 0, FW * FH)
        buf = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
        info = torch.from_numpy(np.full((FW * FH, 4), SENT, np.uint32).view(np.int32)).to(dev)
        n_dev = torch.tensor([count], dtype=torch.int32, device=dev)
        eng.trace_indirect(buf, n_dev, FW * FH, 0, FAR, FW, FH, info=info)
        form = eng.last_trace_form()
        torch.cuda.synchronize()
        rc, ic = rays.copy(), np.full((FW * FH, 4), SENT, np.uint32)
        if count:
            assert O.trace(sc, rc, count, 0, FAR, FW, FH, info=ic, nthreads=CPU_THREADS)[0] == 0
        got = {"rays": buf.cpu().numpy(), "info": info.cpu().numpy().view(np.uint32)}
        return got, {"rays": rc.view(np.uint8), "info": ic}, form
    run.__doc__ = f"tt_trace_closest_indirect with a device count of {count} (capacity {FW} * {FH}), 40-triangle mesh."
    return run


def case_compact_stream():
    """tt_trace_closest_hits on a bounce-1 list of the 40-triangle mesh's rays: hits_out and a non-zero ray_offset."""
    import torch

    eng, sc = _engine(), _scene(40)
    eng.upload(sc)
    dev = torch.device("cuda:0")
    rays = _sentinel(_as_bounce(_rays(40), N, W * H), W * H, N)
    buf = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
    hs = torch.from_numpy(np.full((N, 4), SENT, np.uint32).view(np.int32)).to(dev)
    eng.trace(buf, N, 1, FAR, W, H, device=True, hits_out=hs)
    form = eng.last_trace_form()
    torch.cuda.synchronize()
    rc = rays.copy()
    assert O.trace(sc, rc, N, 1, FAR, W, H, nthreads=CPU_THREADS)[0] == 0
    got = {"rays": buf.cpu().numpy(), "hits_out": hs.cpu().numpy().view(np.uint32)}
    return got, {"rays": rc.view(np.uint8), "hits_out": rc["hits"][W * H:W * H + N].copy()}, form


def _case_many_chunks(nt, bounce):
    def run():
        w, h = 320, 200  # 1,000 chunks over the 256 waves of a grid of one block per CU
        sc = _scene(nt)
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
    run.__doc__ = (f"A 320x200 frame on the {nt}-triangle mesh, bounce {bounce}, on a grid of one block per CU: several "
                   "chunks per wave, refills that read slots left from the previous chunk.")
    return run


def _case_kat(make):
    def run():
        _, sc, rays, n, expected = make()
        assert tthip.tlas_root_form(sc.nodes[:1]) == tthip.TT_ROOT_ONE_INSTANCE
        eng = _engine()
        eng.upload(sc)
        got, want, form = _pair(eng, sc, rays, n, 0, n, 1)
        assert want["rays"].view(tthip.RAY_DTYPE)["hits"][:n].tolist() == expected
        return got, want, form
    run.__doc__ = f"kat_cases.{make.__name__} through the leaf-TLAS kernel: the Reps bound at the oracle's step."
    return run


def _case_root_rewritten(nt):
    def run():
        eng, sc = _engine(), _scene(nt)
        eng.upload(sc)
        rays = _sentinel(_rays(nt), 0, N)
        g1, w1, f1 = _pair(eng, sc, rays, N, 0, W, H)
        root = _blas_root(sc)
        nodes = sc.nodes.copy()
        meta = np.ascontiguousarray(nodes[root]["meta"]).view(np.uint8).copy()
        live = np.nonzero(meta >> 5)[0]
        meta[live[::2]] = 0  # every other child of the BLAS root is gone
        nodes[root]["meta"] = meta.view(np.uint32)
        eng.update_nodes(root, nodes[root:root + 1])
        sc2 = tthip.Scene(nodes, sc.tris, sc.tlas, sc.meshdata, sc.materials, tlas_nodes=sc.tlas_nodes)
        g2, w2, f2 = _pair(eng, sc2, rays, N, 0, W, H)
        assert f1 == f2
        assert not np.array_equal(w1["rays"], w2["rays"]), "the rewritten root changes the hits"
        return ({"rays": g1["rays"], "info": g1["info"], "rays2": g2["rays"], "info2": g2["info"]},
                {"rays": w1["rays"], "info": w1["info"], "rays2": w2["rays"], "info2": w2["info"]}, f2)
    run.__doc__ = (f"tt_scene_update_nodes rewrites the {nt}-triangle mesh's BLAS root between two launches on one "
                   "context: the second launch follows the new bytes (the kernel reads the node at every launch).")
    return run


CASES = {
    **{f"mesh{nt}_count{n}": _case_count(nt, n) for nt in MESHES for n in COUNTS},
    **{f"mesh{nt}_bounce{b}_info0": _case_info(nt, b, False, 0) for nt in (3, 40) for b in (0, 1)},
    **{f"mesh{nt}_bounce1_info2_{name}": _case_info(nt, 1, True, f) for nt in (3, 40)
       for name, f in (("plain", 0), ("asvgf", tthip.TT_TRACE_USE_ASVGF), ("restirgi", tthip.TT_TRACE_USE_RESTIRGI))},
    **{f"frame_mesh{nt}": _case_frame(nt) for nt in (8, 40)},
    **{f"indirect_{c}": _case_indirect(c) for c in (0, 1, 65, FW * FH)},
    "compact_stream": case_compact_stream,
    "many_chunks_mesh8_bounce0": _case_many_chunks(8, 0),
    "many_chunks_mesh40_bounce1": _case_many_chunks(40, 1),
    "reps_exhausted": _case_kat(K.case_reps_exhausted),
    "chain_within_bound": _case_kat(K.case_chain_within_bound),
    **{f"root_rewritten_mesh{nt}": _case_root_rewritten(nt) for nt in (8, 40)},
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
    path = str(tmp_path_factory.mktemp("leaf_rootstep") / "generic.npz")
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
def test_leaf_rootstep_case(generic_run, name):
    got, want, form = CASES[name]()
    assert form == LEAF, f"{name}: took form {form}, expected the leaf-TLAS kernels"
    assert int(generic_run[f"{name}/form"]) == GENERIC, "TT_LEAF_KERNEL=0 forces the generic kernels"
    for k in want:
        g = np.ascontiguousarray(got[k]).view(np.uint8)
        assert np.array_equal(g, np.ascontiguousarray(want[k]).view(np.uint8)), f"{name}: {k} differs from the oracle"
        assert np.array_equal(g, generic_run[f"{name}/{k}"].view(np.uint8)), f"{name}: {k} differs from the generic kernel"


if __name__ == "__main__":
    _run_all(sys.argv[1])
