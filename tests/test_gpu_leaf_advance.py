"""The ready-made lane state and the reordered advance of the leaf-TLAS closest-hit kernels (tt_trace_leaf_kernel,
csrc/tt_trace_leaf.h: the pool record's ready-made state word, the ballots from the compares' lane masks, the pop after
the restart, the empty-group branch that writes nothing, the wave-uniform segment state). The chunk setup stores in words 10 and 11 of a pool record what a starting lane takes verbatim
(octant byte, imask-or-0, Reps; the root step's hit mask), a finishing lane parks its result word by word, restarts,
and the other used-up lanes pop afterwards. None of it may change a byte: every case runs in this process (the
leaf-TLAS kernels), on the oracle, in a child process with TT_LEAF_KERNEL=0 (the generic kernels, which have none of
this) and in a child with TT_CHUNKS_PER_WAVE=16 (the leaf-TLAS kernels on a sixteenth of the waves, so that every wave
runs many chunks and lanes restart all the time), and RayData with its hit records, the _PrimaryTriangleInfo texels
and the compact hit stream must be equal in all four. Records and texels start from a sentinel.

What the cases are chosen for:
  * a 64x40 frame (40 chunks) on a 2,000-triangle soup seen from where more than half the rays miss it:
    restarts, and parked records of misses;
  * a frame on a dense soup where every ray hits;
  * launches of 1, 64 and 65 rays: the last chunk partial, the slots past the last ray never read;
  * rays of which half head away from the root's box: they start with Reps 1 and both groups empty;
  * a BLAS whose root has only leaf children (imask 0): a lane starts in the triangle phase with cg.y == 0; and one
    whose root has both kinds (a hit on leaf children only must give cg.y == 0 although the root has an imask);
  * INFO 0, 1 and 2, the indirect form, with and without the compact stream.
A last child runs the library built with TT_TEST_PARK_SWAP (u and v swapped in the parked words), on few waves so
that lanes are sure to restart, and must differ from the oracle: the new parking stores are what the records come from.

Run as a script (`python test_gpu_leaf_advance.py out.npz [case ...]`) it is such a child.
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

import oracle_ctypes as O
import tthip
from parity_util import CPU_THREADS, FAR

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
GENERIC, LEAF = tthip.TT_TRACE_FORM_GENERIC, tthip.TT_TRACE_FORM_LEAF
NEAR = 0.05
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
    a, b = np.deg2rad(-27.0), np.deg2rad(14.0)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ np.diag([0.9, 1.2, -1.1])
    m[:3, 3] = (-0.2, 0.1, 0.3)
    return m


def _root_imask(sc):
    """The imask of the one instance's BLAS root: which of its children are inner nodes."""
    return int(sc.nodes[int(sc.meshdata[0]["mesh_data_bvh_offsets"])]["e_imask"]) >> 24


def _scene(name):
    if ("scene", name) not in _CACHE:
        if name == "soup":  # ~2,000 small triangles: most of the box is empty
            sc = tthip.single_object_scene(tthip.Mesh.soup(21, 2000, 1.0, 0.12), _l2w())
            assert _root_imask(sc) == 0xFF
        elif name == "dense":  # as many large ones: no ray through the middle of the box gets past them
            sc = tthip.single_object_scene(tthip.Mesh.soup(22, 2000, 1.0, 0.6), _l2w())
        elif name == "leafroot":  # six triangles: the root's children are all leaves
            sc = tthip.single_object_scene(tthip.Mesh.soup(3, 6, 1.0, 0.5))
            assert _root_imask(sc) == 0
        else:  # twenty: the root has inner and leaf children
            sc = tthip.single_object_scene(tthip.Mesh.soup(3, 20, 1.0, 0.5))
            root = sc.nodes[int(sc.meshdata[0]["mesh_data_bvh_offsets"])]
            meta = np.concatenate([root["meta"][:1].view(np.uint8), root["meta"][1:].view(np.uint8)])
            assert _root_imask(sc) not in (0, 0xFF) and ((meta >> 5) != 0).sum() > bin(_root_imask(sc)).count("1")
        assert tthip.tlas_root_form(sc.nodes[:1]) == tthip.TT_ROOT_ONE_INSTANCE
        _CACHE["scene", name] = sc
    return _CACHE["scene", name]


def _frame(name, w, h):
    """A jittered primary frame: the soup from where it fills about a third of the screen, the dense soup from
    close by through a narrow lens."""
    if ("frame", name, w, h) not in _CACHE:
        if name == "soup":
            c2w, ip = tthip.unity_camera((-0.2, 0.1, 3.6), (0.02, -0.01, -1), (0, 1, 0), 55, w, h, NEAR, FAR)
        else:
            c2w, ip = tthip.unity_camera((-0.2, 0.1, 3.0), (0.0, 0.0, -1), (0, 1, 0), 12, w, h, NEAR, FAR)
        _CACHE["frame", name, w, h] = O.generate(c2w, ip, w, h, NEAR, FAR, jitter=1, frames=2, max_bounce=2)
    return _CACHE["frame", name, w, h].copy()


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _ray_list(name, n, seed, flip=0.0):
    """n rays from an eye in front of the scene's box into it; a share `flip` of them reversed (away from the box)."""
    rng = np.random.default_rng(seed)
    o = np.tile(np.array([-0.2, 0.1, 3.4]), (n, 1)) + rng.uniform(-0.05, 0.05, (n, 3))
    d = _unit(rng.uniform([-0.35, -0.35, -1.0], [0.35, 0.35, -1.0], (n, 3)))
    d[rng.random(n) < flip] *= -1.0
    rays = np.zeros(n, tthip.RAY_DTYPE)
    rays["origin"], rays["direction"] = o, d
    rays["PixelIndex"] = np.arange(n)
    return rays


def _colors(wh, bounce):
    colors = np.zeros(wh, tthip.COL_DTYPE)
    colors["Data"][:, 3] = np.array([-1.0, float(bounce), 0.0, 2.0], np.float32)[np.arange(wh) % 4]
    return colors


def _launch(sc, src, n, w, h, info, stream=False, indirect=None):
    """One launch of the first n rays of src on the GPU and (in the test process) on the oracle: (got, want, form).
    info: 0 none, 1 the bounce-0 form, 2 the bounce-1 form (the rays at offset w * h, GlobalColors Data.w over -1,
    the bounce index, 0 and 2). stream: with the compact hit stream. indirect: the device count (capacity n)."""
    wh = w * h
    bounce = 1 if info == 2 else 0
    first = wh if bounce else 0
    rays = np.zeros(2 * max(wh, n), tthip.RAY_DTYPE)
    rays[first:first + n] = src[:n]
    rays["hits"][first:first + n] = SENT
    colors = _colors(wh, bounce) if info == 2 else None
    count = n if indirect is None else indirect
    eng = _engine()
    eng.upload(sc)
    rg, rc = rays.copy(), rays.copy()
    ig = np.full((wh, 4), SENT, np.uint32) if info else None
    ic = np.full((wh, 4), SENT, np.uint32) if info else None
    got = {}
    if stream or indirect is not None:
        import torch

        dev = torch.device("cuda:0")
        buf = torch.from_numpy(rg.view(np.uint8)).to(dev)
        it = torch.from_numpy(ig.view(np.int32)).to(dev) if info else None
        ct = torch.from_numpy(colors.view(np.uint8)).to(dev) if colors is not None else None
        if indirect is not None:
            n_dev = torch.tensor([indirect], dtype=torch.int32, device=dev)
            eng.trace_indirect(buf, n_dev, n, bounce, FAR, w, h, info=it, colors=ct)
        else:
            hs = torch.from_numpy(np.full((n, 4), SENT, np.uint32).view(np.int32)).to(dev)
            eng.trace(buf, n, bounce, FAR, w, h, info=it, colors=ct, device=True, hits_out=hs)
        form = eng.last_trace_form()
        torch.cuda.synchronize()
        got["rays"] = buf.cpu().numpy()
        if indirect is None:
            got["hits_out"] = hs.cpu().numpy().view(np.uint32)
        if info:
            got["info"] = it.cpu().numpy().view(np.uint32)
    else:
        eng.trace(rg, n, bounce, FAR, w, h, info=ig, colors=colors)
        form = eng.last_trace_form()
        got["rays"] = rg.view(np.uint8)
        if info:
            got["info"] = ig
    want = None
    if WITH_ORACLE:
        if count:
            assert O.trace(sc, rc, count, bounce, FAR, w, h, info=ic, colors=colors, nthreads=CPU_THREADS)[0] == 0
        want = {"rays": rc.view(np.uint8)}
        if info:
            want["info"] = ic
        if stream and indirect is None:
            want["hits_out"] = rc["hits"][first:first + n].copy()
    return got, want, form


def _hits(want, first, n):
    return want["rays"].view(tthip.RAY_DTYPE)["hits"][first:first + n, 1] != 0xFFFFFFFF


# ------------------------------------------------------------------ cases: () -> (got, want, form)
def _case_frame(name, w, h, info, stream):
    def run():
        got, want, form = _launch(_scene(name), _frame(name, w, h), w * h, w, h, info, stream=stream)
        if want is not None:
            hit = _hits(want, w * h if info == 2 else 0, w * h)
            if name == "soup":
                assert hit.any() and hit.mean() <= 0.5, "at least half the rays must miss the mesh"
            else:
                assert hit.all(), "every ray must hit"
        return got, want, form
    run.__doc__ = f"The {w}x{h} frame on the {name} scene, INFO {info}{', compact stream' if stream else ''}."
    return run


def _case_count(n, info, stream):
    w, h = 13, 5  # 65 texels; 13 is no multiple of 8: no tile swizzle

    def run():
        return _launch(_scene("soup"), _frame("soup", 64, 40)[1000:], n, w, h, info, stream=stream)
    run.__doc__ = f"A launch of {n} rays of the soup frame, INFO {info}{', compact stream' if stream else ''}."
    return run


def _case_list(name, n, flip, info, stream=False, indirect=None):
    w, h = 21, 10  # 210 texels

    def run():
        got, want, form = _launch(_scene(name), _ray_list(name, n, 31, flip), n, w, h, info, stream=stream,
                                  indirect=indirect)
        if want is not None and indirect is None:
            hit = _hits(want, w * h if info == 2 else 0, n)
            assert hit.any() and not hit.all()
        return got, want, form
    run.__doc__ = (f"{n} rays into the {name} scene, {int(flip * 100)} % of them heading away from the root's box, INFO "
                   f"{info}" + (f", device count {indirect}" if indirect is not None else ""))
    return run


CASES = {
    **{f"frame_soup_info{i}{'_stream' if s else ''}": _case_frame("soup", 64, 40, i, s)
       for i, s in ((0, False), (1, False), (2, False), (0, True), (1, True), (2, True))},
    **{f"frame_dense_info{i}": _case_frame("dense", 24, 16, i, False) for i in (0, 1, 2)},
    **{f"count{n}_info{i}{'_stream' if s else ''}": _case_count(n, i, s)
       for n in (1, 64, 65) for i, s in ((0, False), (1, False), (2, True))},
    **{f"rootmiss_info{i}": _case_list("soup", 200, 0.5, i, stream=(i == 1)) for i in (0, 1, 2)},
    **{f"{name}_info{i}": _case_list(name, 130, 0.25, i) for name in ("leafroot", "mixedroot") for i in (0, 1, 2)},
    **{f"indirect_{c}_info{i}": _case_list("soup", 200, 0.5, i, indirect=c) for c, i in ((0, 1), (1, 1), (65, 2), (200, 1))},
}
CONTROL = "frame_dense_info1"  # the case the TT_TEST_PARK_SWAP child runs: every ray hits, u != v


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
    tmp = tmp_path_factory.mktemp("leaf_advance")
    yield {"generic": _child(tmp, "generic", {"TT_LEAF_KERNEL": "0"}),
           "dense": _child(tmp, "dense", {"TT_CHUNKS_PER_WAVE": "16"})}
    global _ENGINE
    if _ENGINE is not None:
        _ENGINE.close()
        _ENGINE = None


@pytest.mark.parametrize("name", list(CASES))
def test_leaf_advance_case(children, name):
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
    """The control: the library built with TT_TEST_PARK_SWAP parks u and v swapped, through the same stores. On
    the one wave that runs all six chunks of the case its records must differ from the oracle's, in the uv word only."""
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
    assert np.array_equal(got["hits"][:, :3], ref["hits"][:, :3])  # mesh, triangle and t are parked where they belong
    assert not np.array_equal(run[f"{CONTROL}/info"], want["info"])  # (the INFO 1 texel carries u and v too)


if __name__ == "__main__":
    _run(sys.argv[1], sys.argv[2:] or list(CASES))
