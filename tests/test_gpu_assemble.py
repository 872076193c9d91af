"""GPU-resident objects and the on-device scene assembly (tt_object_*, tt_scene_assemble_objects): context B,
assembled from one object per BLAS under the host-built TLAS side, must hold byte for byte what context A holds
after tt_scene_upload of AssetManager.build()'s arrays -- in both forms of the gather -- trace the same frame
(which equals the oracle's) and answer every later call the same way. Scene S (tests/assemble_cases.py): parents
of 1, 65 and 4,097 triangles, instance parents of 63 and 373, 3 instances. The suite builds no
TT_NODE_STRIDE=128 library, so the strided node copy of the gather is not run here.
Bad inputs are refused on the host before anything is launched."""
import dataclasses
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import assemble_cases as AC
import handbuilt as HB
import oracle_ctypes as O
import tthip
from parity_util import CPU_THREADS, FAR, same_floats

pytestmark = pytest.mark.gpu

W = H = 64
N = W * H
CAM = tthip.unity_camera((0, 2, 14), (0, -0.1, -1), (0, 1, 0), 55, W, H, 0.3, FAR)
INVALID = tthip.TT_ERR_INVALID_ARG


class Pair:
    """A: tt_scene_upload of the host build. B: one object per BLAS, assembled on the device."""

    def __init__(self, am=None, scene=None):
        if am is None:
            am, scene = AC.scene_s()
        self.am, self.s = am, scene if scene is not None else am.build()
        self.A, self.B = tthip.Engine(0), tthip.Engine(0)
        self.extra = []
        self.A.upload(self.s)
        self.objects = [self.B.create_object(b) for b in am.blases()]
        self.region = 2 * len(self.s.meshdata)
        self.B.assemble(self.objects, self.s.nodes[:self.region], self.s.tlas, self.s.meshdata, self.s.materials)

    def close(self):
        for e in self.extra + [self.A, self.B]:
            e.close()
        for o in self.objects:
            o.destroy()


@pytest.fixture
def pair():
    p = Pair()
    yield p
    p.close()


def read_all(e, s):
    return e.scene_nodes(0, len(s.nodes)), e.scene_tris(0, len(s.tris))


def assert_same_scene(p, s=None):
    s = s or p.s
    (na, ta), (nb, tb) = read_all(p.A, s), read_all(p.B, s)
    assert na.tobytes() == nb.tobytes(), "nodes differ between upload and assembly"
    assert ta.tobytes() == tb.tobytes(), "triangles differ between upload and assembly"
    return na, ta


def frame(e):
    """Generate, primary with info texels, diffuse enqueue, bounce 1, one any-hit launch."""
    c2w, ip = CAM
    rays = np.zeros(2 * N, tthip.RAY_DTYPE)
    e.generate(rays, c2w, ip, W, H, 0.3, FAR, jitter=1, frames=3, max_bounce=1)
    gen = rays.copy()
    info = np.zeros((N, 4), np.uint32)
    e.trace(rays, N, 0, FAR, W, H, info=info)
    nb = e.enqueue_bounce(rays, N, 0, FAR, W, H, frames=3, max_bounce=1)
    e.trace(rays, nb, 1, FAR, W, H)
    sr = HB.nee_rays_from_hits(rays, N, (3.0, 9.0, 4.0), seed=5, far=FAR)
    vis = np.full((len(sr), 4), 7.0, np.float32)
    e.trace_shadow(sr, len(sr), 0, W, H, visibility=vis)
    return dict(gen=gen, rays=rays, info=info, nb=nb, sr=sr, vis=vis)


def assert_same_frame(fa, fb):
    assert fa["nb"] == fb["nb"]
    for k in ("gen", "rays", "info", "sr"):
        assert np.ascontiguousarray(fa[k]).tobytes() == np.ascontiguousarray(fb[k]).tobytes(), k
    assert same_floats(fa["vis"], fb["vis"])


def oracle_frame(sc, gen):
    rays = gen.copy()
    info = np.zeros((N, 4), np.uint32)
    assert O.trace(sc, rays, N, 0, FAR, W, H, info=info, nthreads=CPU_THREADS)[0] == 0
    nb = O.enqueue_bounce(sc, rays, N, 0, FAR, W, H, frames=3, max_bounce=1)
    assert O.trace(sc, rays, nb, 1, FAR, W, H, nthreads=CPU_THREADS)[0] == 0
    sr = HB.nee_rays_from_hits(rays, N, (3.0, 9.0, 4.0), seed=5, far=FAR)
    vis = np.full((len(sr), 4), 7.0, np.float32)
    assert O.shadow(sc, sr, len(sr), 0, W, H, visibility=vis, nthreads=CPU_THREADS)[0] == 0
    return dict(gen=gen, rays=rays, info=info, nb=nb, sr=sr, vis=vis)


# ------------------------------------------------------------------ objects and layout
def test_objects_report_their_counts_and_the_layout_has_an_8_byte_aligned_start(pair):
    bl = pair.am.blases()
    assert [b.n_tris for b in bl] == list(AC.PARENT_TRIS + AC.INSTANCE_PARENT_TRIS)
    for o, b in zip(pair.objects, bl):
        i = o.info
        assert (i.n_nodes, i.n_tris, i.device, i.root) == (b.n_nodes, b.n_tris, 0, 0)
        assert i.bytes == 80 * b.n_nodes + (88 + 48) * b.n_tris
    no, to, tn, tt = tthip.scene_layout(pair.objects, pair.region)
    assert (tn, tt) == (len(pair.s.nodes), len(pair.s.tris))
    assert no.tolist() == tthip.scene_layout([(b.n_nodes, b.n_tris) for b in bl], pair.region)[0].tolist()
    # the case the gather's regrouped stores exist for: 88-byte records at an 8- but not 16-byte aligned offset
    assert any((int(t) * 88) % 16 == 8 for t in to) and any((int(t) * 88) % 16 == 0 for t in to[1:])


def test_create_refuses_a_blas_that_does_not_stand_alone(pair):
    nodes, tris = pair.am.blases()[2].arrays()
    for name, (a, t, root) in AC.bad_objects(nodes, tris).items():
        with pytest.raises(tthip.TTError) as e:
            pair.B.create_object((a, t), root)
        assert e.value.status == INVALID and "object validation failed" in str(e.value), name


# ------------------------------------------------------------------ byte identity
def test_assembled_scene_is_byte_identical_to_upload(pair):
    nodes, tris = assert_same_scene(pair)
    assert nodes.tobytes() == pair.s.nodes.tobytes() and tris.tobytes() == pair.s.tris.tobytes()
    assert pair.A.scene_bytes() == pair.B.scene_bytes()


@pytest.mark.parametrize("form", ["kernel", "memcpy"])
def test_both_forms_are_byte_identical_to_upload(pair, form):
    """Each form in a child process with TT_ASSEMBLE_FORM set, against this process's upload."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "assemble_form_child.py")
    r = subprocess.run([sys.executable, child], env=dict(os.environ, TT_ASSEMBLE_FORM=form), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1].split()
    na, ta = read_all(pair.A, pair.s)
    want = [form, hashlib.sha1(na.tobytes()).hexdigest(), hashlib.sha1(ta.tobytes()).hexdigest(),
            hashlib.sha1(_primary(pair.A)).hexdigest()]
    assert got[1:] == want


def _primary(e):
    c2w, ip = CAM
    rays = np.zeros(2 * N, tthip.RAY_DTYPE)
    e.generate(rays, c2w, ip, W, H, 0.3, FAR, jitter=1, frames=3, max_bounce=1)
    info = np.zeros((N, 4), np.uint32)
    e.trace(rays, N, 0, FAR, W, H, info=info)
    return rays.tobytes() + info.tobytes()


# ------------------------------------------------------------------ trace identity
def test_frame_is_identical_and_equals_the_oracle(pair):
    fa, fb = frame(pair.A), frame(pair.B)
    assert_same_frame(fa, fb)
    fo = oracle_frame(pair.s, fb["gen"])
    assert fo["nb"] == fb["nb"]
    assert np.array_equal(fb["rays"]["hits"][:N + fb["nb"]], fo["rays"]["hits"][:N + fo["nb"]])
    assert np.array_equal(fb["info"], fo["info"]) and same_floats(fb["vis"], fo["vis"])
    hit = fb["rays"]["hits"][:N, 1] != 0xFFFFFFFF
    assert hit.sum() > N // 20 and len(set(fb["rays"]["hits"][:N, 0][hit].tolist())) >= 4, "the frame sees the scene"


# ------------------------------------------------------------------ later calls
def _moved(s, seed=3):
    rng = np.random.default_rng(seed)
    md = s.meshdata.copy()
    boxes = np.ascontiguousarray(s.meta["mesh_aabbs"], np.float32).copy()
    for i in range(len(AC.PARENT_TRIS), len(md)):  # the instances move
        d = rng.normal(0, 0.8, 3)
        w2l = md["W2L"][i].astype(np.float64).reshape(4, 4).T
        shift = np.eye(4)
        shift[:3, 3] = -d
        md["W2L"][i] = tthip.unity_colmajor(w2l @ shift)
        boxes[i, 0:3] += d.astype(np.float32)
        boxes[i, 3:6] += d.astype(np.float32)
    return md, boxes


def test_tlas_refit_and_meshdata_update_behave_the_same(pair):
    s = pair.s
    md, boxes = _moved(s)
    for e in (pair.A, pair.B):
        e.update_meshdata(0, md)
        e.tlas_refit(s.tlas_nodes, boxes)
    ta, tb = pair.A.scene_nodes(0, s.tlas_nodes), pair.B.scene_nodes(0, s.tlas_nodes)
    assert ta.tobytes() == tb.tobytes()
    st, want = O.tlas_refit(s, boxes)
    assert st == 0 and tb.tobytes() == want[:s.tlas_nodes].tobytes()
    assert not np.array_equal(tb, s.nodes[:s.tlas_nodes]), "the refit moved the TLAS"
    assert_same_scene(pair)
    fa, fb = frame(pair.A), frame(pair.B)
    assert_same_frame(fa, fb)
    moved = dataclasses.replace(s, nodes=want, meshdata=md)
    assert np.array_equal(fb["rays"]["hits"][:N], oracle_frame(moved, fb["gen"])["rays"]["hits"][:N])
    # a record re-pointed at another object's BLAS: validated against the bookkeeping the assembly composed
    md2 = md.copy()
    for f in ("NodeOffset", "TriOffset", "mesh_data_bvh_offsets"):
        md2[f][0] = md[f][1]
    for e in (pair.A, pair.B):
        e.update_meshdata(0, md2[:1])
    assert_same_frame(frame(pair.A), frame(pair.B))
    md2["mesh_data_bvh_offsets"][0] = len(s.nodes)  # a root outside the scene: both refuse, with the same status
    status = []
    for e in (pair.A, pair.B):
        with pytest.raises(tthip.TTError) as err:
            e.update_meshdata(0, md2[:1])
        status.append(err.value.status)
    assert status == [INVALID, INVALID]


def test_update_nodes_of_the_tlas_behaves_the_same(pair):
    s = pair.s
    _, boxes = _moved(s, 8)
    st, want = O.tlas_refit(s, boxes)
    assert st == 0
    for e in (pair.A, pair.B):
        e.update_nodes(0, want[:s.tlas_nodes])
    assert_same_scene(pair)
    # a BLAS node rewritten through the host path takes the full re-validation on both
    k = int(s.meshdata["NodeOffset"][2])
    for e in (pair.A, pair.B):
        e.update_nodes(k, s.nodes[k:k + 2])
    assert_same_scene(pair)
    assert_same_frame(frame(pair.A), frame(pair.B))


def test_blas_refit_of_the_largest_parent_behaves_the_same(pair):
    from test_blas_refit import deform, vertex_buffer

    mesh, blas = AC.meshes_and_blases()[0][2], AC.meshes_and_blases()[1][2]
    pos, nrm, idx = mesh.arrays()
    V = vertex_buffer(deform(pos, 0.7), nrm)
    leaf = blas.leaf_order()
    for e in (pair.A, pair.B):
        e.blas_refit(2, V, idx, leaf)
    nodes, tris = assert_same_scene(pair)
    st, want_nodes, want_tris = O.blas_refit(pair.s, 2, V, idx, leaf)
    assert st == 0 and nodes.tobytes() == want_nodes.tobytes() and tris.tobytes() == want_tris.tobytes()
    assert tris.tobytes() != pair.s.tris.tobytes()
    assert_same_frame(frame(pair.A), frame(pair.B))
    # a re-assembly reverts the deformed mesh to its object's triangles (the reference's RefitMesh, too, writes
    # only the aggregated buffers)
    pair.B.assemble(pair.objects, pair.s.nodes[:pair.region], pair.s.tlas, pair.s.meshdata, pair.s.materials)
    nb, tb = read_all(pair.B, pair.s)
    assert nb.tobytes() == pair.s.nodes.tobytes() and tb.tobytes() == pair.s.tris.tobytes()


def test_frame_slot_over_an_assembled_scene_traces_the_frame(pair):
    sa, sb = tthip.Engine(0), tthip.Engine(0)
    pair.extra += [sa, sb]
    sa.share_blas(pair.A, pair.s.tlas_nodes)
    sb.share_blas(pair.B, pair.s.tlas_nodes)
    md, boxes = _moved(pair.s, 11)
    for e in (sa, sb):
        e.update_meshdata(0, md)
        e.tlas_refit(pair.s.tlas_nodes, boxes)
    na, nb = sa.scene_nodes(0, len(pair.s.nodes)), sb.scene_nodes(0, len(pair.s.nodes))
    assert na.tobytes() == nb.tobytes()
    fa, fb = frame(sa), frame(sb)
    assert_same_frame(fa, fb)
    assert_same_frame(frame(pair.A), frame(pair.B))  # the lenders still trace the first pose
    assert fb["rays"]["hits"].tobytes() != frame(pair.B)["rays"]["hits"].tobytes()
    # while a borrower exists, both ways of loading a scene are refused alike
    status = []
    for call in (lambda: pair.A.upload(pair.s),
                 lambda: pair.B.assemble(pair.objects, pair.s.nodes[:pair.region], pair.s.tlas, pair.s.meshdata,
                                         pair.s.materials)):
        with pytest.raises(tthip.TTError) as err:
            call()
        status.append((err.value.status, "share this scene" in str(err.value)))
    assert status == [(INVALID, True), (INVALID, True)]
    assert_same_frame(frame(pair.A), frame(pair.B))  # a refused call on a lender leaves its scene alone


def test_one_object_assembly_selects_the_leaf_tlas_kernel():
    am = tthip.AssetManager()
    am.add_parent(tthip.Blas(tthip.Mesh.cornell()), None, np.zeros(8, tthip.MAT_DTYPE))
    p = Pair(am)
    try:
        assert len(p.objects) == 1 and tthip.tlas_root_form(p.s.nodes) == tthip.TT_ROOT_ONE_INSTANCE
        assert_same_scene(p)
        c2w, ip = tthip.unity_camera((0, 0, 3.4), (0, 0, -1), (0, 1, 0), 40, W, H, 0.3, FAR)
        out = []
        for e in (p.A, p.B):
            rays = O.generate(c2w, ip, W, H, 0.3, FAR)
            info = np.zeros((N, 4), np.uint32)
            e.trace(rays, N, 0, FAR, W, H, info=info)
            out.append((rays.tobytes(), info.tobytes(), e.last_trace_form()))
        assert out[0] == out[1] and out[1][2] == tthip.TT_TRACE_FORM_LEAF
    finally:
        p.close()


# ------------------------------------------------------------------ re-assembly
def test_reassembly_with_one_object_swapped_equals_a_fresh_upload(pair):
    _, bl = AC.meshes_and_blases()
    new_blas = tthip.Blas(tthip.Mesh.soup(77, 129, 1.5, 0.35))
    am2 = AC.manager([bl[0], new_blas, bl[2]], bl[3:])  # the 65-triangle parent leaves, a 129-triangle one arrives
    s2 = am2.build()
    assert len(s2.tris) == len(pair.s.tris) + 64
    new_obj = pair.B.create_object(new_blas)
    objs = [pair.objects[0], new_obj] + pair.objects[2:]
    pair.objects.append(new_obj)
    no, to, tn, tt = tthip.scene_layout(objs, 2 * len(s2.meshdata))
    assert (tn, tt) == (len(s2.nodes), len(s2.tris)) and int(s2.meshdata["NodeOffset"][2]) == no[2]
    pair.B.assemble(objs, s2.nodes[:2 * len(s2.meshdata)], s2.tlas, s2.meshdata, s2.materials)
    pair.A.upload(s2)
    nodes, tris = assert_same_scene(pair, s2)
    assert nodes.tobytes() == s2.nodes.tobytes() and tris.tobytes() == s2.tris.tobytes()
    fa, fb = frame(pair.A), frame(pair.B)
    assert_same_frame(fa, fb)
    # the assembly copied the objects: destroy them all, trace again
    for o in pair.objects:
        o.destroy()
    assert_same_frame(fa, frame(pair.B))
    fo = oracle_frame(s2, fb["gen"])
    assert np.array_equal(fb["rays"]["hits"][:N + fb["nb"]], fo["rays"]["hits"][:N + fo["nb"]])


def test_assembly_is_refused_while_a_plain_borrower_exists(pair):
    c = tthip.Engine(0)
    pair.extra.append(c)
    c.share_scene(pair.B)
    d = tthip.Engine(0)
    pair.extra.append(d)
    d.share_scene(pair.A)
    got = []
    for call in (lambda: pair.A.upload(pair.s),
                 lambda: pair.B.assemble(pair.objects, pair.s.nodes[:pair.region], pair.s.tlas, pair.s.meshdata,
                                         pair.s.materials),
                 lambda: c.assemble(pair.objects, pair.s.nodes[:pair.region], pair.s.tlas, pair.s.meshdata,
                                    pair.s.materials),
                 lambda: d.upload(pair.s)):
        with pytest.raises(tthip.TTError) as err:
            call()
        got.append(err.value.status)
    assert got == [INVALID] * 4
    assert_same_frame(frame(c), frame(d))


# ------------------------------------------------------------------ refusals, before anything is launched
def _bad_inputs(p, name):
    s = p.s
    objs, tlas_nodes, tlas, md = list(p.objects), s.nodes[:p.region].copy(), s.tlas.copy(), s.meshdata.copy()
    if name == "mesh record matches no object":
        md["TriOffset"][0] += 1
    elif name == "root outside its object":  # the next object's first node: the whole-scene check would accept it
        md["mesh_data_bvh_offsets"][1] = md["NodeOffset"][1] + p.objects[1].info.n_nodes
    elif name == "TLASBVH8Indices entry == n_mesh":
        tlas[0] = len(md)
    elif name == "TLAS child index == tlas_region":
        k = next(k for k in range(8) if AC.meta_of(tlas_nodes, 0, k) == 0)
        AC.set_meta(tlas_nodes, 0, k, (1 << 5) | 24)  # an inner child in slot 0 ...
        tlas_nodes["e_imask"][0] |= np.uint32(1 << 24)
        tlas_nodes["base_child"][0] = p.region      # ... at the first node past the region
    elif name == "null object":
        objs[3] = None
    elif name == "n_objects == 0":
        objs = []
    else:
        raise AssertionError(name)
    return objs, tlas_nodes, tlas, md


@pytest.mark.parametrize("name", ["mesh record matches no object", "root outside its object",
                                  "TLASBVH8Indices entry == n_mesh", "TLAS child index == tlas_region", "null object",
                                  "n_objects == 0"])
def test_refusals_leave_the_context_without_a_scene(pair, name):
    objs, tlas_nodes, tlas, md = _bad_inputs(pair, name)
    pair.B.scene_nodes(0, 1)  # B holds a scene ...
    with pytest.raises(tthip.TTError) as e:
        pair.B.assemble(objs, tlas_nodes, tlas, md, pair.s.materials)
    assert e.value.status == INVALID
    assert len(str(e.value).split(":", 2)[-1].strip()) > 10, "a reason is given"
    with pytest.raises(tthip.TTError) as e:  # ... and none after the refused call, as after a refused upload
        pair.B.scene_nodes(0, 1)
    assert e.value.status == tthip.TT_ERR_NO_SCENE
    # a good assembly afterwards works again
    pair.B.assemble(pair.objects, pair.s.nodes[:pair.region], pair.s.tlas, pair.s.meshdata, pair.s.materials)
    assert_same_scene(pair)
