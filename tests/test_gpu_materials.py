"""The kernels against texture space, with nothing in between: what the material-check form of the generic
closest-hit kernel and the MATCHECK form of the any-hit kernel write for scenes with Cutout and glass materials
is compared with materials.py, the float64 model written from the reference's text, on the scenes, atlases, ray
sets, caps, coverage floors and controls of test_materials_host.py (materials_cases.py holds them). The parity
tests prove kernel == restatement bit for bit; a mistake the two share (an atlas indexed x * h + y, the rectangle's
corners the other way round, the half texel on the wrong sampler, texedge1 and texedge2 exchanged, a tint under the
wrong condition) passes them all and fails here. The restatement is not called in this file.

Beyond the host file's matrix: the affine-UV scenes built by tt_blas_build_device, and built as objects by
tt_object_build_device / tt_objects_build_device and assembled on the device under one MaterialOffset per
object, with the triangle records taken back from the device; and the same comparison after tt_blas_refit and
tt_blas_refit_many. Each of these scenes is compared under two models: one reads UVs and MatDat from the records
that came back, the other takes the surface UV of the rest mesh and MatDat from the mesh's own arrays, so nothing a
builder, the assembler or a refit wrote into those fields can pass by being read on both sides."""
import dataclasses

import numpy as np
import pytest

import bruteforce as BF
import bruteforce_cases as C
import materials as M
import materials_cases as MC
import tthip

pytestmark = pytest.mark.gpu

FAR = MC.FAR
N_SHORT = 65  # one full wave and one lane of the next
GENERIC = tthip.TT_TRACE_FORM_GENERIC


def gpu_closest(engine, rays, n, flags, bounce):
    """Traces the first n rays of a buffer on the uploaded scene; every launch of a scene with a Cutout material
    must take the generic kernel."""
    W = len(rays) // 2
    r = rays.copy()
    engine.trace(r, n, bounce, FAR, W, 1, flags=flags)
    assert engine.last_trace_form() == GENERIC
    keep = np.ones(len(r), bool)
    keep[W * bounce:W * bounce + n] = False
    assert r[keep].tobytes() == rays[keep].tobytes(), "a ray outside the launch was written"
    return r["hits"][W * bounce:W * bounce + n]


def gpu_any_hit(engine, before, W, H, bounce, visibility_check):
    after = before.copy()
    vis, col, nee = C.shadow_outputs(len(before), W * H)
    engine.trace_shadow(after, len(after), bounce, W, H, visibility=vis, colors=col, nee_pos=nee,
                        flags=tthip.TT_SHADOW_VISIBILITY_CHECK if visibility_check else 0)
    return after, vis, col, nee, None


class KernelSide(MC.Side):
    """The host-built scenes of materials_cases, uploaded when a launch asks for another one."""

    def __init__(self, engine):
        super().__init__()
        self.engine, self.uploaded = engine, None

    def _upload(self, sc):
        if self.uploaded is not sc:
            self.engine.upload(sc)
            self.uploaded = sc

    def trace(self, sc, rays, n, flags, bounce):
        self._upload(sc)
        return gpu_closest(self.engine, rays, n, flags, bounce)

    def nee_frame(self, sc, c2w, ip):
        self._upload(sc)
        frame = np.zeros(2 * C.NEE_W * C.NEE_H, tthip.RAY_DTYPE)
        self.engine.generate(frame, c2w, ip, C.NEE_W, C.NEE_H, 0.05, FAR)
        self.engine.trace(frame, C.NEE_W * C.NEE_H, 0, FAR, C.NEE_W, C.NEE_H)
        return frame

    def shadow(self, sc, before, W, H, bounce, visibility_check):
        self._upload(sc)
        return gpu_any_hit(self.engine, before, W, H, bounce, visibility_check)


@pytest.fixture(scope="module")
def atlas_engine():
    """A context of this module's own: the atlases stay with a context for good, and tests of the shared context
    rely on its having none."""
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    eng = tthip.Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def side(atlas_engine):
    return KernelSide(atlas_engine)


# ------------------------------------------------------------------ closest hit, the linear sampler
@pytest.mark.parametrize("ray_set", ["random", "axis"])
@pytest.mark.parametrize("name", MC.SCENES)
def test_closest_kernel(side, name, ray_set):
    """The four flag sets at both bounces; and a launch that ends one lane into a wave: the same rays, the same
    answers."""
    for flags in C.FLAGS:
        for bounce in (0, 1):
            MC.closest_case(side, name, "noise", ray_set, flags, bounce).check()
    ref, _ = MC.closest_reference(name, "noise", ray_set, 0, 1)
    short = gpu_closest(side.engine, MC.closest_rays(name, ray_set), N_SHORT, 0, 1)
    C.compare_closest(C.head(ref, N_SHORT), short, caps=False).check()


@pytest.mark.parametrize("atlas", MC.ATLASES[1:])
@pytest.mark.parametrize("name", MC.SCENES)
def test_closest_kernel_other_atlases(side, name, atlas):
    for flags, bounce in ((0, 1), (C.FLAGS[3], 0)):
        MC.closest_case(side, name, atlas, "random", flags, bounce).check()


@pytest.mark.parametrize("name", MC.SCENES)
def test_closest_kernel_4096_rays(side, name):
    MC.closest_case(side, name, "noise", "big", 0, 1).check()


@pytest.mark.parametrize("name", MC.AFFINE)
def test_record_uv_is_the_surface_uv(side, name):
    MC.uv_case(side, name)


# ------------------------------------------------------------------ any-hit, the point sampler and the tints
@pytest.mark.parametrize("name,ray_set", MC.SHADOW_CASES)
def test_any_hit_kernel(side, name, ray_set):
    for visibility_check in (False, True):
        for bounce in (0, 1):
            MC.any_hit_case(side, name, "noise", ray_set, bounce, visibility_check).check()


@pytest.mark.parametrize("atlas", MC.ATLASES[1:])
@pytest.mark.parametrize("name", MC.SCENES)
def test_any_hit_kernel_other_atlases(side, name, atlas):
    MC.any_hit_case(side, name, atlas, "random", 0, False).check()


@pytest.mark.parametrize("name", MC.SCENES)
def test_any_hit_kernel_4096_rays(side, name):
    MC.any_hit_case(side, name, "noise", "big", 0, False).check()


@pytest.mark.parametrize("family", list(MC.FAMILIES))
def test_coverage(side, family):
    MC.coverage_case(side, family)


# ------------------------------------------------------------------ controls: the comparison must be able to fail
@pytest.mark.parametrize("variant", MC.TEXTURE_CONTROLS)
def test_control_texture_space(side, variant):
    MC.control_texture_space(side, variant)


def test_control_tints(side):
    MC.control_tints(side)


def test_control_le_for_lt_at_exact_equality(side):
    MC.control_equality(side)


def test_numpy_edits_of_a_correct_output_are_reported(side):
    MC.control_numpy_edits(side)


# ------------------------------------------------------------------ the device builders
KEPT_FIELDS = ("tex0", "texedge1", "texedge2", "MatDat")


def mesh_matdat(name, sc, leaves, n_tris):
    """MatDat per triangle record from the parts' own per-triangle arrays through leaf_of_triangle: nothing that a
    builder, the assembler or a refit wrote into a record."""
    out = np.zeros(n_tris, np.uint32)
    for k, part in enumerate(MC.parts(name)):
        out[int(sc.meshdata["TriOffset"][k]) + np.asarray(leaves[k], np.int64)] = part.matdat
    return out


def assert_records_kept(before, after):
    """The UVs and MatDat of every record, bit for bit."""
    for f in KEPT_FIELDS:
        a, b = (np.ascontiguousarray(x[f]).view(np.uint32).reshape(len(x), -1) for x in (before, after))
        bad = np.nonzero((a != b).any(1))[0]
        assert not len(bad), f"{len(bad)} records changed their {f}, first record {int(bad[0])}"


def two_models(name, sc, tris, leaves, positions=None, rest=None):
    """(name, model) twice. "record": UVs and MatDat from the records read back from the device. "surface": the
    affine UV of the hit point (of the same barycentric point of the rest triangle where `rest` is given) and MatDat
    from the meshes through leaf_of_triangle; its copy of the records has NaN UVs, so it cannot have read them.
    positions: (p0, e1, e2) float64 replacing the records' (a deformed mesh)."""
    like = MC.with_atlases(dataclasses.replace(sc, tris=tris), "noise")
    own = tris.copy()
    own["MatDat"] = mesh_matdat(name, sc, leaves, len(tris))
    for f in KEPT_FIELDS[:3]:
        own[f] = np.nan
    indep = dataclasses.replace(like, tris=own)
    pos = () if positions is None else positions
    return (("record", M.Model(like, geometry=BF.Geometry.from_scene(like, *pos), affine=MC.affine_of(name), rest=rest)),
            ("surface", M.Model(indep, geometry=BF.Geometry.from_scene(indep, *pos), uv="surface",
                                affine=MC.affine_of(name), rest=rest)))


DEVICE_LAUNCHES = (("random", 0, 1), ("axis", C.FLAGS[3], 0), ("random", 0, 0))


def device_scene_reports(engine, name, models):
    """The closest-hit and any-hit comparisons on the scene that is on the device, under the noise atlas, once per
    model: {model name: [reports]}. Record UV against surface UV on every robust hit of the record model."""
    engine.upload_alpha_atlas(MC.alpha_atlas("noise"))
    engine.upload_texture_atlas(MC.texture_atlas())
    before, W, H = MC.shadow_rays(name, "random")
    hits = {launch: gpu_closest(engine, MC.closest_rays(name, launch[0]), len(MC.closest_rays(name, launch[0])) // 2,
                                launch[1], launch[2]) for launch in DEVICE_LAUNCHES}
    shadow = gpu_any_hit(engine, before, W, H, 0, False)
    reports = {}
    for which, mdl in models:
        reports[which] = []
        checked, worst = 0, 0.0
        for launch in DEVICE_LAUNCHES:
            rays = MC.closest_rays(name, launch[0])
            n = len(rays) // 2
            ref = mdl.closest(rays["origin"][:n], rays["direction"][:n], FAR, launch[1], launch[2])
            reports[which].append(C.compare_closest(ref, hits[launch]))
            if which == "record":
                ratio, k = MC.check_uv(mdl, ref, rays[:n])
                checked, worst = checked + k, max(worst, ratio)
        if which == "record":
            print(f"{name}: largest record-versus-surface UV ratio to db {worst:.3g} over {checked} robust hits")
            assert checked >= 300
        reports[which].append(MC.compare_any_hit(mdl, before, shadow, 0))
    return reports


def device_scene_checks(engine, name, models):
    for which, reps in device_scene_reports(engine, name, models).items():
        for rep in reps:
            print(which, end=": ")
            rep.check()


@pytest.mark.parametrize("name", MC.AFFINE)
def test_scene_of_device_built_blases(atlas_engine, side, name):
    """tt_blas_build_device for every part; the scene is assembled on the host and uploaded."""
    side.uploaded = None
    blases = [tthip.Blas(p.mesh(), engine=atlas_engine) for p in MC.parts(name)]
    sc = MC.assemble(name, blases).build()
    MC.check_order(sc, name)
    atlas_engine.upload(sc)
    tris = atlas_engine.scene_tris(0, len(sc.tris))
    device_scene_checks(atlas_engine, name, two_models(name, sc, tris, [b.leaf_order() for b in blases]))


def assembled_objects(engine, name):
    """The parts as device-built objects (the first by tt_object_build_device, the others in one
    tt_objects_build_device call), assembled on the device. Returns (scene without triangles, objects)."""
    meshes = [p.mesh() for p in MC.parts(name)]
    objects = [engine.build_object(meshes[0])] + (engine.build_objects(meshes[1:]) if len(meshes) > 1 else [])
    sc, objects = MC.assemble(name, objects, "add_parent_object").assemble_objects(engine)
    MC.check_order(sc, name)
    return sc, objects


@pytest.mark.parametrize("name", MC.AFFINE)
def test_scene_of_objects_assembled_on_the_device(atlas_engine, side, name):
    side.uploaded = None
    sc, objects = assembled_objects(atlas_engine, name)
    try:
        tris = atlas_engine.scene_tris(0, sc.meta["n_tris_total"])
        device_scene_checks(atlas_engine, name, two_models(name, sc, tris, [o.read()[2] for o in objects]))
    finally:
        for o in objects:
            o.destroy()


# ------------------------------------------------------------------ after the refits
def refit_checks(engine, name, sc, before, moved, leaves, boxes=None):
    """before: the records as they stood ahead of the refit; moved: {mesh record: deformed float32 vertices};
    leaves: leaf_of_triangle per mesh record. The refit must have kept every record's UVs and MatDat bit for bit.
    Both models see positions rebuilt in float64 from the deformed vertex arrays; the surface model takes its UV from
    the same barycentric point of the rest triangle and its MatDat from the meshes, so a refit that harmed the fields
    beside pos0 and the edges fails it on every pair the kernels test, winners or not."""
    tris = engine.scene_tris(0, len(before))
    assert_records_kept(before, tris)
    like = dataclasses.replace(sc, tris=tris)
    p0, e1, e2 = (tris[f].astype(np.float64) for f in ("pos0", "posedge1", "posedge2"))
    r0, r1, r2 = (before[f].astype(np.float64) for f in ("pos0", "posedge1", "posedge2"))
    for k, V in moved.items():
        part = MC.parts(name)[k]
        gd = C.deformed_geometry(like, k, V, part.idx, leaves[k])
        gr = C.deformed_geometry(like, k, part.pos, part.idx, leaves[k])
        lo, hi = gd.ranges[k]
        p0[lo:hi], e1[lo:hi], e2[lo:hi] = gd.p0[lo:hi], gd.e1[lo:hi], gd.e2[lo:hi]
        r0[lo:hi], r1[lo:hi], r2[lo:hi] = gr.p0[lo:hi], gr.e1[lo:hi], gr.e2[lo:hi]
    engine.tlas_refit(sc.tlas_nodes, C.world_boxes(BF.Geometry.from_scene(like, p0, e1, e2)) if boxes is None else boxes)
    device_scene_checks(engine, name, two_models(name, sc, tris, leaves, (p0, e1, e2), (r0, r1, r2)))


def test_after_gpu_blas_refit_of_the_affine_soup(atlas_engine, side):
    """tt_blas_refit rewrites pos0 and the edges inside the 88-byte records; the UVs and MatDat beside them must
    still be the rest mesh's."""
    side.uploaded = None
    name = "soup"
    part = MC.parts(name)[0]
    blas = tthip.Blas(part.mesh())
    sc = MC.assemble(name, [blas]).build()
    atlas_engine.upload(sc)
    before = atlas_engine.scene_tris(0, len(sc.tris))
    V = C.deformed_vertices(part.pos)
    leaf = blas.leaf_order()
    atlas_engine.blas_refit(0, C.vertex_buffer(V), part.idx.reshape(-1), leaf)
    refit_checks(atlas_engine, name, sc, before, {0: V}, [leaf])


def test_after_gpu_blas_refit_many_of_two_assembled_objects(atlas_engine, side):
    """tt_blas_refit_many on the two icospheres of the device-assembled scene, the ground left alone; the world
    boxes the call writes feed the TLAS refit."""
    side.uploaded = None
    name = "parts"
    sc, objects = assembled_objects(atlas_engine, name)
    try:
        before = atlas_engine.scene_tris(0, sc.meta["n_tris_total"])
        leaves = [o.read()[2] for o in objects]
        moved, items = {}, []
        for k in (1, 2):
            part = MC.parts(name)[k]
            moved[k] = C.deformed_vertices(part.pos)
            items.append(tthip.RefitItem(k, len(part.idx), leaves[k],
                                         [tthip.RefitPart(C.vertex_buffer(moved[k]), part.idx.reshape(-1))], part.l2w))
        boxes = np.ascontiguousarray(sc.meta["mesh_aabbs"], np.float32).copy()
        atlas_engine.blas_refit_many(items, mesh_aabbs=boxes)
        refit_checks(atlas_engine, name, sc, before, moved, leaves, boxes)
    finally:
        for o in objects:
            o.destroy()


def test_damaged_records_are_reported(atlas_engine, side):
    """What a refit that harmed the fields beside the positions would leave: the soup uploaded with the MatDat of one
    record, the robust winner of the most rays, set to the material that rejects everything. The field comparison
    names MatDat (and tex0, edited likewise); the surface model, whose MatDat comes from the mesh, reports the rays;
    the record model, which reads the damaged records as the kernels do, reports nothing, which is why it does not
    stand alone."""
    side.uploaded = None
    name = "soup"
    part = MC.parts(name)[0]
    blas = tthip.Blas(part.mesh())
    sc = MC.assemble(name, [blas]).build()
    rays = MC.closest_rays(name, "random")
    n = len(rays) // 2
    ref = MC.model(name).closest(rays["origin"][:n], rays["direction"][:n], FAR, 0, 1)
    won = ref.tri[ref.hit & ref.robust]
    victim = int(np.bincount(won).argmax())
    damaged = sc.tris.copy()
    damaged["MatDat"][victim] = 8  # cutoff 1.5
    assert sc.tris["MatDat"][victim] != 8
    atlas_engine.upload(dataclasses.replace(sc, tris=damaged))
    tris = atlas_engine.scene_tris(0, len(sc.tris))
    with pytest.raises(AssertionError, match="MatDat, first record %d" % victim):
        assert_records_kept(sc.tris, tris)
    shifted = sc.tris.copy()
    shifted["tex0"][victim, 1] += np.float32(0.25)
    with pytest.raises(AssertionError, match="tex0, first record %d" % victim):
        assert_records_kept(sc.tris, shifted)
    reports = device_scene_reports(atlas_engine, name, two_models(name, sc, tris, [blas.leaf_order()]))
    assert sum(r.mismatches for r in reports["record"]) == 0, [r.failures for r in reports["record"]]
    assert sum(r.mismatches for r in reports["surface"]) >= 1
    assert any("robust rays differ" in t for r in reports["surface"] for t in r.failures)
