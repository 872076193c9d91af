"""The kernels against geometry, with no oracle in between: what the leaf-TLAS kernel, the generic
two-level kernel and the any-hit kernel write is compared with the float64 brute force of bruteforce.py, on
the scenes, ray sets, caps and assertions of test_oracle_bruteforce.py (bruteforce_cases.py holds them), and
again after a GPU BLAS refit and a GPU TLAS refit. The parity tests prove kernel == oracle bit for bit; an error
the two share passes them all and fails here. The oracle is not called in this file."""
import functools

import numpy as np
import pytest

import bruteforce_cases as C
import tthip

pytestmark = pytest.mark.gpu

FAR = C.FAR
N_RAYS = 600
N_SHORT = 65  # one full wave and one lane of the next
LEAF, GENERIC = tthip.TT_TRACE_FORM_LEAF, tthip.TT_TRACE_FORM_GENERIC


@functools.lru_cache(maxsize=None)
def closest_rays(name, ray_set):
    g = C.geometry(name)
    seed = 100 + C.SCENES.index(name)
    o, d = C.random_rays(g, seed, N_RAYS) if ray_set == "random" else C.axis_rays(g, seed, N_RAYS)
    return C.ray_buffer(o, d)


def gpu_closest(engine, rays, n, flags, bounce, form=None):
    """Traces the first n rays of a buffer of N_RAYS pixels on the uploaded scene; returns their hit records."""
    W = len(rays) // 2
    r = rays.copy()
    engine.trace(r, n, bounce, FAR, W, 1, flags=flags)
    if form is not None:
        assert engine.last_trace_form() == form
    keep = np.ones(len(r), bool)
    keep[W * bounce:W * bounce + n] = False
    assert r[keep].tobytes() == rays[keep].tobytes(), "a ray outside the launch was written"
    return r["hits"][W * bounce:W * bounce + n]


def check_closest(engine, sc, g, rays, flags, bounce, form):
    engine.upload(sc)
    ref = C.reference_closest(g, rays, N_RAYS, flags, bounce)
    C.compare_closest(ref, gpu_closest(engine, rays, N_RAYS, flags, bounce, form)).check()
    # a launch that ends one lane into a wave: the same rays, the same answers
    C.compare_closest(C.head(ref, N_SHORT), gpu_closest(engine, rays, N_SHORT, flags, bounce, form), caps=False).check()


def one_instance_form(kind, flags, bounce):
    """The form tt_trace_last_form documents for a scene of one instance: the leaf-TLAS kernel serves the
    launches that need no material check, and a launch needs one for an Invisible material or IGNORE_BACKFACING
    at bounce 0 and for IGNORE_GLASS over a glass material (every table here has glass)."""
    check = bounce == 0 and (kind == "closest" or flags & tthip.TT_TRACE_IGNORE_BACKFACING)
    return GENERIC if check or flags & tthip.TT_TRACE_IGNORE_GLASS else LEAF


# the table with Invisible materials under every flag; the table without, where bounce 0 takes the leaf kernel too
LEAF_LAUNCHES = [("closest", f) for f in C.FLAGS] + [("glass", 0), ("glass", C.FLAGS[3])]


@pytest.mark.parametrize("bounce", [0, 1])
@pytest.mark.parametrize("kind,flags", LEAF_LAUNCHES)
@pytest.mark.parametrize("ray_set", ["random", "axis"])
@pytest.mark.parametrize("name", C.LEAF_SCENES)
def test_one_instance_closest(engine, name, ray_set, kind, flags, bounce):
    """Scenes of one instance: the leaf-TLAS kernel wherever the launch qualifies for it (asserted), the generic
    kernel behind its material check elsewhere."""
    check_closest(engine, C.scene(name, kind), C.geometry(name, kind), closest_rays(name, ray_set), flags, bounce,
                  one_instance_form(kind, flags, bounce))


@pytest.mark.parametrize("bounce", [0, 1])
@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("ray_set", ["random", "axis"])
def test_generic_kernel_closest(engine, ray_set, flags, bounce):
    check_closest(engine, C.scene("instances"), C.geometry("instances"), closest_rays("instances", ray_set), flags,
                  bounce, GENERIC)


# ------------------------------------------------------------------ any-hit kernel
@pytest.fixture(scope="module")
def atlas_engine(engine):
    """A context of this module's own for the scenes with glass: their texture atlas stays with a context for
    good (no call takes it away again), and tests of the shared context rely on its having none."""
    eng = tthip.Engine(0)
    yield eng
    eng.close()


def shadow_rays(engine, name, ray_set):
    """(rays, width, height); the NEE set comes from a frame the engine generates and traces itself."""
    g = C.geometry(name, "shadow")
    seed = 200 + C.SCENES.index(name)
    if ray_set == "nee":
        c2w, ip, light = C.nee_camera(g)
        frame = np.zeros(2 * C.NEE_W * C.NEE_H, tthip.RAY_DTYPE)
        engine.generate(frame, c2w, ip, C.NEE_W, C.NEE_H, 0.05, FAR)
        engine.trace(frame, C.NEE_W * C.NEE_H, 0, FAR, C.NEE_W, C.NEE_H)
        return C.nee_shadow_rays(frame, light, seed), C.NEE_W, C.NEE_H
    if ray_set == "axis":
        o, d = C.axis_rays(g, seed, N_RAYS)
        return C.axis_shadow_buffer(g, o, d, seed), N_RAYS, 1
    o, d = C.random_rays(g, seed, N_RAYS)
    return C.shadow_buffer(o, d, seed), N_RAYS, 1


@pytest.mark.parametrize("ray_set", ["random", "axis", "nee"])
@pytest.mark.parametrize("name", ["soup", "instances"])
def test_any_hit_kernel(atlas_engine, name, ray_set):
    """Bounce 0 and 1, the default mode and the visibility check; occlusion is read from the in-place t and
    the visibility rows."""
    engine = atlas_engine
    engine.upload(C.scene(name, "shadow"))
    before, W, H = shadow_rays(engine, name, ray_set)
    g = C.geometry(name, "shadow")
    for visibility_check in (False, True):
        ref = C.reference_any_hit(g, before, visibility_check)
        for bounce in (0, 1):
            after = before.copy()
            vis, col, nee = C.shadow_outputs(len(before), W * H)
            engine.trace_shadow(after, len(after), bounce, W, H, visibility=vis, colors=col, nee_pos=nee,
                                flags=tthip.TT_SHADOW_VISIBILITY_CHECK if visibility_check else 0)
            C.compare_any_hit(ref, before, after, vis, col, nee, bounce, visibility_check).check()


# ------------------------------------------------------------------ after the GPU refits
def test_closest_after_gpu_blas_refit(engine):
    """tt_blas_refit of the soup under a smooth displacement of at most 0.1, then the TLAS refit a caller runs
    next; the reference sees triangles rebuilt in float64 from the deformed vertex array, not the triangles the
    refit wrote. The device TLAS refit leaves the generic kernel; once the host has read node 0 back and written
    it again, the leaf-TLAS kernel walks the refit BLAS too."""
    sc, pos, idx, leaf = C.refit_soup()
    V = C.deformed_vertices(pos)
    g = C.deformed_geometry(sc, 0, V, idx, leaf)
    engine.upload(sc)
    engine.blas_refit(0, C.vertex_buffer(V), idx, leaf)
    engine.tlas_refit(sc.tlas_nodes, C.world_boxes(g))
    o, d = C.random_rays(g, 31, N_RAYS)
    rays = C.ray_buffer(o, d)
    for flags, bounce in ((0, 0), (C.FLAGS[3], 0), (0, 1)):
        ref = C.reference_closest(g, rays, N_RAYS, flags, bounce)
        C.compare_closest(ref, gpu_closest(engine, rays, N_RAYS, flags, bounce, GENERIC)).check()
    engine.update_nodes(0, engine.scene_nodes(0, sc.tlas_nodes))
    C.compare_closest(ref, gpu_closest(engine, rays, N_RAYS, 0, 1, LEAF)).check()


def test_closest_after_gpu_tlas_refit(engine):
    """Six of the twelve instances moved: update_meshdata, then tt_tlas_refit from world boxes computed in
    float64 from the moved triangles and rounded outward; the reference uses the new W2L."""
    a, meshdata, g, boxes = C.moved_instances()
    engine.upload(a)
    engine.update_meshdata(0, meshdata)
    engine.tlas_refit(a.tlas_nodes, boxes)
    o, d = C.random_rays(g, 32, N_RAYS)
    rays = C.ray_buffer(o, d)
    for flags, bounce in ((0, 0), (C.FLAGS[3], 0), (0, 1)):
        ref = C.reference_closest(g, rays, N_RAYS, flags, bounce)
        C.compare_closest(ref, gpu_closest(engine, rays, N_RAYS, flags, bounce)).check()
