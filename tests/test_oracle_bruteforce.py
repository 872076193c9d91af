"""The oracle against geometry: CWBVH8 traversal must give the answers of a float64 brute-force
Moller-Trumbore over every triangle of every instance (bruteforce.py; numpy, neither nodes nor TLAS read).
Golden fixtures pin the oracle against itself over time and the GPU parity tests pin the kernels against
the oracle; this file pins the oracle against truth, for the closest hit under every launch flag and at
both bounces, for the any-hit loop in both of its modes, and for axis-parallel rays whose slabs are inf / NaN.

A ray whose answer could turn on a float32 rounding is unrobust (bruteforce.py has the predicates) and only
counted; every other ray must agree exactly on miss / (mesh, triangle) or on occluded / visible, and every
hit on the reference's triangle must have t and its uv codes within the conditioned bound of
bruteforce_cases.compare_closest. test_gpu_bruteforce.py makes the same comparison for the kernels."""
import dataclasses
import functools

import numpy as np
import pytest

import bruteforce as BF
import bruteforce_cases as C
import oracle_ctypes as O
import tthip

FAR = C.FAR
THREADS = 4


# ------------------------------------------------------------------ the cases this file had before the matrix
def _check(sc, rays, n):
    """Flags 0, bounce 0, the scene as it is (test_blas_refit.py uses this too)."""
    r = rays.copy()
    st, _ = O.trace(sc, r, n, 0, FAR, n, 1, nthreads=THREADS)
    assert st == 0
    ref = C.reference_closest(BF.Geometry.from_scene(sc), rays, n, 0, 0)
    hits = r["hits"][:n]
    assert np.all(hits[~ref.exact, 1] == 0xFFFFFFFF), "oracle hit something brute force misses"
    assert (ref.robust & ref.hit).sum() > 0.3 * n
    C.compare_closest(ref, hits, caps=False).check()


def _random_rays(rng, n, center, spread):
    rays = np.zeros(2 * n, tthip.RAY_DTYPE)
    rays["origin"][:n] = center + rng.uniform(-spread, spread, (n, 3))
    d = rng.normal(size=(n, 3))
    rays["direction"][:n] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays["PixelIndex"][:n] = np.arange(n)
    return rays


@pytest.mark.parametrize("seed", [1, 2])
def test_single_blas_soup_matches_brute_force(seed):
    sc = tthip.single_object_scene(tthip.Mesh.soup(seed, 3000, 2.0, 0.2))
    rng = np.random.default_rng(seed)
    rays = _random_rays(rng, 400, np.zeros(3), 3.0)
    _check(sc, rays, 400)


def test_two_level_instances_match_brute_force():
    rng = np.random.default_rng(11)
    am = tthip.AssetManager()
    am.add_parent(tthip.Blas(tthip.Mesh.soup(5, 800, 6.0, 0.6)), tthip.trs_matrix((0, 0, 0)), np.zeros(2, tthip.MAT_DTYPE))
    props = [am.add_instance_parent(tthip.Blas(tthip.Mesh.prop(100 + k, int(rng.integers(60, 400)))),
                                    np.zeros(2, tthip.MAT_DTYPE)) for k in range(3)]
    for i in range(12):
        am.add_instance(props[i % 3], tthip.trs_matrix(rng.uniform(-8, 8, 3) * [1, 0.2, 1],
                                                       float(rng.uniform(0, 360)), float(rng.uniform(0.4, 1.5))))
    sc = am.build()
    rays = _random_rays(rng, 300, np.array([0.0, 2.0, 0.0]), 8.0)
    _check(sc, rays, 300)


def test_sponza_shaped_c2_matches_brute_force():
    """C2's 262k-triangle BLAS (the bench scene), random rays from around the bench camera."""
    import ttconfigs as T

    sc = T.c2_sponza()
    rng = np.random.default_rng(3)
    rays = _random_rays(rng, 128, np.array(T.C2_VIEW.position), 1.0)
    _check(sc, rays, 128)


# ------------------------------------------------------------------ closest-hit matrix
N_RAYS = 600
RAY_SETS = ("random", "axis")


@functools.lru_cache(maxsize=None)
def closest_rays(name, ray_set):
    g = C.geometry(name)
    seed = 100 + C.SCENES.index(name)
    o, d = C.random_rays(g, seed, N_RAYS) if ray_set == "random" else C.axis_rays(g, seed, N_RAYS)
    return C.ray_buffer(o, d)


def oracle_closest(sc, rays, flags, bounce):
    n = len(rays) // 2
    r = rays.copy()
    st, _ = O.trace(sc, r, n, bounce, FAR, n, 1, flags=flags, nthreads=THREADS)
    assert st == 0
    other = slice(n, 2 * n) if bounce == 0 else slice(0, n)
    assert r[other].tobytes() == rays[other].tobytes(), "the other half of the ping-pong buffer was written"
    return r["hits"][n * bounce:n * bounce + n]


@pytest.mark.parametrize("bounce", [0, 1])
@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("ray_set", RAY_SETS)
@pytest.mark.parametrize("name", C.SCENES)
def test_closest_matrix(name, ray_set, flags, bounce):
    rays = closest_rays(name, ray_set)
    hits = oracle_closest(C.scene(name), rays, flags, bounce)
    ref = C.reference_closest(C.geometry(name), rays, len(hits), flags, bounce)
    C.compare_closest(ref, hits).check()


# ------------------------------------------------------------------ any-hit matrix
SHADOW_SETS = ("random", "axis", "nee")
# the NEE set needs something between a surface and the light: Cornell's walls and the ground have nothing
SHADOW_CASES = [(name, s) for name in C.SCENES for s in SHADOW_SETS if s != "nee" or name in ("soup", "instances")]


@functools.lru_cache(maxsize=None)
def shadow_rays(name, ray_set):
    """(rays, width, height) of a shadow case."""
    g = C.geometry(name, "shadow")
    seed = 200 + C.SCENES.index(name)
    if ray_set == "nee":
        c2w, ip, light = C.nee_camera(g)
        frame = O.generate(c2w, ip, C.NEE_W, C.NEE_H, 0.05, FAR)
        n = C.NEE_W * C.NEE_H
        assert O.trace(C.scene(name, "shadow"), frame, n, 0, FAR, C.NEE_W, C.NEE_H, nthreads=THREADS)[0] == 0
        return C.nee_shadow_rays(frame, light, seed), C.NEE_W, C.NEE_H
    if ray_set == "axis":
        o, d = C.axis_rays(g, seed, N_RAYS)
        return C.axis_shadow_buffer(g, o, d, seed), N_RAYS, 1
    o, d = C.random_rays(g, seed, N_RAYS)
    return C.shadow_buffer(o, d, seed), N_RAYS, 1


def oracle_any_hit(sc, before, W, H, bounce, visibility_check):
    after = before.copy()
    vis, col, nee = C.shadow_outputs(len(before), W * H)
    st, cnt = O.shadow(sc, after, len(after), bounce, W, H, visibility=vis, colors=col, nee_pos=nee, counts=True,
                       nthreads=THREADS, flags=tthip.TT_SHADOW_VISIBILITY_CHECK if visibility_check else 0)
    assert st == 0
    return after, vis, col, nee, cnt["status"]


@pytest.mark.parametrize("visibility_check", [False, True], ids=["default", "vischeck"])
@pytest.mark.parametrize("bounce", [0, 1])
@pytest.mark.parametrize("name,ray_set", SHADOW_CASES)
def test_any_hit_matrix(name, ray_set, bounce, visibility_check):
    before, W, H = shadow_rays(name, ray_set)
    after, vis, col, nee, status = oracle_any_hit(C.scene(name, "shadow"), before, W, H, bounce, visibility_check)
    ref = C.reference_any_hit(C.geometry(name, "shadow"), before, visibility_check)
    C.compare_any_hit(ref, before, after, vis, col, nee, bounce, visibility_check, status).check()


# ------------------------------------------------------------------ the comparison must be able to fail
def test_comparison_fails_for_a_reference_without_invisible():
    rays = closest_rays("soup", "random")
    hits = oracle_closest(C.scene("soup"), rays, 0, 0)
    wrong = C.reference_closest(C.geometry("soup"), rays, len(hits), 0, 0, honour_invisible=False)
    rep = C.compare_closest(wrong, hits)
    assert rep.mismatches > 0 and rep.failures, rep.text


def test_comparison_fails_for_a_reference_without_shadow_tags():
    before, W, H = shadow_rays("soup", "random")
    after, vis, col, nee, status = oracle_any_hit(C.scene("soup", "shadow"), before, W, H, 0, False)
    wrong = C.reference_any_hit(C.geometry("soup", "shadow"), before, honour_tags=False)
    rep = C.compare_any_hit(wrong, before, after, vis, col, nee, 0, False, status)
    assert rep.mismatches > 0 and rep.failures, rep.text


def test_comparison_fails_for_a_blas_root_that_lost_a_child():
    """The oracle walks a scene whose BLAS root has the meta byte of one live child zeroed (the child is never
    entered); the reference sees the true triangles."""
    sc = C.scene("soup")
    root = int(sc.meshdata["mesh_data_bvh_offsets"][0]) & 0x7FFFFFFF
    nodes = sc.nodes.copy()
    meta = nodes[root:root + 1]["meta"].copy().view(np.uint8).reshape(8)
    live = np.nonzero(meta)[0]
    assert len(live) > 1
    meta[live[0]] = 0
    nodes["meta"][root] = meta.view(np.uint32)
    rays = closest_rays("soup", "random")
    hits = oracle_closest(dataclasses.replace(sc, nodes=nodes), rays, 0, 0)
    rep = C.compare_closest(C.reference_closest(C.geometry("soup"), rays, len(hits), 0, 0), hits)
    assert rep.mismatches > 0 and rep.failures, rep.text


# ------------------------------------------------------------------ after the refits
def test_closest_after_a_blas_refit_of_deformed_vertices():
    """The oracle's BLAS refit (then its TLAS refit, as a caller runs them) of the soup under a smooth
    displacement; the reference sees triangles rebuilt in float64 from the deformed vertex array."""
    sc, pos, idx, leaf = C.refit_soup()
    V = C.deformed_vertices(pos)
    st, nodes, tris = O.blas_refit(sc, 0, C.vertex_buffer(V), idx, leaf)
    assert st == 0
    g = C.deformed_geometry(sc, 0, V, idx, leaf)
    sc2 = dataclasses.replace(sc, nodes=nodes, tris=tris)
    st, nodes2 = O.tlas_refit(sc2, C.world_boxes(g))
    assert st == 0
    o, d = C.random_rays(g, 31, N_RAYS)
    rays = C.ray_buffer(o, d)
    hits = oracle_closest(dataclasses.replace(sc2, nodes=nodes2), rays, 0, 0)
    C.compare_closest(C.reference_closest(g, rays, N_RAYS, 0, 0), hits).check()


def test_closest_after_a_tlas_refit_of_moved_instances():
    """Six of the twelve instances moved: new mesh records, world boxes from the moved triangles, the TLAS
    refit with its topology kept; the reference uses the new W2L."""
    a, meshdata, g, boxes = C.moved_instances()
    moved = dataclasses.replace(a, meshdata=meshdata)
    st, nodes = O.tlas_refit(moved, boxes)
    assert st == 0
    o, d = C.random_rays(g, 32, N_RAYS)
    rays = C.ray_buffer(o, d)
    hits = oracle_closest(dataclasses.replace(moved, nodes=nodes), rays, 0, 0)
    C.compare_closest(C.reference_closest(g, rays, N_RAYS, 0, 0), hits).check()
