"""Terrains without a GPU: the tt_terrain layout, every refusal of the upload's validator, and the scalar host
reference (host/tt_terrain.cpp) of the two heightmap kernels -- against an analytic plane, against a table of
special rays derived by hand from IntersectionKernels.compute:513-703, under the sanitizers in a stand-alone
program, and for the coverage the randomized GPU set (tests/terrain_cases.py) must have."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_ctypes as O
import terrain_cases as TC
import tthip

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HDR = open(os.path.join(REPO, "include", "truetrace_hip.h")).read()
TID = tthip.TT_TERRAIN_MESH_ID


# ------------------------------------------------------------------ layout
def test_terrain_layout_matches_the_reference_struct():
    d = tthip.TERRAIN_DTYPE
    assert d.itemsize == 60
    offs = {n: d.fields[n][1] for n in d.names}
    # TerrainData: float3 PositionOffset; float HeightScale; float2 TerrainDim; float4 AlphaMap; float4 HeightMap;
    # int MatOffset (CommonData.cginc:280-287)
    assert offs == {"PositionOffset": 0, "HeightScale": 12, "TerrainDim": 16, "AlphaMap": 24, "HeightMap": 40,
                    "MatOffset": 56}
    assert re.search(r"TT_STATIC_ASSERT\(sizeof\(tt_terrain\) == 60", HDR)
    assert int(re.search(r"#define TT_TERRAIN_MESH_ID (\d+)u", HDR).group(1)) == TID == 9999999
    assert int(re.search(r"#define TT_TERRAIN_MAX_STEPS (\d+)", HDR).group(1)) == tthip.TT_TERRAIN_MAX_STEPS == 2000


def test_new_entry_points_are_exported():
    L, S = tthip.hip_lib(), tthip.scene_lib()
    for name in ["tt_scene_upload_terrains", "tt_terrain_validate", "tt_trace_heightmap", "tt_trace_heightmap_indirect",
                 "tt_trace_shadow_heightmap", "tt_trace_shadow_heightmap_indirect"]:
        assert hasattr(L, name), name
    for name in ["tt_terrain_trace_host", "tt_terrain_trace_detail_host", "tt_terrain_occluded_host",
                 "tt_terrain_normal_host"]:
        assert hasattr(S, name), name


# ------------------------------------------------------------------ upload refusals (host-only validator)
def _good():
    return TC.terrains().copy(), TC.atlas()


def test_validator_accepts_the_test_scene_and_an_empty_set():
    t, a = _good()
    assert tthip.terrain_validate(t, a) == (tthip.TT_OK, "")
    assert tthip.terrain_validate(np.zeros(0, tthip.TERRAIN_DTYPE), None)[0] == tthip.TT_OK


@pytest.mark.parametrize("field,index", [("PositionOffset", 1), ("HeightScale", None), ("TerrainDim", 0),
                                         ("AlphaMap", 3), ("HeightMap", 2)])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_validator_refuses_non_finite_fields(field, index, bad):
    t, a = _good()
    if index is None:
        t[1][field] = bad
    else:
        t[1][field][index] = bad
    st, why = tthip.terrain_validate(t, a)
    assert st == tthip.TT_ERR_INVALID_ARG
    assert "terrain 1" in why and field in why and "finite" in why


@pytest.mark.parametrize("k,value", [(0, 1.0001), (1, -0.0001), (2, 2.0), (3, -1.0)])
def test_validator_refuses_rectangles_outside_the_atlas(k, value):
    t, a = _good()
    t[0]["HeightMap"][k] = value
    st, why = tthip.terrain_validate(t, a)
    assert st == tthip.TT_ERR_INVALID_ARG and "terrain 0" in why and "[0, 1]" in why


def test_validator_refuses_missing_arrays():
    t, a = _good()
    L = tthip.hip_lib()
    why = C.create_string_buffer(128)
    assert L.tt_terrain_validate(None, 2, a.ctypes.data, 64, 48, why, 128) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_terrain_validate(t.ctypes.data, 2, None, 64, 48, why, 128) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_terrain_validate(t.ctypes.data, 2, a.ctypes.data, 0, 48, why, 128) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_terrain_validate(t.ctypes.data, 2, a.ctypes.data, 64, 0, why, 128) == tthip.TT_ERR_INVALID_ARG
    assert b"atlas" in why.value
    assert L.tt_terrain_validate(t.ctypes.data, 2, a.ctypes.data, 1 << 16, 1 << 16, None, 0) == tthip.TT_ERR_INVALID_ARG


def test_host_reference_refuses_bad_arguments():
    t, a = _good()
    S = tthip.scene_lib()
    p = tthip.TraceParams(n_rays=1, bounce=0, far_plane=TC.FAR, screen_width=1, screen_height=1, flags=0)
    rays = np.zeros(2, tthip.RAY_DTYPE)
    assert S.tt_terrain_trace_host(t.ctypes.data, 2, None, 64, 48, C.byref(p), rays.ctypes.data, None, None) == 1
    assert S.tt_terrain_trace_host(t.ctypes.data, 2, a.ctypes.data, 64, 48, None, rays.ctypes.data, None, None) == 1
    out = np.zeros(3, np.float32)
    pos = np.zeros(3, np.float32)
    assert S.tt_terrain_normal_host(t.ctypes.data, 2, a.ctypes.data, 64, 48, pos.ctypes.data, 2, out.ctypes.data) == 1


# ------------------------------------------------------------------ the KAT scene: constant heightmaps
# terrain 0: [0, 32]^2 from y = 0, surface y = 0.01 + 2 * 0.25 * 4 = 2.01; terrain 1: x in [40, 56], z in [0, 16],
# surface y = 0.01 + 2 * 0.25 * 4.4 = 2.21
def _kat_scene():
    hm = np.full((8, 8), 0.25, np.float16).view(np.uint16)
    t = np.zeros(2, tthip.TERRAIN_DTYPE)
    t[0]["HeightScale"], t[0]["TerrainDim"] = 4.0, (32.0, 32.0)
    t[1]["PositionOffset"], t[1]["HeightScale"], t[1]["TerrainDim"] = (40.0, 0.0, 0.0), 4.4, (16.0, 16.0)
    t["HeightMap"] = (1.0, 1.0, 0.0, 0.0)
    return t, hm


def _rays(specs):
    """specs: (origin, direction, t, mesh_id, triangle_id) per ray; PixelIndex = its index."""
    r = np.zeros(len(specs), tthip.RAY_DTYPE)
    for i, (o, d, t, mesh, tri) in enumerate(specs):
        d = np.asarray(d, np.float64)
        r[i]["origin"], r[i]["direction"] = o, (d / np.linalg.norm(d)).astype(np.float32)
        r[i]["PixelIndex"] = i
        r[i]["hits"] = (mesh, tri, np.float32(t).view(np.uint32), 0)
    return r


def test_rays_from_above_end_on_the_analytic_plane():
    """A constant heightmap h makes the surface the plane y = offset.y + 0.01 + 2 h HeightScale. The march accepts a
    sample within 1e-4 / g = 2.24e-4 of it; the reported t lies 0.0001 before that sample (the origin shift of :649
    is not part of t), so the hit height is within 3.3e-4 plus rounding of the plane: 5e-4 at coordinates <= 64.
    u, v are the last sample's x / dimX, z / dimY, within the 16-bit packing's 1 / 65535 (plus 4e-7 for the float
    roundings of this check's own x, z and divisions at coordinates <= 64)."""
    t, hm = _kat_scene()
    rng = np.random.default_rng(5)
    n = 512
    tgt = np.stack([rng.uniform(2, 30, n), np.full(n, 2.01), rng.uniform(2, 30, n)], 1)
    org = np.stack([rng.uniform(2, 30, n), rng.uniform(8, 28, n), rng.uniform(2, 30, n)], 1)
    rays = np.zeros(2 * 32 * 32, tthip.RAY_DTYPE)
    rays[:n] = _rays([(o, g - o, TC.FAR, 0, 0) for o, g in zip(org, tgt)])
    stats = tthip.terrain_trace_host(t, hm, rays, n, 0, TC.FAR, 32, 32)
    h = rays["hits"][:n]
    assert stats.hits == n and np.all(h[:, 0] == TID) and np.all(h[:, 1] == 0)
    tt = h[:, 2].view(np.float32)
    o, d = rays["origin"][:n], rays["direction"][:n]
    y = o[:, 1] + d[:, 1] * tt
    assert np.abs(y - np.float32(2.01)).max() <= 5e-4
    ts = tt + np.float32(0.0001)
    x, z = o[:, 0] + d[:, 0] * ts, o[:, 2] + d[:, 2] * ts
    u = (h[:, 3] & 0xFFFF).astype(np.float32) / np.float32(65535.0)
    v = (h[:, 3] >> 16).astype(np.float32) / np.float32(65535.0)
    tol = 1.0 / 65535.0 + 4e-7
    assert np.abs(u - x / np.float32(32.0)).max() <= tol and np.abs(v - z / np.float32(32.0)).max() <= tol


# (origin, direction, record t, record mesh, record triangle), then: hit?, terrain index. Derived by hand:
SPECIAL = [
    # straight down, two zero direction components: the x and z slabs give (-inf, +inf), t0 = 0.025, and the march
    # converges on y = 2.01 long before 2,000 steps
    (((10, 25, 10), (0, -1, 0), TC.FAR, 0, 0), True, 0),
    # horizontal at y = 25: each step is (25 - 2.01) g = 10.28 long, the third sample is past x = 32; terrain 1's box
    # tops out at y = 16
    (((10, 25, 10), (1, 0, 0), TC.FAR, 0, 0), False, 0),
    # starts inside the box above the surface (t0 = the 0.025 floor), reaches y = 2.01 at x = 22 < 32
    (((16, 10, 16), (0.6, -0.8, 0), TC.FAR, 0, 0), True, 0),
    # starts below the surface: the first sample has q.y < 0 (dist = 0, throwa), the bisection halves PrevDist = 0
    # ten times and the hit is at CurDist = 0, t = t0
    (((16, 1, 16), (0, 1, 0), TC.FAR, 0, 0), True, 0),
    (((16, 1, 16), (1, 0, 0), TC.FAR, 0, 0), True, 0),
    # y = 3 clears both surfaces (2.01, 2.21): steps of ~0.44 / ~0.35 carry it out through each far side
    (((-5, 3, 8), (1, 0, 0), TC.FAR, 0, 0), False, 0),
    # descends 0.02 per unit x from y = 3.27 at x = -5: y = 2.53 leaving terrain 0 at x = 32 (above 2.01), 2.37
    # entering terrain 1 at x = 40 (above 2.21), and reaches 2.21 at x = 48 < 56
    (((-5, 3.27, 8), (1, -0.02, 0), TC.FAR, 0, 0), True, 1),
    # a triangle hit at t = 5: the box passes (t0 = 0.025 <= t1 = 5) but the first step, 10.27, ends CurDist < 5
    (((10, 25, 10), (0, -1, 0), 5.0, 0, 7), False, 0),
    # a triangle hit nearer than the 0.025 floor: t0 = 0.025 > t1 = 0.01, no march
    (((10, 25, 10), (0, -1, 0), 0.01, 0, 7), False, 0),
    # beside the footprint: the x slab gives an empty interval
    (((-10, 25, 10), (0, -1, 0), TC.FAR, 0, 0), False, 0),
    # straight down onto terrain 1 only
    (((48, 10, 8), (0, -1, 0), TC.FAR, 0, 0), True, 1),
]


def test_special_rays_match_the_hand_derived_table():
    t, hm = _kat_scene()
    n = len(SPECIAL)
    rays = np.zeros(2 * 16, tthip.RAY_DTYPE)
    rays[:n] = _rays([s[0] for s in SPECIAL])
    before = rays.copy()
    info = np.full((16, 4), 0xABABABAB, np.uint32)
    detail = np.zeros(n, np.uint32)
    tthip.terrain_trace_host(t, hm, rays, n, 0, TC.FAR, 4, 4, info=info, detail=detail)
    for i, (_, hit, terrain) in enumerate(SPECIAL):
        rec = rays["hits"][i]
        assert (rec[0] == TID) == hit, i
        if hit:
            assert rec[1] == terrain, i
            assert tuple(info[i][:2]) == (TID, terrain), i
        else:  # a miss leaves the record and the texel untouched
            assert np.array_equal(rec, before["hits"][i]), i
            assert np.all(info[i] == 0xABABABAB), i
    assert detail[3] & 2 and detail[4] & 2, "the rays from below the surface take the bisection"
    assert rays["hits"][3, 2].view(np.float32) == np.float32(0.025)  # CurDist = 0, t = t0
    # the shadow form of the same rays (max distance 60): those that hit within reach are occluded
    s = np.zeros(n, tthip.SHADOW_DTYPE)
    s["origin"], s["direction"], s["t"] = before["origin"][:n], before["direction"][:n], -60.0
    s["t"][2] = 0.0  # not marched
    occ, _ = tthip.terrain_occluded_host(t, hm, s, n)
    assert list(occ) == [1, 0, 0, 1, 1, 0, 1, 1, 1, 0, 1]  # rays 7 and 8: no triangle record culls a shadow ray


def test_flat_heightmap_normal_points_as_the_reference_writes_it():
    t, hm = _kat_scene()
    # cross(normalize(+x step), normalize(+z step)) on a flat surface: (0, -1, 0)
    assert np.array_equal(tthip.terrain_normal_host(t, hm, (10.0, 2.01, 10.0), 0), np.float32([0, -1, 0]))


# ------------------------------------------------------------------ sanitizers
def test_host_reference_under_sanitizers(tmp_path):
    """The stand-alone KAT program (its own main, no Python in the run) built with ASan + UBSan together with
    host/tt_terrain.cpp."""
    exe = tmp_path / "terrain_kat"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(HERE, "native", "terrain_kat_main.cpp"),
                    os.path.join(REPO, "truetrace-unity-pathtracer_amd", "host", "tt_terrain.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout and "runtime error" not in r.stderr


# ------------------------------------------------------------------ coverage of the randomized GPU set
def test_randomized_set_covers_every_path():
    """Asserted on the reference's output for the set tests/test_gpu_terrain.py runs on the GPU (bounce 1, the odd
    half): records as the triangle oracle leaves them, then the terrain march."""
    T, A, S = TC.terrains(), TC.atlas(), TC.scene()
    n, off = TC.N_RANDOM, TC.RW * TC.RH
    rays = np.zeros(2 * off, tthip.RAY_DTYPE)
    rays[off:off + n] = TC.random_rays()
    assert O.trace(S, rays, n, 1, TC.FAR, TC.RW, TC.RH)[0] == 0
    free = rays.copy()
    TC.miss_records(free[off:off + n])
    det, det_free = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    stats = tthip.terrain_trace_host(T, A, rays, n, 1, TC.FAR, TC.RW, TC.RH, detail=det)
    tthip.terrain_trace_host(T, A, free, n, 1, TC.FAR, TC.RW, TC.RH, detail=det_free)
    hit = (det & 1) == 1
    assert stats.hits == hit.sum() and stats.rays == n
    assert hit.mean() >= 0.25
    assert ((det >> 1) & 1).mean() >= 0.02, "bisection"
    assert ((det >> 2) & 1).sum() >= 1 and stats.reps_exhausted >= 1, "a march at the 2,000-step bound"
    over_first = ((det >> 8) & 1) == 1  # marched through terrain 0's box ...
    assert (over_first & (((det >> 16) & 1) == 0) & (((det >> 17) & 1) == 1)).mean() >= 0.05  # ... then hit terrain 1
    culled = ((det_free & 1) == 1) & ~hit  # would hit a terrain, but the triangle hit is nearer
    assert culled.mean() >= 0.10
    assert stats.node_visits > 20 * n


def test_shadow_set_mixes_signs_zeros_and_occlusion():
    s = TC.shadow_rays()
    occ, stats = tthip.terrain_occluded_host(TC.terrains(), TC.atlas(), s, TC.N_SHADOW)
    assert (s["t"] == 0).mean() > 0.05 and (s["t"] > 0).mean() > 0.3 and (s["t"] < 0).mean() > 0.3
    assert stats.rays == (s["t"] != 0).sum() and stats.hits == occ.sum()
    assert 0.1 < occ.mean() < 0.5 and not occ[s["t"] == 0].any()


def test_synthetic_heightmap_is_seeded_hills_plus_a_step():
    a, b = tthip.synthetic_heightmap(7, 40, 24), tthip.synthetic_heightmap(7, 40, 24)
    assert a.dtype == np.uint16 and a.shape == (24, 40) and np.array_equal(a, b)
    assert not np.array_equal(a, tthip.synthetic_heightmap(8, 40, 24))
    f = a.view(np.float16).astype(np.float32)
    assert f.min() >= 0.0 and f.max() <= 1.0
    jumps = np.abs(np.diff(f, axis=1)).max(axis=0)  # per column boundary: the step is one column wide
    assert jumps.max() > 0.3 and np.sort(jumps)[-2] < 0.2
