"""The host reference of the enqueue's terrain rows (tt_terrain_bounce_host, host/tt_terrain.cpp) without a GPU,
pinned against the oracle (oracle/tt_oracle.c), which knows no terrains but shares every other step of the diffuse
subset: the random(1, pixel) draw and its pdf, the survive decision, and the origin offset along the unsmoothed
normal. The direction is checked against the terrain normal it was sampled about."""
import os
import re
import subprocess

import numpy as np

import oracle_ctypes as O
import terrain_cases as TC
import tthip

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HDR = open(os.path.join(REPO, "include", "truetrace_hip.h")).read()
TID = tthip.TT_TERRAIN_MESH_ID
W, H = 32, 16
N = W * H
MAXB = 4


def _flat():
    """One terrain with a constant heightmap (tests/test_terrain_host.py pins its normal: (0, -1, 0)), wide
    enough to hold the Cornell box's floor."""
    hm = np.full((8, 8), 0.25, np.float16).view(np.uint16)
    t = np.zeros(1, tthip.TERRAIN_DTYPE)
    t[0]["PositionOffset"] = (-16.0, -3.0, -16.0)
    t[0]["HeightScale"], t[0]["TerrainDim"], t[0]["HeightMap"] = 4.0, (32.0, 32.0), (1.0, 1.0, 0.0, 0.0)
    return t, hm


def _floor_frame():
    """N rays from inside the Cornell box down onto its floor (y = -1), traced by the oracle: triangle records.
    PixelIndex = the ray's index."""
    rng = np.random.default_rng(0x7E44B0)
    org = np.stack([rng.uniform(-0.3, 0.3, N), rng.uniform(0.2, 0.8, N), rng.uniform(2.0, 3.0, N)], 1)
    tgt = np.stack([rng.uniform(-0.9, 0.9, N), np.full(N, -1.0), rng.uniform(-0.9, 0.6, N)], 1)
    d = tgt - org
    rays = np.zeros(2 * N, tthip.RAY_DTYPE)
    rays["origin"][:N] = org.astype(np.float32)
    rays["direction"][:N] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays["PixelIndex"][:N] = np.arange(N)
    rays["last_pdf"] = 1.0
    TC.miss_records(rays)
    assert O.trace(TC.scene(), rays, N, 0, TC.FAR, W, H)[0] == 0
    return rays


def _as_terrain(rays, n):
    """The same rays with the same t and uv, as records of terrain 0."""
    out = rays.copy()
    hit = out["hits"][:n, 2].view(np.float32) < TC.FAR
    out["hits"][:n][hit, 0] = TID
    out["hits"][:n][hit, 1] = 0
    return out, hit


def _oracle_survivors(tri, frames):
    r = tri.copy()
    cnt = O.enqueue_bounce(TC.scene(), r, N, 0, TC.FAR, W, H, frames=frames, max_bounce=MAXB)
    return {int(x["PixelIndex"]): x for x in r[N:N + cnt]}


def test_same_draw_and_survive_decision_as_the_oracle():
    t, hm = _flat()
    tri = _floor_frame()
    ter, hit = _as_terrain(tri, N)
    assert hit.sum() > 300
    for frames in (3, 11):
        want = _oracle_survivors(tri, frames)
        out, sv = tthip.terrain_bounce_host(t, hm, ter, N, 0, TC.FAR, W, H, frames=frames, max_bounce=MAXB)
        # the same through the batched decode: PixelIndex p + W H at frames - 1 is pixel p of frame 1
        shifted = ter.copy()
        shifted["PixelIndex"][:N] += N
        out2, sv2 = tthip.terrain_bounce_host(t, hm, shifted, N, 0, TC.FAR, W, 2 * H, frames=frames - 1,
                                              max_bounce=MAXB, frame_pixels=N)
        assert np.array_equal(sv, sv2)
        assert 0 < len(want) and (sv[hit] == 1).sum() == len(want)
        for i in np.nonzero(hit)[0]:
            assert (sv[i] == 1) == (i in want), i
            if sv[i] == 1:
                assert out["last_pdf"][i:i + 1].view(np.uint32)[0] == want[i]["last_pdf"].view(np.uint32), i
                assert out2["last_pdf"][i:i + 1].view(np.uint32)[0] == want[i]["last_pdf"].view(np.uint32), i
                assert out2["PixelIndex"][i] == i + N and out["PixelIndex"][i] == i
        assert (sv[~hit] == -1).all()


def test_origin_equals_the_oracles_on_a_horizontal_triangle():
    """The flat terrain's normal (0, -1, 0) flips to (0, 1, 0) for a downward ray; the Cornell floor's unsmoothed
    normal (axis-aligned edges, identity W2L) ends as (0, 1, 0) too. Both offset the same pos = dir * t + origin."""
    t, hm = _flat()
    tri = _floor_frame()
    ter, hit = _as_terrain(tri, N)
    tt = tri["hits"][:N, 2].view(np.float32)
    pos_y = tri["direction"][:N, 1] * tt + tri["origin"][:N, 1]
    floor = hit & (np.abs(pos_y + 1.0) < 1e-5)
    assert floor.sum() > 200
    want = _oracle_survivors(tri, 7)
    out, sv = tthip.terrain_bounce_host(t, hm, ter, N, 0, TC.FAR, W, H, frames=7, max_bounce=MAXB)
    checked = 0
    for i in np.nonzero(floor)[0]:
        if sv[i] == 1:
            assert np.array_equal(out["origin"][i].view(np.uint32), want[i]["origin"].view(np.uint32)), i
            checked += 1
    assert checked > 200


def test_direction_is_a_unit_vector_about_the_flipped_terrain_normal():
    """In the orthonormal frame direction . norm = omega_o.y = last_pdf * pi, and norm differs from the flipped
    terrain normal only by the 16:16 octahedral round trip (step 1 / 32767.5): 1e-4."""
    T, A = TC.terrains(), TC.atlas()
    n, off = TC.N_RANDOM, TC.RW * TC.RH
    rays = np.zeros(2 * off, tthip.RAY_DTYPE)
    rays[off:off + n] = TC.random_rays()
    tthip.terrain_trace_host(T, A, rays, n, 1, TC.FAR, TC.RW, TC.RH)
    rays["hits"][off + 5] = (3, 17, np.float32(2.5).view(np.uint32), 0)          # a triangle record
    bad = off + int(np.nonzero(rays["hits"][off:off + n, 0] == TID)[0][0])
    rays["hits"][bad, 1] = len(T)                                                # triangle_id >= n: malformed
    out, sv = tthip.terrain_bounce_host(T, A, rays, n, 1, TC.FAR, TC.RW, TC.RH, frames=2, max_bounce=MAXB)
    win = rays[off:off + n]
    ter = win["hits"][:, 0] == TID
    assert np.array_equal(sv >= 0, ter) and sv[5] == -1 and sv[bad - off] == 0
    assert (sv[win["hits"][:, 2].view(np.float32) >= TC.FAR] == -1).all()        # misses
    live = np.nonzero(sv == 1)[0]
    assert len(live) > 1000 and (sv == 0).sum() >= 1
    assert (win["hits"][live, 1] == 1).any() and (win["hits"][live, 1] == 0).any()
    assert np.array_equal(out["hits"][live], win["hits"][live]), "hits are copied"
    assert np.array_equal(out["PixelIndex"][live], win["PixelIndex"][live])
    t = win["hits"][:, 2].view(np.float32)
    pos = win["direction"] * t[:, None] + win["origin"]
    flipped = 0
    for i in live[:: max(1, len(live) // 500)]:
        nn = tthip.terrain_normal_host(T, A, pos[i], int(win["hits"][i, 1])).astype(np.float64)
        d_in = win["direction"][i].astype(np.float64)
        if np.dot(d_in, nn) > 0:
            nn = -nn
            flipped += 1
        d = out["direction"][i].astype(np.float64)
        assert abs(np.linalg.norm(d) - 1.0) <= 1e-6, i
        assert abs(np.dot(d, nn) - float(out["last_pdf"][i]) * np.pi) <= 1e-4, i
        # (one float32 rounding of a coordinate below 16: half an ulp, 9.6e-7)
        assert np.abs(out["origin"][i].astype(np.float64) - (pos[i] + 1e-4 * nn)).max() <= 2e-6, i
    assert flipped > 50, "the reference's normal points down: rays from above flip it"


def test_entry_points_are_exported_and_the_flag_is_bit_8():
    L, S = tthip.hip_lib(), tthip.scene_lib()
    for name in ["tt_trace_heightmap_hits", "tt_group_scene_upload_terrains"]:
        assert hasattr(L, name), name
    assert hasattr(S, "tt_terrain_bounce_host")
    assert int(re.search(r"TT_ENQUEUE_TERRAIN_BOUNCE\s*=\s*1u\s*<<\s*(\d+)", HDR).group(1)) == 8
    assert tthip.TT_ENQUEUE_TERRAIN_BOUNCE == 1 << 8
    trace_bits = [int(b) for b in re.findall(r"TT_TRACE_\w+\s*=\s*1u\s*<<\s*(\d+)", HDR)]
    assert 8 not in trace_bits and len(set(trace_bits)) == len(trace_bits)
    for m in ["trace_heightmap_hits", "enqueue_bounce", "enqueue_bounce_indirect"]:
        assert hasattr(tthip.Engine, m)
    assert hasattr(tthip.Group, "upload_terrains")


def test_bounce_reference_under_sanitizers(tmp_path):
    """A stand-alone program (its own main, no Python in the run) built with ASan + UBSan together with
    host/tt_terrain.cpp."""
    exe = tmp_path / "terrain_bounce_kat"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(HERE, "native", "terrain_bounce_kat_main.cpp"),
                    os.path.join(REPO, "truetrace-unity-pathtracer_amd", "host", "tt_terrain.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout and "runtime error" not in r.stderr
