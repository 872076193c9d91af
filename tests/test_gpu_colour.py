"""The float64 colour pin (tests/colour.py) on what the engine leaves: tt_trace_shadow_ex, tt_trace_shadow,
tt_trace_shadow_ex_indirect, tt_trace_shadow_heightmap and tt_trace_shadow_heightmap_indirect on the cases of
tests/colour_cases.py. Every report line must equal the host's (tests/test_colour_host.py prints the same lines from
the oracle and the terrain expectation): a differing figure is a finding."""
import os
import subprocess
import sys

import numpy as np
import pytest

import colour as CM
import colour_cases as CC
import terrain_cases as TC
import tthip

pytestmark = pytest.mark.gpu
RC, RG = tthip.TT_SHADOW_RADIANCE_CACHE, tthip.TT_TRACE_USE_RESTIRGI
SENTINEL = np.float32(-7.5)
COMBOS = [(b, f) for f in CC.FLAGS for b in (0, 1)]


@pytest.fixture(scope="module")
def engine():
    """An engine of this module's own: the glass soups leave their texture atlas on the context they are uploaded to,
    and tests of the session's shared engine rely on its having none."""
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    e = tthip.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def terrain_eng():
    if tthip.device_count() == 0:
        pytest.skip("no GPU visible")
    e = tthip.Engine(0)
    e.upload(TC.scene())
    e.upload_terrains(TC.terrains(), TC.atlas())
    yield e
    e.close()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def gpu_run(eng, case, bounce, flags, n=None, mode="host", with_vis=True, legacy=False):
    """One call on copies of the case's buffers; returns (vis, col, cache) as left. mode: host pointers, device
    pointers, or the indirect form with *n_rays_dev = n of a capacity of 4,096."""
    cap = 4096
    n = len(case.rays) if n is None else n
    rays = np.zeros(cap, tthip.SHADOW_DTYPE) if mode == "indirect" else case.rays.copy()
    rays[: len(case.rays)] = case.rays
    col, cache = case.col.copy(), case.cache.copy()
    vis = np.full((len(rays), 4), SENTINEL, np.float32)
    terrain = case.form == CM.TERRAIN
    kw = dict(visibility=vis if with_vis else None, colors=col)
    if not legacy:
        kw.update(cache=cache, flags=flags)
    if mode == "host":
        if terrain:
            eng.shadow_heightmap(rays, n, bounce, case.W, case.H, **kw)
        else:
            eng.trace_shadow(rays, n, bounce, case.W, case.H, legacy=legacy, **kw)
        return vis[: len(case.rays)], col, cache
    import torch

    d = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    d_rays = _dev(rays)
    if mode == "device":
        if terrain:
            eng.shadow_heightmap(d_rays, n, bounce, case.W, case.H, device=True, **d)
        else:
            eng.trace_shadow(d_rays, n, bounce, case.W, case.H, device=True, **d)
    else:
        n_dev = torch.tensor([n], dtype=torch.int32, device="cuda:0")
        if terrain:
            eng.shadow_heightmap(d_rays, cap, bounce, case.W, case.H, n_rays_dev=n_dev, **d)
        else:
            eng.trace_shadow_indirect(d_rays, n_dev, cap, bounce, case.W, case.H, **d)
    eng.sync()
    if with_vis:
        vis = _host(d["visibility"], vis)
    return vis[: len(case.rays)], _host(d["colors"], col), _host(d["cache"], cache)


def _same_as_host(case, bounce, flags, out, n=None, legacy=False):
    """The engine's report, which must carry no failure and read as the host's does."""
    rep = CC.check(case, *out, bounce, flags, n=n, legacy=legacy)
    print(f"{case.name} bounce {bounce} flags {flags:#x}: {rep.text}")
    assert not rep.fails, rep.fails
    h = CC.host_run(case, bounce, flags, n=n, legacy=legacy)
    want = CC.check(case, *h, bounce, flags, n=n, legacy=legacy)
    assert rep.text == want.text, (rep.text, want.text)
    return rep


# ------------------------------------------------------------------ any-hit
@pytest.mark.parametrize("bounce,flags", COMBOS)
def test_traced_case(engine, bounce, flags):
    case = CC.traced(bounce, flags)
    engine.upload(case.scene)
    rep = _same_as_host(case, bounce, flags, gpu_run(engine, case, bounce, flags))
    assert rep.reached > 200


@pytest.mark.parametrize("bounce", [0, 1])
def test_legacy_entry_leaves_the_rest_to_its_caller(engine, bounce):
    case = CC.traced(bounce, 0)
    engine.upload(case.scene)
    _same_as_host(case, bounce, 0, gpu_run(engine, case, bounce, 0, legacy=True), legacy=True)


@pytest.mark.parametrize("bounce,flags", COMBOS)
def test_edge_table_every_launch_size(engine, bounce, flags):
    case = CC.edge_table(CM.ANY_HIT)
    engine.upload(case.scene)
    for n in CC.LAUNCH_SIZES:
        out = gpu_run(engine, case, bounce, flags, n=n)
        assert (out[0][:n] == 1).all() and (out[0][n:] == SENTINEL).all()
        _same_as_host(case, bounce, flags, out, n=n)


@pytest.mark.parametrize("bounce,flags", [(0, RC), (1, RC | RG), (1, 0)])
def test_edge_table_device_indirect_and_null_visibility(engine, bounce, flags):
    case = CC.edge_table(CM.ANY_HIT)
    engine.upload(case.scene)
    ref = gpu_run(engine, case, bounce, flags)
    dev = gpu_run(engine, case, bounce, flags, mode="device")
    for a, b in zip(ref, dev):
        assert np.array_equal(a, b)          # (the padding beyond W * H travels with device pointers)
    _same_as_host(case, bounce, flags, dev)
    ind = gpu_run(engine, case, bounce, flags, n=257, mode="indirect")
    assert (ind[0][257:] == SENTINEL).all()
    _same_as_host(case, bounce, flags, ind, n=257)
    for mode in ("host", "device"):
        blind = gpu_run(engine, case, bounce, flags, mode=mode, with_vis=False)
        assert np.array_equal(blind[1], ref[1]) and np.array_equal(blind[2], ref[2]), "visibility = NULL changes the colours"


def test_pinned_edge_words(engine, terrain_eng):
    """Non-finite and negative illumination: the words of tests/colour_cases.py's PINNED, exactly, in both forms."""
    case = CC.pinned_edges(CM.ANY_HIT)
    engine.upload(case.scene)
    CC.check_pinned(case, *gpu_run(engine, case, 0, RC))
    case = CC.pinned_edges(CM.TERRAIN)
    CC.check_pinned(case, *gpu_run(terrain_eng, case, 0, RC))


# ------------------------------------------------------------------ terrain
@pytest.mark.parametrize("bounce,flags", COMBOS)
@pytest.mark.parametrize("which", ["set", "edge"])
def test_terrain_form(terrain_eng, which, bounce, flags):
    case = CC.terrain_set() if which == "set" else CC.edge_table(CM.TERRAIN)
    out = gpu_run(terrain_eng, case, bounce, flags)
    rep = _same_as_host(case, bounce, flags, out)
    live = case.rays["t"] != 0
    assert (out[0][~live] == SENTINEL).all(), "the terrain form skips t == 0 (-0.0 too)"
    if which == "edge":
        assert (out[0][live] == 1).all()
    assert rep.reached > 200


@pytest.mark.parametrize("bounce,flags", [(0, RC), (1, RC | RG), (1, 0)])
def test_terrain_edge_table_sizes_device_indirect_and_null_visibility(terrain_eng, bounce, flags):
    case = CC.edge_table(CM.TERRAIN)
    for n in CC.LAUNCH_SIZES[:-1]:
        _same_as_host(case, bounce, flags, gpu_run(terrain_eng, case, bounce, flags, n=n), n=n)
    ref = gpu_run(terrain_eng, case, bounce, flags)
    dev = gpu_run(terrain_eng, case, bounce, flags, mode="device")
    for a, b in zip(ref, dev):
        assert np.array_equal(a, b)
    ind = gpu_run(terrain_eng, case, bounce, flags, n=257, mode="indirect")
    _same_as_host(case, bounce, flags, ind, n=257)
    for mode in ("host", "device"):
        blind = gpu_run(terrain_eng, case, bounce, flags, mode=mode, with_vis=False)
        assert np.array_equal(blind[1], ref[1]) and np.array_equal(blind[2], ref[2]), "visibility = NULL changes the colours"


def test_terrain_persistent_form(terrain_eng):
    """TT_TERRAIN_FORM is read once per process: a child runs both terrain cases on the persistent kernels and
    prints their report lines, which must be the default form's."""
    want = []
    for case in (CC.terrain_set(), CC.edge_table(CM.TERRAIN)):
        for bounce, flags in COMBOS:
            rep = CC.check(case, *gpu_run(terrain_eng, case, bounce, flags), bounce, flags)
            assert not rep.fails
            want.append(f"REPORT {case.name} bounce {bounce} flags {flags:#x}: {rep.text}")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "colour_form_child.py")
    r = subprocess.run([sys.executable, child], env=dict(os.environ, TT_TERRAIN_FORM="persistent"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [x for x in r.stdout.splitlines() if x.startswith("REPORT ")] == want
