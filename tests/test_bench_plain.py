"""bench.py's plain run (no --full): setup, warm-up, the timed steps and the JSON line, nothing beside the
headline; and --dump-outputs, the last timed step's records as float64 .npy files that repeat from run to run.
A small frame of the bench's own scene (the legs and the files do not depend on the frame size): one bench process
per module, one more for the repeat."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
W, H, STEPS = 256, 128, 2
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--width", str(W), "--height", str(H)]
NAMES = ("primary_hits", "bounce_hits", "primary_info", "bounce_info", "counts")


def _run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, BENCH] + ARGS + ["--dump-outputs", str(out_dir)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    (line,) = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    return line, {n: np.load(os.path.join(str(out_dir), n + ".npy")) for n in NAMES}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump_a")
    line, arrays = _run(d)
    return d, line, arrays


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone(plain):
    _, d, _ = plain
    assert d["full"] is False and d["n_gpus"] == 1 and d["steps"] == STEPS and d["warmup"] == 1
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["metric"].startswith("Mrays/sec") and d["value"] > 0 and d["ms_per_step"] > 0
    c = d["config"]
    # value = the timed steps' rays / their time; ms_per_step = that time / steps (both rounded in the line)
    assert abs(d["value"] - c["rays_per_step_all_ranks"] / d["ms_per_step"] / 1e3) <= 0.01 * d["value"]
    assert c["primary_rays"] == c["frames_per_step"] * W * H
    for key in ("cpu_baseline", "oracle_check", "oracle_identical", "interactive"):
        assert d[key] is None, key
    for key in ("steady_state", "gather_identical_to_1gpu", "aux_recur_unjittered", "aux_shadow_nee",
                "aux_ray_producers", "aux_configs", "aux_group_tiles", "aux_strong_tiles", "aux_c5_tiles"):
        assert c[key] is None, key
    assert d["roofline"]["single_stream"] is None


@pytest.mark.gpu
def test_dump_outputs_are_the_last_steps_records(plain):
    out_dir, d, a = plain
    c = d["config"]
    assert sorted(os.listdir(str(out_dir))) == sorted(n + ".npy" for n in NAMES)
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(os.path.getsize(os.path.join(str(out_dir), n + ".npy")) for n in NAMES) <= 64 << 20
    n_prim, n_bnc = (int(v) for v in a["counts"])
    assert n_prim == c["primary_rays"] and 0 < n_bnc <= n_prim
    assert a["primary_hits"].shape == (min(n_prim, 200_000), 5) and a["bounce_hits"].shape == (min(n_bnc, 200_000), 5)
    assert a["primary_info"].shape == a["bounce_info"].shape == (min(n_prim, 200_000), 4)
    for h in (a["primary_hits"], a["bounce_hits"]):
        hit = h[:, 1] >= 0
        assert hit.any() and np.all((h[hit, 2] > 0) & (h[hit, 2] < 1000.0))  # t of a hit: inside (0, far)
        assert np.all((h[:, 3:5] >= 0) & (h[:, 3:5] <= 1))


@pytest.mark.gpu
def test_dump_outputs_repeat_with_the_same_arguments(plain, tmp_path):
    _, d, a = plain
    d2, b = _run(tmp_path / "dump_b")
    assert d2["config"]["primary_rays"] == d["config"]["primary_rays"]
    assert d2["config"]["bounce_rays"] == d["config"]["bounce_rays"]
    for n in NAMES:
        assert np.array_equal(a[n], b[n], equal_nan=True), n
