"""The float64 producer model (tests/producers.py) on what tt_generate_kernel, tt_resolve_kernel (triangle branch) and
tt_bounce_kernel<false> leave in memory, through the C ABI, with no oracle in between: the comparisons and cases of
tests/producers_cases.py that tests/test_producers_host.py runs on the oracle.

Worst values on an MI355X, as fractions of the derived bounds (pytest -s prints them):
  Generate, 40 cases                  direction 0.10, origin 0.15 (0.33 on the far camera of the traced chains)
  resolve                             smooth normal 0.09 (5.2e-7 absolute), unsmoothed 0.05 against the restated chain
                                      and against the world triangle, smooth against the analytic ellipsoid 0.72
  bounce, the indirect form included  |direction| - 1 0.63, last_pdf pi - omega_o.y 0.39, direction . norm - last_pdf pi
                                      0.13, direction . norm - disc sample 0.11, pair angle 0.05, origin offset 0.91
  KS at alpha = 0.001                 jitter x 0.46 and y 0.59 of the limit; cos^2 0.37 and azimuth 0.52
  look-back                           134,274 survivors of 266,241 in source order
  left open                           0 rays in every case beside the rays that are marginal by construction
Every figure equals the oracle's (tests/test_producers_host.py): the kernels are bit-identical to it.
"""
import numpy as np
import pytest

import producers as P
import producers_cases as PC
import tthip

pytestmark = pytest.mark.gpu
FAR = PC.FAR


class GpuSide:
    """The engine behind the interface of producers_cases; the scene is uploaded when a call names another one."""

    def __init__(self, engine):
        self.e, self.sc = engine, None

    def _scene(self, sc):
        if self.sc is not sc:
            self.e.upload(sc)
            self.sc = sc

    def generate(self, c2w, ip, W, H, near, far, jitter, frames, max_bounce):
        rays = np.zeros(2 * W * H, tthip.RAY_DTYPE)
        self.e.generate(rays, c2w, ip, W, H, near, far, jitter=jitter, frames=frames, max_bounce=max_bounce)
        return rays

    def trace(self, sc, buf, n, bounce, W, H):
        self._scene(sc)
        self.e.trace(buf, n, bounce, FAR, W, H)

    def resolve(self, sc, buf, n, bounce, W, H):
        self._scene(sc)
        return self.e.resolve_normals(buf, n, bounce, FAR, W, H)

    def enqueue(self, sc, buf, n, bounce, W, H, frames, max_bounce, frame_pixels):
        self._scene(sc)
        self.e.set_frame_pixels(frame_pixels)
        try:
            return self.e.enqueue_bounce(buf, n, bounce, FAR, W, H, frames=frames, max_bounce=max_bounce)
        finally:
            self.e.set_frame_pixels(0)


@pytest.fixture
def side(engine):
    return GpuSide(engine)


# ------------------------------------------------------------------ Generate
def test_generate_every_camera_size_and_parameter_set(side):
    worst = {}
    for cn, W, H, jit, fr, mb in PC.generate_cases():
        cam = PC.CAMERAS[cn]
        c2w, ip = PC.camera_matrices(cam, W, H)
        rays = side.generate(c2w, ip, W, H, cam.near, cam.far, jit, fr, mb)
        rep = PC.compare_generate(cam, W, H, jit, fr, mb, rays).check()
        for k, v in rep.worst.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"generate, {len(PC.generate_cases())} cases: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_jitter_is_uniform_over_the_footprint(side):
    cam = PC.CAMERAS["oblique"]
    W, H = 64, 65
    c2w, ip = PC.camera_matrices(cam, W, H)
    by = {fr: side.generate(c2w, ip, W, H, cam.near, cam.far, 1, fr, 5) for fr in (0, 3, 0x7FFFFFFF)}
    PC.compare_jitter(cam, W, H, by).check().say("jitter")


# ------------------------------------------------------------------ traced chains
@pytest.mark.parametrize("name", list(PC.TRACED))
def test_traced_chain(side, name):
    seen = {}
    for stage, rep in PC.traced_chain(side, name):
        rep.check().say(f"{name} {stage}")
        seen[stage] = rep
    assert seen["bounce 0"].counts["survivors"] > 300
    assert seen["bounce 1"].counts["survivors"] >= (0 if name == "far" else 30)


def test_the_mirrored_parent_is_traced_as_the_brute_force_does(side):
    import bruteforce as BF
    import bruteforce_cases as BFC

    sname, cam, W, H = PC.TRACED["near"]
    sc = PC.scene(sname)
    c2w, ip = PC.camera_matrices(cam, W, H)
    buf = side.generate(c2w, ip, W, H, cam.near, cam.far, 1, 3, 5)
    side.trace(sc, buf, W * H, 0, W, H)
    pick = np.arange(0, W * H, 5)
    ref = BF.closest(BF.Geometry.from_scene(sc), buf["origin"][pick], buf["direction"][pick], FAR)
    assert (ref.hit & (ref.mesh == PC.MIRRORED)).sum() >= 50
    BFC.compare_closest(ref, buf["hits"][pick]).check()


# ------------------------------------------------------------------ the normal resolve
def test_resolve_of_the_synthetic_records(side):
    """n no multiple of 256, the odd bounce's offset, and six zeros for misses, t >= far and out-of-range ids."""
    c = PC.resolve_case()
    sc = PC.scene(c.scene)
    buf, off, _ = PC.frame_buffer(c)
    n = len(c.src)
    assert n % 256 != 0 and c.bounce == 1 and off == c.W * c.H
    out = np.full((n, 6), 7.0, np.float32)
    side._scene(sc)
    side.e.resolve_normals(buf, n, c.bounce, FAR, c.W, c.H, out=out)
    rep = PC.compare_resolve(sc, c.src, out, True).check().say("resolve, synthetic")
    assert n - rep.counts["valid"] > 500


# ------------------------------------------------------------------ the synthetic enqueue cases
def test_coverage_case(side):
    c = PC.coverage_case()
    sc = PC.scene(c.scene)
    count, rows, rep = PC.run_enqueue(side, c)
    rep.check()
    m = P.bounce(sc.tris, sc.meshdata, c.src, FAR, c.bounce, c.frames, c.max_bounce)
    rep = PC.compare_bounce(c, count, rows, m).check().say("coverage")
    for k, least in PC.COVERAGE.items():
        assert rep.counts[k] >= least, (k, rep.counts)
    PC.compare_lobe(c, rows, m).check().say("lobe")


@pytest.mark.parametrize("name", PC.PATTERNS)
def test_survivor_patterns(side, name):
    c = PC.pattern_case(name)
    count, rows, rep = PC.run_enqueue(side, c)
    rep.check()
    rep = PC.compare_bounce(c, count, rows).check().say(name)
    assert rep.counts["survivors"] == count


def test_look_back_order(side):
    c = PC.lookback_case()
    count, rows, rep = PC.run_enqueue(side, c)
    rep.check()
    PC.compare_bounce(c, count, rows).check()
    assert 100_000 < count < 170_000
    print(f"look-back: {count} survivors of {len(c.src)} in source order")


def test_batched_frames(side):
    c = PC.batched_case()
    count, rows, rep = PC.run_enqueue(side, c)
    rep.check()
    PC.compare_bounce(c, count, rows).check().say("batched")
    assert (rows["PixelIndex"] >= c.frame_pixels).sum() > 500


def test_indirect_enqueue_with_the_count_on_the_device(side):
    """tt_enqueue_diffuse_bounce_indirect: the traced count (less than the capacity) and the survivor count stay on
    the device; the rays past the count are not enqueued."""
    import torch

    c = PC.coverage_case()
    sc = PC.scene(c.scene)
    n, k = len(c.src), 5000
    buf, off, dst = PC.frame_buffer(c)
    side._scene(sc)
    d = torch.from_numpy(buf.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    n_dev = torch.tensor([k], dtype=torch.int32, device="cuda:0")
    n_next = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    side.e.enqueue_bounce_indirect(d, n_dev, n, n_next, c.bounce, FAR, c.W, c.H, frames=c.frames, max_bounce=c.max_bounce)
    side.e.sync()
    count = int(n_next.item())
    out = d.cpu().numpy().view(tthip.RAY_DTYPE)
    head = PC.dataclasses.replace(c, src=c.src[:k], by_construction=c.by_construction[:k])
    PC.compare_bounce(head, count, out[dst:dst + count].copy()).check().say("indirect")
    assert np.array_equal(out[off:off + c.W * c.H], buf[off:off + c.W * c.H])
    assert np.array_equal(out[dst + count:dst + c.W * c.H], buf[dst + count:dst + c.W * c.H])
