#!/usr/bin/env python3
"""Times the NEE emit and the shadow trace of its rays beside the trace and the enqueue of the same frame.

Scene: C2 (the Sponza-shaped hall) at 1920x1080 with an 8 x 4 grid of emissive ceiling panels
(ttconfigs.c2_sponza_lights). Per repetition, for bounce 0 and bounce 1, on one context and one stream:
    tt_trace_closest(_indirect) -> tt_emit_nee_indirect -> tt_trace_shadow_ex_indirect on the emitted rays
    -> tt_enqueue_diffuse_bounce_indirect
and, for comparison, tt_trace_shadow on the point-light rays bench.py's aux_shadow_nee leg builds (every hit aimed at
one point, light = (0, 9, 0.5)). Times are the HIP-event durations of the calls (tt_timing_read), medians of --reps
repetitions after --warmup, with min and max. No time here is a threshold: the path is new.

    python tools/lights_bench.py [--out profiles/lights/bench.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "truetrace-unity-pathtracer_amd", "python"))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tris", type=int, default=0, help="triangles of the hall (0: C2's 262,267)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lights", "bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import ttconfigs
    import tthip

    W, H = args.width, args.height
    n = W * H
    scene, lights = ttconfigs.c2_sponza_lights(n_tris=args.tris or ttconfigs.C2_TRIS)
    eng = tthip.Engine(0)
    eng.upload(scene)
    eng.upload_lights(lights)
    c2w, ip = ttconfigs.C2_VIEW.camera(W, H)
    FAR, MB = ttconfigs.FAR, 3
    rays = torch.zeros(2 * n * 48, dtype=torch.uint8, device="cuda:0")
    sh = [torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    vis = torch.zeros(n * 4, dtype=torch.float32, device="cuda:0")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda:0")  # n1, shadow rays of bounce 0, of bounce 1
    names = ["trace_b0", "emit_nee_b0", "shadow_nee_b0", "enqueue_b0", "trace_b1", "emit_nee_b1", "shadow_nee_b1",
             "shadow_point_b0", "shadow_point_b1"]
    ms = {k: [] for k in names}
    counts = {}
    for it in range(args.warmup + args.reps):
        eng.generate(rays, c2w, ip, W, H, ttconfigs.NEAR, FAR, jitter=1, frames=it, max_bounce=MB, device=True)
        torch.cuda.synchronize()
        eng.timing_reset()
        eng.trace(rays, n, 0, FAR, W, H, device=True, asynchronous=True)
        eng.emit_nee_indirect(rays, None, n, cnt[1:2], 0, FAR, W, H, frames=it, max_bounce=MB, shadow_rays=sh[0])
        eng.trace_shadow_indirect(sh[0], cnt[1:2], n, 0, W, H, visibility=vis)
        eng.enqueue_bounce_indirect(rays, None, n, cnt[0:1], 0, FAR, W, H, frames=it, max_bounce=MB)
        eng.trace_indirect(rays, cnt[0:1], n, 1, FAR, W, H)
        eng.emit_nee_indirect(rays, cnt[0:1], n, cnt[2:3], 1, FAR, W, H, frames=it, max_bounce=MB, shadow_rays=sh[1])
        eng.trace_shadow_indirect(sh[1], cnt[2:3], n, 1, W, H, visibility=vis)
        eng.sync()
        c = cnt.cpu().numpy()
        n1 = int(c[0])
        # the point-light rays of bench.py's aux_shadow_nee leg, from the same records (setup, not timed)
        p0 = bench.nee_rays(torch, rays, n, FAR, (0.0, 9.0, 0.5))
        p1 = bench.nee_rays(torch, rays[n * 48:], n1, FAR, (0.0, 9.0, 0.5))
        torch.cuda.synchronize()
        eng.trace_shadow(p0, p0.numel() // 48, 0, W, H, visibility=vis, device=True, legacy=True)
        eng.trace_shadow(p1, p1.numel() // 48, 1, W, H, visibility=vis, device=True, legacy=True)
        got = eng.timing_read()
        assert len(got) == len(names), (len(got), names)
        if it >= args.warmup:
            for k, v in zip(names, got):
                ms[k].append(float(v))
            counts = {"rays_b0": n, "rays_b1": n1, "nee_rays_b0": int(c[1]), "nee_rays_b1": int(c[2]),
                      "point_rays_b0": p0.numel() // 48, "point_rays_b1": p1.numel() // 48}
    out = {"scene": "C2 + 8x4 ceiling panels", "width": W, "height": H, "light_triangles": int(len(lights.tris)),
           "light_nodes": int(len(lights.nodes)), "reps": args.reps, "warmup": args.warmup, "counts_last_rep": counts}
    for k, v in ms.items():
        out[k] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
