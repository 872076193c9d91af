#!/usr/bin/env python3
"""Times the two heightmap passes (tt_trace_heightmap, tt_trace_shadow_heightmap) beside the triangle trace
of the same launch, in both kernel forms: the one-thread-per-ray grid kernels (the product) and the persistent
refill kernels (TT_TERRAIN_FORM=persistent, read once per process, so each form runs in a child process of its own).

Scene: C2 (the Sponza-shaped hall) at 1920x1080 plus one 1,025 x 1,025 terrain under it, whose box -- as tall as
it is wide, like every Unity terrain's -- encloses the hall. Passes: the closest-hit pass over the primary rays
right after tt_trace_closest, the shadow pass over one NEE ray per pixel (from the primary hit point towards
a sun), and -- the hall is closed, so its triangle hits end every march after a few steps -- the closest-hit pass
once more over the untraced primary rays ("heightmap_open": what an open terrain costs). Times are HIP-event
durations of the calls (tt_timing_read), median of --reps after --warmup.

    python tools/terrain_bench.py [--out profiles/r08/terrain/bench.json]

The enqueue leg (--enqueue) times, on the same workload, the bounce enqueue without and with
TT_ENQUEUE_TERRAIN_BOUNCE after trace + heightmap, and tt_trace_heightmap beside tt_trace_heightmap_hits; with
--parent-lib (the previous commit's libtruetrace_hip.so) the two libraries run alternately, one child process per
run, --runs runs each, and the record holds the median of the runs' medians with their min - max.

    python tools/terrain_bench.py --enqueue --parent-lib PATH [--out profiles/r16/terrain_bounce/bench.json]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "truetrace-unity-pathtracer_amd", "python"))


def child(args):
    import numpy as np
    import torch

    import ttconfigs
    import tthip

    W, H = args.width, args.height
    n = W * H
    scene = ttconfigs.c2_sponza()
    terr = np.zeros(1, tthip.TERRAIN_DTYPE)
    terr[0]["PositionOffset"] = (-60.0, -4.0, -60.0)
    terr[0]["HeightScale"] = 1.5
    terr[0]["TerrainDim"] = (120.0, 120.0)
    terr[0]["HeightMap"] = (1.0, 1.0, 0.0, 0.0)
    hmap = tthip.synthetic_heightmap(0x7E44B0, 1025, 1025)
    eng = tthip.Engine(0)
    eng.upload(scene)
    eng.upload_terrains(terr, hmap)
    c2w, ip = ttconfigs.C2_VIEW.camera(W, H)
    rays0 = torch.zeros(2 * n * 48, dtype=torch.uint8, device="cuda:0")
    eng.generate(rays0, c2w, ip, W, H, ttconfigs.NEAR, ttconfigs.FAR, device=True)
    rays = rays0.clone()
    # the shadow rays: from each primary hit (after the terrain pass) towards a sun, 200 units
    eng.trace(rays, n, 0, ttconfigs.FAR, W, H, device=True)
    eng.trace_heightmap(rays, n, 0, ttconfigs.FAR, W, H, device=True)
    r = rays.cpu().numpy().view(tthip.RAY_DTYPE)[:n]
    closed_sha1 = hashlib.sha1(rays.cpu().numpy().tobytes()).hexdigest()
    t = r["hits"][:, 2].view(np.float32)
    sun = np.float32([0.35, 0.8, 0.48])
    sun /= np.linalg.norm(sun)
    s = np.zeros(n, tthip.SHADOW_DTYPE)
    s["origin"] = r["origin"] + r["direction"] * (np.minimum(t, 200.0) - 1e-3)[:, None]
    s["direction"] = sun
    s["t"] = 200.0
    s["illumination"] = 1.0
    s["PixelIndex"] = np.arange(n)
    srays = torch.from_numpy(s.view(np.uint8).reshape(-1)).to("cuda:0")
    colors = torch.zeros(n * 64, dtype=torch.uint8, device="cuda:0")
    nee = torch.zeros(n * 4, dtype=torch.float32, device="cuda:0")
    vis = torch.zeros(n * 4, dtype=torch.float32, device="cuda:0")
    ms = {"trace_closest": [], "heightmap": [], "shadow_heightmap": [], "heightmap_open": []}
    for it in range(args.warmup + args.reps):
        rays.copy_(rays0)
        colors.zero_()
        torch.cuda.synchronize()
        eng.timing_reset()
        eng.trace(rays, n, 0, ttconfigs.FAR, W, H, device=True)
        eng.trace_heightmap(rays, n, 0, ttconfigs.FAR, W, H, device=True)
        eng.shadow_heightmap(srays, n, 0, W, H, visibility=vis, colors=colors, nee_pos=nee, device=True)
        rays.copy_(rays0)  # the same rays with no triangle hit to cull them: an open terrain's long, uneven marches
        eng.trace_heightmap(rays, n, 0, ttconfigs.FAR, W, H, device=True)
        got = eng.timing_read()
        assert len(got) == 4, got
        if it >= args.warmup:
            for k, v in zip(ms, got):
                ms[k].append(float(v))
    st = eng.trace_heightmap(rays0.clone(), n, 0, ttconfigs.FAR, W, H, device=True, stats=True)
    h = r["hits"]
    out = {"form": args.form, "rays": n,
           "terrain_hits": int((h[:, 0] == tthip.TT_TERRAIN_MESH_ID).sum()),
           "occluded": int((vis.cpu().numpy().reshape(n, 4)[:, 3] == 0).sum()),
           "records_sha1": closed_sha1, "open_terrain_hits": int((rays.cpu().numpy().view(tthip.RAY_DTYPE)["hits"][:n, 0]
                                                                 == tthip.TT_TERRAIN_MESH_ID).sum()),
           "open_records_sha1": hashlib.sha1(rays.cpu().numpy().tobytes()).hexdigest(),
           "outputs_sha1": hashlib.sha1(vis.cpu().numpy().tobytes() + colors.cpu().numpy().tobytes()).hexdigest(),
           "samples_on_untraced_records": int(st.node_visits)}
    for k, v in ms.items():
        m = float(np.median(v))
        out[k] = {"ms": round(m, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "mrays_per_s": round(n / m / 1e3, 1)}
    eng.close()
    print("RESULT " + json.dumps(out))


def enqueue_child(args):
    """One run of the enqueue leg on the library TT_HIP_LIB names (default: this tree's)."""
    import numpy as np
    import torch

    import ttconfigs
    import tthip

    W, H = args.width, args.height
    n = W * H
    scene = ttconfigs.c2_sponza()
    terr = np.zeros(1, tthip.TERRAIN_DTYPE)
    terr[0]["PositionOffset"] = (-60.0, -4.0, -60.0)
    terr[0]["HeightScale"] = 1.5
    terr[0]["TerrainDim"] = (120.0, 120.0)
    terr[0]["HeightMap"] = (1.0, 1.0, 0.0, 0.0)
    hmap = tthip.synthetic_heightmap(0x7E44B0, 1025, 1025)
    eng = tthip.Engine(0)
    eng.upload(scene)
    eng.upload_terrains(terr, hmap)
    new = hasattr(eng.L, "tt_trace_heightmap_hits")  # (the parent library has neither new form)
    c2w, ip = ttconfigs.C2_VIEW.camera(W, H)
    far = ttconfigs.FAR
    rays = torch.zeros(2 * n * 48, dtype=torch.uint8, device="cuda:0")
    eng.generate(rays, c2w, ip, W, H, ttconfigs.NEAR, far, device=True)
    eng.trace(rays, n, 0, far, W, H, device=True)
    traced = rays.clone()      # after kernel_trace
    eng.trace_heightmap(rays, n, 0, far, W, H, device=True)
    marched = rays.clone()     # after kernel_heightmap
    # the hall is closed, so almost no primary ray reaches the terrain: the untraced rays marched alone give the
    # records of an open terrain, where the flagged enqueue has terrain rows to bounce
    eng.generate(rays, c2w, ip, W, H, ttconfigs.NEAR, far, device=True)
    eng.trace_heightmap(rays, n, 0, far, W, H, device=True)
    open_marched = rays.clone()
    hits = torch.zeros(n * 4, dtype=torch.int32, device="cuda:0")
    count = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    # two timed loops, so that the legs both libraries have run in the same sequence on either side
    common = ["enqueue", "heightmap"]
    added = ["enqueue_terrain_bounce", "heightmap_beside_hits", "heightmap_hits", "enqueue_open_unflagged",
             "enqueue_open_terrain_bounce"] if new else []
    ms = {k: [] for k in common + added}
    survivors = {}
    for names in (common, added):
        for it in range((args.warmup + args.reps) if names else 0):
            flagged = names is added
            rays.copy_(marched)
            torch.cuda.synchronize()
            eng.timing_reset()
            eng.enqueue_bounce_indirect(rays, None, n, count, 0, far, W, H, frames=1, max_bounce=3,
                                        **({"terrain_bounce": True} if flagged else {}))
            eng.sync()
            survivors[names[0]] = int(count.item())
            rays.copy_(traced)
            eng.trace_heightmap(rays, n, 0, far, W, H, device=True, asynchronous=True)
            if flagged:
                rays.copy_(traced)
                eng.trace_heightmap_hits(rays, hits, n, 0, far, W, H, asynchronous=True)
                for k, kw in (("enqueue_open_unflagged", {}), ("enqueue_open_terrain_bounce", {"terrain_bounce": True})):
                    rays.copy_(open_marched)
                    eng.enqueue_bounce_indirect(rays, None, n, count, 0, far, W, H, frames=1, max_bounce=3, **kw)
                    eng.sync()
                    survivors[k] = int(count.item())
            eng.sync()
            got = eng.timing_read()
            assert len(got) == len(names), got
            if it >= args.warmup:
                for k, v in zip(names, got):
                    ms[k].append(float(v))
    h = marched.cpu().numpy().view(tthip.RAY_DTYPE)["hits"][:n]
    out = {"rays": n, "terrain_hits": int((h[:, 0] == tthip.TT_TERRAIN_MESH_ID).sum()), "survivors": survivors,
           "records_sha1": hashlib.sha1(marched.cpu().numpy().tobytes()).hexdigest()}
    for k, v in ms.items():
        out[k] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    eng.close()
    print("RESULT " + json.dumps(out))


def enqueue_main(args):
    sides = (["parent"] if args.parent_lib else []) + ["new"]
    runs = {k: [] for k in sides}
    for _ in range(args.runs):  # alternated: parent, new, parent, new, ...
        for side in sides:
            env = dict(os.environ)
            env.pop("TT_HIP_LIB", None)
            if side == "parent":
                env["TT_HIP_LIB"] = os.path.abspath(args.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--enqueue-child", "--width", str(args.width), "--height",
                   str(args.height), "--warmup", str(args.warmup), "--reps", str(args.reps)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                return p.returncode
            runs[side].append(json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:]))
            sys.stderr.write(f"{side}: enqueue {runs[side][-1]['enqueue']['ms']} ms, heightmap "
                             f"{runs[side][-1]['heightmap']['ms']} ms\n")
            sys.stderr.flush()
    import statistics

    summary = {}
    for side, rs in runs.items():
        summary[side] = {}
        for k in ("enqueue", "heightmap", "enqueue_terrain_bounce", "heightmap_beside_hits", "heightmap_hits",
                  "enqueue_open_unflagged", "enqueue_open_terrain_bounce"):
            v = [r[k]["ms"] for r in rs if k in r]
            if v:
                summary[side][k] = {"median_ms": round(statistics.median(v), 4), "min_ms": min(v), "max_ms": max(v)}
    doc = {"scene": "C2 (262,267 tris) + one 1025x1025 terrain, 120 x 120 units, under the hall",
           "screen": [args.width, args.height], "reps": args.reps, "runs_per_side": args.runs,
           "what": "medians over the runs of each run's median; min - max over the runs", "summary": summary,
           "runs": runs,
           "records_identical": len({r["records_sha1"] for rs in runs.values() for r in rs}) == 1}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"summary": summary, "records_identical": doc["records_identical"]}, indent=1))
    return 0 if doc["records_identical"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r08", "terrain", "bench.json"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--form", choices=["persistent", "grid"], help="(child) run one form and print its result")
    ap.add_argument("--enqueue", action="store_true", help="the enqueue leg (see the module text)")
    ap.add_argument("--enqueue-child", action="store_true", help="(child) one run of the enqueue leg")
    ap.add_argument("--parent-lib", help="the previous commit's libtruetrace_hip.so, run alternately with this tree's")
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    if args.enqueue_child:
        return enqueue_child(args)
    if args.enqueue:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(REPO, "profiles", "r16", "terrain_bounce", "bench.json")
        return enqueue_main(args)
    if args.form:
        return child(args)
    res = {}
    for form in ("persistent", "grid", "persistent", "grid"):  # alternated: two runs of each
        env = dict(os.environ)
        env.pop("TT_TERRAIN_FORM", None)
        if form == "persistent":
            env["TT_TERRAIN_FORM"] = "persistent"
        cmd = [sys.executable, os.path.abspath(__file__), "--form", form, "--width", str(args.width), "--height",
               str(args.height), "--warmup", str(args.warmup), "--reps", str(args.reps)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            return p.returncode
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
        res.setdefault(form, []).append(json.loads(line[7:]))
    a, b = res["persistent"][0], res["grid"][0]
    doc = {"scene": "C2 (262,267 tris) + one 1025x1025 terrain, 120 x 120 units, under the hall", "screen":
           [args.width, args.height], "reps": args.reps, "runs": res,
           "forms_identical": all(a[k] == b[k] for k in ("records_sha1", "open_records_sha1", "outputs_sha1"))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))
    return 0 if doc["forms_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
