#!/usr/bin/env python3
"""Times tt_lights_refit against the route a host has without it.

Three sizes:
    L3        tests/lights_cases.py's 1,024-light-triangle grid, one light mesh: the mesh pass and the TLAS pass;
    grid64k   a synthetic 256 x 128 grid of quads, 65,536 light triangles, one light mesh: the mesh pass;
    props1k   1,024 instances of the 6-light-triangle prop: the TLAS pass.
Per size, medians of --reps calls after --warmup, with min and max:
    refit_ms        the HIP-event duration of the whole call (tt_timing_read: one entry per call);
    refit_wall_ms   host wall time of an asynchronous call followed by tt_sync;
the result is then compared, byte for byte, with tt_lights_refit_host;
and the route of today, where there is one:
    TLAS part   tt_light_bounds_transform per instance + tt_light_bvh_build_tlas on the CPU, then
                tt_scene_update_light_nodes (host wall time, the call synchronized). The bounds stage is one
                binding call per instance from a Python loop, mostly interpreter time, so it is reported apart
                from the build + update stage (two native calls), which is the figure to compare;
    mesh part   nothing: a deforming emissive mesh cannot be followed without the refit.
No time here is a threshold: nobody has measured this path before.

    python tools/lights_refit_bench.py [--out profiles/lights/refit_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "truetrace-unity-pathtracer_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lights", "refit_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch  # noqa: F401  (binds the HIP runtime first)

    import lights_cases as LC
    import tthip

    def grid_case(nx, nz):
        rng = np.random.default_rng(0x4C64)
        s = LC._Soup()
        s.quad((-8, 0, -4), (0, 0, 8), (16, 0, 0))
        gx, gz = np.meshgrid(np.arange(nx + 1), np.arange(nz + 1), indexing="ij")
        vx = -8 + (16.0 / nx) * gx + rng.uniform(-0.01, 0.01, gx.shape)
        vz = -4 + (8.0 / nz) * gz + rng.uniform(-0.01, 0.01, gz.shape)
        vy = 4 + rng.uniform(-0.05, 0.05, gx.shape)
        P = lambda i, j: (vx[i, j], vy[i, j], vz[i, j])  # noqa: E731
        for i in range(nx):
            for j in range(nz):
                s.tri(P(i, j), P(i + 1, j), P(i + 1, j + 1), LC.EMISSIVE)
                s.tri(P(i, j), P(i + 1, j + 1), P(i, j + 1), LC.EMISSIVE)
        am = tthip.AssetManager()
        am.add_parent(tthip.Blas(s.mesh()), None, np.zeros(2, tthip.MAT_DTYPE))
        return LC._assemble("grid", am, [np.eye(4)], ((0.0, 1.5, 6.0), (0.0, -0.1, -1.0), 70.0))

    def props_case(n):
        rng = np.random.default_rng(0x4C65)
        s = LC._Soup()
        s.quad((-40, 0, -40), (0, 0, 80), (80, 0, 0))
        am = tthip.AssetManager()
        mats = np.zeros(2, tthip.MAT_DTYPE)
        am.add_parent(tthip.Blas(s.mesh()), None, mats)
        ip = am.add_instance_parent(tthip.Blas(LC._prop_mesh()), mats)
        l2w = [np.eye(4)]
        for _ in range(n):
            m = LC._trs(rng.uniform((-38, 1, -38), (38, 6, 38)), rng.uniform(-180, 180, 3), rng.uniform(0.5, 2.0, 3))
            am.add_instance(ip, m)
            l2w.append(m)
        return LC._assemble("props", am, l2w, ((0.0, 2.0, 0.0), (0.0, 0.0, -1.0), 70.0))

    def stat(v):
        return {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def run(name, case, mesh_pass, tlas_pass):
        eng = tthip.Engine(0)
        eng.upload(case.scene)
        eng.upload_lights(case.lights)
        md, lm = case.scene.meshdata, case.lights.meshes
        records = sorted({int(r) for r in lm["LockedMeshIndex"]}, key=lambda r: int(md["LightNodeOffset"][r]))
        records = [r for k, r in enumerate(records) if k == 0 or int(md["LightNodeOffset"][r]) != int(md["LightNodeOffset"][records[k - 1]])]
        mats = [np.asarray(m, np.float64) for _, _, m in case.instances]
        offs = [int(md["LightNodeOffset"][int(r)]) for r in lm["LockedMeshIndex"]]
        x = tthip.light_transforms(mats, offs) if tlas_pass else None
        xd = None if x is None else torch.from_numpy(x.view(np.uint8).copy()).cuda()
        dev_ms, wall_ms = [], []
        for it in range(args.warmup + args.reps):
            eng.sync()
            eng.timing_reset()
            t0 = time.perf_counter()
            eng.refit_lights(records if mesh_pass else [], xd, device=True, asynchronous=True)
            eng.sync()
            t1 = time.perf_counter()
            got = eng.timing_read()
            assert len(got) == 1, got
            if it >= args.warmup:
                dev_ms.append(float(got[0]))
                wall_ms.append((t1 - t0) * 1e3)
        # the timed calls' result against the scalar host reference (a refit is a pure function of its inputs)
        want = tthip.lights_refit_host(case.lights, case.scene, records if mesh_pass else [], x)
        same = (eng.read_light_nodes(0, len(want.nodes)).tobytes() == want.nodes.tobytes() and
                eng.read_light_tris(0, len(want.tris)).tobytes() == want.tris.tobytes())
        assert same, f"{name}: the device's nodes differ from tt_lights_refit_host"
        out = {"light_triangles": int(len(case.lights.tris)), "light_meshes": int(len(lm)), "light_nodes": int(len(case.lights.nodes)),
               "passes": [p for p, on in (("mesh", mesh_pass), ("tlas", tlas_pass)) if on],
               "refit_ms": stat(dev_ms), "refit_wall_ms": stat(wall_ms), "identical_to_host_reference": bool(same)}
        if tlas_pass:
            # today's route: the world bounds of every instance, the TLAS on the CPU, the copy of its nodes
            roots = {}
            for par, (lt, nr) in enumerate(case.parents):
                roots[par] = tthip.light_bvh_build_mesh(lt, nr)[1]
            bounds_ms, build_ms, host_ms = [], [], []
            for it in range(args.warmup + args.reps):
                eng.sync()
                t0 = time.perf_counter()
                world = np.concatenate([tthip.light_bounds_transform(roots[par], m) for par, _, m in case.instances])
                t1 = time.perf_counter()
                nodes = tthip.light_bvh_build_tlas(world)
                eng.update_light_nodes(0, nodes)
                eng.sync()
                t2 = time.perf_counter()
                if it >= args.warmup:
                    bounds_ms.append((t1 - t0) * 1e3)
                    build_ms.append((t2 - t1) * 1e3)
                    host_ms.append((t2 - t0) * 1e3)
            # the bounds stage is one binding call per instance from a Python loop: mostly interpreter time, which a
            # native host would not pay; the build + update stage is two native calls
            out["host_route_tlas_wall_ms"] = stat(host_ms)
            out["host_route_bounds_python_wall_ms"] = stat(bounds_ms)
            out["host_route_build_update_wall_ms"] = stat(build_ms)
        if mesh_pass:
            out["host_route_mesh"] = "none: a deforming emissive mesh cannot be followed without tt_lights_refit"
        eng.close()
        print(name, json.dumps(out), flush=True)
        return out

    out = {"reps": args.reps, "warmup": args.warmup,
           "L3": run("L3", LC.l3_deep(), True, True),
           "grid64k": run("grid64k", grid_case(256, 128), True, False),
           "props1k": run("props1k", props_case(1024), False, True)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
