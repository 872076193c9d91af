#!/usr/bin/env python3
"""BLAS build times, host vs the GPU stages (row f4's builder half: BVH2 only, BVH2 + BVH8), on the BASELINE meshes:
C2 Sponza-shaped (262k tris) and C5 San-Miguel-shaped (10M tris). Both builds must be byte-identical
(nodes, leaf-ordered triangles, leaf order). Usage: build_bench.py [--meshes c2,c5]
Prints one JSON document (commit under profiles/).

--leg object [--meshes c2,c5,c4] [--routes a,b,c] [--repeats 7] [--check] [--out FILE]: a mesh set to GPU-resident
objects, (a) Blas(mesh, engine=...) + Engine.create_object (host triangle records, four trips over the bus) against
(b) Engine.build_object per mesh (tt_object_build_device) and (c) one Engine.build_objects call over the set
(tt_objects_build_device); the chosen routes alternate, wall-clock to the synchronize, medians and ranges of the
repeats after one warm-up; (b)'s and (c)'s stage splits from the HIP-event entries of tt_timing_read
(host_walk_and_rest: the wall clock outside them -- the mesh upload, allocations, the host walk). c4 is
C4's object set: the street plane and 600 props. --check compares what (b) and (c) read back with the host build.
--routes b with TT_HIP_LIB naming another build of the library measures that build's per-object loop."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "truetrace-unity-pathtracer_amd", "python"))


COPY_TBS = 6.29  # the float4 copy rate of profiles/r09/assemble/bench.json, TB/s
STAGES = ("pass1_boxes", "presort", "bvh2_bvh8", "pass2_records", "mirror_copy")


def _stats(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def _mesh_set(tthip, name):
    if name == "c2":
        return [tthip.Mesh.sponza()]
    if name == "c5":
        return [tthip.Mesh.san_miguel()]
    import ttconfigs as T  # C4's object set, as c4_bistro_manager draws it

    rng = np.random.default_rng(T.C4_SEED)
    sizes = np.exp(rng.uniform(np.log(200), np.log(40000), 600)).astype(np.int64)
    return [tthip.Mesh.ground(-110.0, 110.0, -110.0, 110.0, 128, 128)] + [
        tthip.Mesh.prop(T._mix_seed(T.C4_SEED, k), int(sizes[k])) for k in range(600)]


def _pass2_bytes(view):
    """Bytes pass 2 needs per triangle: cwbvh_indices, three indices, three vertices' attributes, MatDat read;
    the 88-byte record, the 48-byte traversal record and leaf_of written."""
    per_vertex = 12 + (12 if view.normals else 0) + (16 if view.tangents else 0) + (8 if view.uvs else 0)
    return 4 + 12 + 3 * per_vertex + (4 if view.matdat else 0) + 136 + 4


def object_leg(tthip, eng, a):
    out = {"tool": "tools/build_bench.py --leg object", "repeats": a.repeats, "host_threads": os.cpu_count(),
           "float4_copy_TBs": COPY_TBS, "rows": []}
    for name in a.meshes.split(","):
        meshes = _mesh_set(tthip, name)
        tris = sum(m.view().n_indices // 3 for m in meshes)
        routes = a.routes.split(",")
        run = {"a": lambda: [eng.create_object(tthip.Blas(m, engine=eng)) for m in meshes],
               "b": lambda: [eng.build_object(m) for m in meshes],
               "c": lambda: eng.build_objects(meshes)}
        times = {r: [] for r in routes}
        on_host = {}
        for rep in range(a.repeats + 1):  # the first round warms up
            for r in routes:
                t0 = time.perf_counter()
                objs = run[r]()
                eng.sync()
                t1 = time.perf_counter()
                if r != "a":
                    on_host[r] = sum(o.build_info.presorted_on_host for o in objs)
                del objs
                if rep:
                    times[r].append((t1 - t0) * 1e3)
        row = {"set": name, "objects": len(meshes), "tris": tris, "routes": routes,
               "library": os.environ.get("TT_HIP_LIB", "this tree")}
        keys = {"a": "a_blas_then_create_object_ms", "b": "b_build_object_ms", "c": "c_build_objects_ms"}
        stats = {r: _stats(times[r]) for r in routes}
        for r in routes:
            row[keys[r]] = stats[r]
            row[r + "_runs_ms"] = [round(x, 3) for x in times[r]]
            if r in on_host:
                row[r + "_presorted_on_host"] = on_host[r]
        for x, y in (("a", "b"), ("b", "c")):
            if x in stats and y in stats:
                row[f"{y}_faster_than_{x}"] = stats[y]["max"] < stats[x]["min"]
                row[f"{x}_{y}_ranges_overlap"] = not (stats[y]["max"] < stats[x]["min"] or stats[x]["max"] < stats[y]["min"])
                row[f"{x}_over_{y}_medians"] = round(stats[x]["median"] / stats[y]["median"], 3)
        eng.set_timing(True)  # the stage splits: five HIP-event entries per object in (b), per call in (c)
        p2_bytes = sum(_pass2_bytes(m.view()) * (m.view().n_indices // 3) for m in meshes)
        row["pass2_bytes"] = p2_bytes
        for r in [r for r in routes if r != "a"]:
            split = []
            for _ in range(3):
                t0 = time.perf_counter()
                ms = []
                if r == "b":
                    for k in range(0, len(meshes), 50):  # the ring keeps 256 entries: read every 50 objects
                        eng.timing_reset()
                        objs = [eng.build_object(m) for m in meshes[k:k + 50]]
                        ms.append(eng.timing_read())
                        del objs
                else:
                    eng.timing_reset()
                    objs = eng.build_objects(meshes)
                    ms.append(eng.timing_read())
                    del objs
                wall = (time.perf_counter() - t0) * 1e3
                ms = np.concatenate(ms)
                assert len(ms) == 5 * (len(meshes) if r == "b" else 1), (len(ms), len(meshes))
                st = dict(zip(STAGES, ms.reshape(-1, 5).sum(0).tolist()))
                st["host_walk_and_rest"] = wall - sum(st.values())
                st["wall"] = wall
                split.append(st)
            stages = {k: round(float(np.median([s[k] for s in split])), 3) for k in split[0]}
            p2_tbs = p2_bytes / (stages["pass2_records"] * 1e-3) / 1e12
            row[r + "_stages_ms"] = stages
            row[r + "_pass2_TBs"] = round(p2_tbs, 3)
            row[r + "_pass2_share_of_float4_copy"] = round(p2_tbs / COPY_TBS, 3)
        eng.set_timing(False)
        if a.check:
            batch = eng.build_objects(meshes) if "c" in routes else [None] * len(meshes)
            same = {r: True for r in routes if r != "a"}
            for m, oc in zip(meshes, batch):
                host = tthip.Blas(m)
                hn, ht = host.arrays()
                for r, o in (("b", eng.build_object(m) if "b" in routes else None), ("c", oc)):
                    if o is None:
                        continue
                    n, t, l = o.read()
                    same[r] = same[r] and n.tobytes() == hn.tobytes() and t.tobytes() == ht.tobytes() and bool(
                        np.array_equal(l, host.leaf_order())) and o.build_info.bvh2_depth == host.info.bvh2_depth
                    o.destroy()
                del host
            for r, ok in same.items():
                row[r + "_identical_to_host_build"] = ok
        out["rows"].append(row)
        print(f"[object] {row}", file=sys.stderr, flush=True)
        del meshes
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="c2,c5")
    ap.add_argument("--leg", default="blas", choices=["blas", "object"])
    ap.add_argument("--routes", default="a,b,c", help="object leg: which of the routes a, b, c to run")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (binds the HIP runtime first)
    import tthip

    eng = tthip.Engine(0)
    if a.leg == "object":
        object_leg(tthip, eng, a)
        eng.close()
        return
    out = {"tool": "tools/build_bench.py", "host_threads": os.cpu_count(), "rows": []}
    for name in a.meshes.split(","):
        mesh = {"c2": tthip.Mesh.sponza, "c5": tthip.Mesh.san_miguel}[name]()
        t0 = time.perf_counter()
        host = tthip.Blas(mesh)
        t_host = time.perf_counter() - t0
        tim2 = {}
        t0 = time.perf_counter()
        dev2 = tthip.Blas(mesh, engine=eng, timings=tim2, device_stages="bvh2")
        t_dev2 = time.perf_counter() - t0
        same2 = dev2.arrays()[0].tobytes() == host.arrays()[0].tobytes()
        del dev2
        tim = {}
        t0 = time.perf_counter()
        dev = tthip.Blas(mesh, engine=eng, timings=tim)
        t_dev = time.perf_counter() - t0
        nh, th = host.arrays()
        nd, td = dev.arrays()
        same = (nh.tobytes() == nd.tobytes() and th.tobytes() == td.tobytes()
                and bool(np.array_equal(host.leaf_order(), dev.leaf_order())))
        row = {"mesh": name, "tris": host.n_tris, "cwbvh_nodes": host.n_nodes, "bvh2_depth": host.info.bvh2_depth,
               "host_build_s": round(t_host, 3),
               "device_bvh2_host_bvh8_s": round(t_dev2, 3), "device_bvh2_host_bvh8_stages_s": {k: round(v, 3) for k, v in tim2.items()},
               "device_bvh2_bvh8_s": round(t_dev, 3), "device_bvh2_bvh8_stages_s": {k: round(v, 3) for k, v in tim.items()},
               "identical": same and same2}
        out["rows"].append(row)
        print(f"[build] {row}", file=sys.stderr, flush=True)
        del host, dev
    eng.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
