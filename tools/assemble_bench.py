#!/usr/bin/env python3
"""Times the scene-change path: loading a whole scene from the host (tt_scene_upload, the only path before
GPU-resident objects existed) beside creating the objects once (tt_object_create) and assembling the scene on
the device (tt_scene_assemble_objects) in both forms of the gather -- the batched kernel and per-object
device-to-device copies (TT_ASSEMBLE_FORM=memcpy, read at every call, so both run in this one process).

Configs: C4 (601 objects: the street plane + 600 instance parents under 2,401 mesh records) and C5 (one
10 M-triangle object). Per repeat the four calls run in turn (the two forms in alternating order), so drift hits
all alike. Wall-clock times of the calls, which all return synchronized: they include the host's validation and
bookkeeping, which is the point of the comparison. "gather_ms" is the GPU time of the gather alone (HIP events,
tt_timing_read); bytes read + written over it gives the copy rate, reported as a fraction of the 6.29 TB/s a
float4 copy reaches on this part.

    python tools/assemble_bench.py [--out profiles/r09/assemble/bench.json] [--configs c4,c5] [--reps 7]

(--configs c4small: a 25-object cut of C4, seconds to build, for checking the tool itself.)
"""
import argparse
import hashlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "truetrace-unity-pathtracer_amd", "python"))

COPY_RATE_TBS = 6.29  # measured float4 copy rate of the MI355X's HBM


def stat(v, digits=3):
    import numpy as np

    return {"median": round(float(np.median(v)), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def run(name, am, s, warmup, reps):
    import tthip

    arrays = [b.arrays() for b in am.blases()]  # what a host holds per ParentObject
    region = 2 * len(s.meshdata)
    tlas_nodes = s.nodes[:region].copy()
    eng = tthip.Engine(0)
    ms = {"upload": [], "create_all": [], "assemble_kernel": [], "assemble_memcpy": []}
    gather = {"kernel": [], "memcpy": []}
    sha = {}

    def digest():
        return hashlib.sha1(eng.scene_nodes(0, len(s.nodes)).tobytes() + eng.scene_tris(0, len(s.tris)).tobytes()).hexdigest()

    for it in range(warmup + reps):
        t0 = time.perf_counter()
        eng.upload(s)
        t1 = time.perf_counter()
        if it == 0:
            sha["upload"] = digest()
        t2 = time.perf_counter()
        objects = [eng.create_object(a) for a in arrays]
        t3 = time.perf_counter()
        took = {"upload": t1 - t0, "create_all": t3 - t2}
        for form in (("kernel", "memcpy") if it % 2 == 0 else ("memcpy", "kernel")):
            os.environ["TT_ASSEMBLE_FORM"] = form
            eng.timing_reset()
            t4 = time.perf_counter()
            eng.assemble(objects, tlas_nodes, s.tlas, s.meshdata, s.materials)
            took["assemble_" + form] = time.perf_counter() - t4
            g = float(eng.timing_read()[-1])
            if it == 0:
                sha[form] = digest()
            if it >= warmup:
                gather[form].append(g)
        for o in objects:
            o.destroy()
        if it >= warmup:
            for k, v in took.items():
                ms[k].append(v * 1e3)
    os.environ.pop("TT_ASSEMBLE_FORM", None)
    eng.close()
    n_obj_nodes = len(s.nodes) - region
    moved = 2 * (80 * n_obj_nodes + (88 + 48) * len(s.tris))  # read + written by the gather
    out = {"objects": len(arrays), "mesh_records": int(len(s.meshdata)), "nodes": int(len(s.nodes)), "tris": int(len(s.tris)),
           "host_bytes_uploaded": int(s.nodes.nbytes + s.tris.nbytes + 48 * len(s.tris)),
           "gather_bytes_read_plus_written": int(moved), "identical_to_upload": sha["kernel"] == sha["memcpy"] == sha["upload"],
           "ms": {k: stat(v) for k, v in ms.items()},
           "gather_ms": {k: stat(v, 4) for k, v in gather.items()}}
    for k in gather:
        rate = moved / (out["gather_ms"][k]["median"] * 1e-3) / 1e12
        out["gather_ms"][k].update(tb_per_s=round(rate, 3), fraction_of_float4_copy=round(rate / COPY_RATE_TBS, 3))
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r09", "assemble", "bench.json"))
    ap.add_argument("--configs", default="c4,c5")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch  # noqa: F401  (binds the HIP runtime first)

    import ttconfigs

    doc = {"reps": args.reps, "warmup": args.warmup, "float4_copy_tb_per_s": COPY_RATE_TBS, "configs": {}}
    for cfg in args.configs.split(","):
        t = time.perf_counter()
        am, s = {"c4": ttconfigs.c4_bistro_manager, "c5": ttconfigs.c5_san_miguel_manager,
                 "c4small": lambda: ttconfigs.c4_bistro_manager(n_unique=24, n_instances=96, max_tris=4000)}[cfg]()
        print(f"{cfg}: built in {time.perf_counter() - t:.1f} s", flush=True)
        doc["configs"][cfg] = run(cfg, am, s, args.warmup, args.reps)
        del am, s
    if "c4" in doc["configs"]:
        k, m = (doc["configs"]["c4"]["ms"][f] for f in ("assemble_kernel", "assemble_memcpy"))
        overlap = k["min"] <= m["max"] and m["min"] <= k["max"]
        doc["default_form"] = "kernel" if overlap or k["median"] <= m["median"] else "memcpy"
        doc["default_rule"] = "the lower C4 median of the assembly call; the kernel when the two ranges overlap"
        doc["c4_ranges_overlap"] = overlap
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    ok = all(c["identical_to_upload"] for c in doc["configs"].values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
