#!/usr/bin/env python3
"""Times the three ways a TLAS topology is renewed, on C4 (2,401 mesh records) with its instances' positions
permuted among themselves, and what the renewal buys in trace time.

  (a) tt_tlas_rebuild: the device build + install; wall time of the call (it synchronizes) and its three
      tt_timing_read entries (presort, BVH2 + BVH8, install).
  (b) tt_tlas_build on the host + the asynchronous tt_scene_update_tlas: the host build's time, the host time of
      the install call (it returns before the GPU is done) and the install's device time.
  (c) the route there was before: tt_scene_assemble_tlas + tt_scene_assemble_objects, which copies every BLAS
      again, synchronizes the stream and is refused on a lender with borrowers.
  (d) the primary and bounce-1 launch times (1920x1080, C4's view) over the refit-only TLAS (the upload-time
      topology, boxes refit to the new pose) and over the rebuilt one; the records are checked to be identical.

One warm-up, then --reps repeats with (a), (b), (c) and the two halves of (d) in turn inside each repeat, so drift
hits all alike. Medians with min-max.

    python tools/tlas_rebuild_bench.py [--out profiles/r18/tlas_rebuild/bench.json] [--config c4|c4small] [--reps 7]

(--config c4small: a 97-record cut of C4, seconds to build, for checking the tool itself.)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "truetrace-unity-pathtracer_amd", "python"))


def stat(v, digits=4):
    import numpy as np

    return {"median": round(float(np.median(v)), digits), "min": round(float(min(v)), digits), "max": round(float(max(v)), digits)}


def tlas_side(am):
    """tt_scene_assemble_tlas over the manager's current matrices: (region nodes, TLASBVH8Indices, _MeshData, mesh
    AABBs, n_tlas_nodes) from the BLASes' summaries alone."""
    import numpy as np
    import tthip

    def desc(b, l2w, nm, d):
        d.n_nodes, d.n_tris = b.info.n_nodes, b.info.n_tris
        d.aabb_min[:], d.aabb_max[:] = b.info.aabb_min[:], b.info.aabb_max[:]
        d.local_to_world[:] = tthip.unity_colmajor(l2w)
        d.world_to_local[:] = tthip.unity_colmajor(np.linalg.inv(l2w))
        d.material_count = nm

    P = (tthip.ObjectDesc * max(1, len(am.parents)))()
    for i, (b, l2w, nm) in enumerate(am.parents):
        desc(b, l2w, nm, P[i])
    IP = (tthip.ObjectDesc * max(1, len(am.instance_parents)))()
    for i, (b, nm) in enumerate(am.instance_parents):
        desc(b, np.eye(4), nm, IP[i])
    I = am._instance_descs()
    h = C.c_void_p()
    L = tthip.scene_lib()
    t0 = time.perf_counter()
    st = L.tt_scene_assemble_tlas(C.addressof(P), len(am.parents), C.addressof(IP), len(am.instance_parents),
                                  C.addressof(I), len(am.instances), C.byref(h))
    took = time.perf_counter() - t0
    assert st == 0, st
    try:
        info = tthip.SceneBuildInfo()
        L.tt_scene_build_get_info(h, C.byref(info))
        nodes = np.zeros(info.n_nodes, tthip.NODE_DTYPE)
        tlas = np.zeros(info.n_tlas_indices, np.int32)
        md = np.zeros(info.n_mesh, tthip.MESH_DTYPE)
        L.tt_scene_build_copy(h, nodes.ctypes.data, None, tlas.ctypes.data, md.ctypes.data)
        boxes = np.zeros((info.n_mesh, 6), np.float32)
        L.tt_scene_build_copy_mesh_aabbs(h, boxes.ctypes.data)
    finally:
        L.tt_scene_build_free(h)
    return {"nodes": nodes, "tlas": tlas, "md": md, "boxes": boxes, "n": int(info.tlas_nodes), "host_s": took}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r18", "tlas_rebuild", "bench.json"))
    ap.add_argument("--config", default="c4")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch

    import ttconfigs
    import tthip

    t = time.perf_counter()
    am, s = (ttconfigs.c4_bistro_manager() if args.config == "c4"
             else ttconfigs.c4_bistro_manager(n_unique=24, n_instances=96, max_tris=4000))
    print(f"{args.config}: built in {time.perf_counter() - t:.1f} s", flush=True)
    mats = s.materials
    pose_a = tlas_side(am)
    assert pose_a["nodes"].tobytes() == s.nodes[:len(pose_a["nodes"])].tobytes()
    # the permuted pose: instance i keeps its prop, yaw and scale and stands where instance perm[i] stood
    perm = np.random.default_rng(1).permutation(len(am.instances))
    inst_a = list(am.instances)
    inst_b = []
    for i, (pi, l2w) in enumerate(inst_a):
        m = np.array(l2w, np.float64)
        m[:3, 3] = np.asarray(inst_a[perm[i]][1], np.float64)[:3, 3]
        inst_b.append((pi, m))
    am.instances = inst_b
    pose_b = tlas_side(am)
    n_mesh = len(pose_b["md"])
    view, FAR = ttconfigs.C4_VIEW, ttconfigs.FAR
    W, H = view.width, view.height
    c2w, ip = view.camera()
    dev = torch.device("cuda:0")
    eng = tthip.Engine(0)
    objects = [eng.create_object(b) for b in am.blases()]
    rays0 = torch.zeros(2 * W * H * 48, dtype=torch.uint8, device=dev)
    eng.generate(rays0, c2w, ip, W, H, ttconfigs.NEAR, FAR, jitter=1, frames=1, max_bounce=1, device=True)
    torch.cuda.synchronize(dev)

    def frame():
        """(primary ms, bounce-1 ms, the records) of one frame on the scene as the engine holds it."""
        r = rays0.clone()
        eng.timing_reset()
        eng.trace(r, W * H, 0, FAR, W, H, device=True)
        p_ms = float(eng.timing_read()[-1])
        nb = eng.enqueue_bounce(r, W * H, 0, FAR, W, H, frames=1, max_bounce=1, device=True)
        eng.timing_reset()
        eng.trace(r, nb, 1, FAR, W, H, device=True)
        b_ms = float(eng.timing_read()[-1])
        return p_ms, b_ms, r

    ms = {k: [] for k in ("a_wall", "a_presort", "a_bvh", "a_install", "b_host_build", "b_install_call",
                          "b_install_device", "c_host_tlas", "c_assemble_call", "c_total", "d_refit_primary",
                          "d_refit_bounce1", "d_rebuilt_primary", "d_rebuilt_bounce1")}
    identical = True
    n_rebuilt = records_differ = 0
    for it in range(args.warmup + args.reps):
        took = {}
        # (c) first: it also puts the scene back to pose A's arrays for the next repeat's other routes
        am.instances = inst_b
        t0 = time.perf_counter()
        side = tlas_side(am)
        eng.assemble(objects, side["nodes"], side["tlas"], side["md"], mats)
        took["c_total"] = (time.perf_counter() - t0) * 1e3
        took["c_host_tlas"] = side["host_s"] * 1e3
        took["c_assemble_call"] = took["c_total"] - took["c_host_tlas"]
        want = eng.scene_nodes(0, 2 * n_mesh).tobytes(), eng.scene_tlas_indices(0, n_mesh).tobytes()
        # pose A as uploaded, then the reference's per-frame update to pose B: _MeshData + TLAS refit
        eng.assemble(objects, pose_a["nodes"], pose_a["tlas"], pose_a["md"], mats)
        eng.update_meshdata(0, pose_b["md"])
        eng.tlas_refit(pose_a["n"], pose_b["boxes"])
        took["d_refit_primary"], took["d_refit_bounce1"], r_refit = frame()
        # (a)
        eng.timing_reset()
        t0 = time.perf_counter()
        n_rebuilt = eng.tlas_rebuild(pose_b["boxes"])
        took["a_wall"] = (time.perf_counter() - t0) * 1e3
        took["a_presort"], took["a_bvh"], took["a_install"] = (float(x) for x in eng.timing_read()[-3:])
        got = eng.scene_nodes(0, 2 * n_mesh).tobytes(), eng.scene_tlas_indices(0, n_mesh).tobytes()
        identical = identical and got == want
        took["d_rebuilt_primary"], took["d_rebuilt_bounce1"], r_rebuilt = frame()
        differing = int((r_refit.view(-1, 48) != r_rebuilt.view(-1, 48)).any(1).sum())
        records_differ = max(records_differ, differing)
        # (b), from the refit-only state again
        eng.assemble(objects, pose_a["nodes"], pose_a["tlas"], pose_a["md"], mats)
        eng.update_meshdata(0, pose_b["md"])
        eng.sync()
        t0 = time.perf_counter()
        nodes, idx = tthip.tlas_build(pose_b["boxes"])
        took["b_host_build"] = (time.perf_counter() - t0) * 1e3
        eng.timing_reset()
        t0 = time.perf_counter()
        eng.update_tlas(nodes, idx, asynchronous=True)
        took["b_install_call"] = (time.perf_counter() - t0) * 1e3
        eng.sync()
        took["b_install_device"] = float(eng.timing_read()[-1])
        got = eng.scene_nodes(0, 2 * n_mesh).tobytes(), eng.scene_tlas_indices(0, n_mesh).tobytes()
        identical = identical and got == want
        if it >= args.warmup:
            for k, v in took.items():
                ms[k].append(v)
    for o in objects:
        o.destroy()
    eng.close()
    doc = {"config": args.config, "reps": args.reps, "warmup": args.warmup, "mesh_records": int(n_mesh),
           "tlas_nodes_uploaded": pose_a["n"], "tlas_nodes_rebuilt": int(n_rebuilt), "screen": [W, H],
           "all_routes_give_identical_device_bytes": identical,
           "ray_records_differing_refit_vs_rebuilt": records_differ, "ms": {k: stat(v) for k, v in ms.items()}}
    a, b_host, b_call = doc["ms"]["a_wall"], doc["ms"]["b_host_build"], doc["ms"]["b_install_call"]
    b_lo, b_hi = b_host["min"] + b_call["min"], b_host["max"] + b_call["max"]
    overlap = a["min"] <= b_hi and b_lo <= a["max"]
    doc["b_total_median"] = round(b_host["median"] + b_call["median"], 4)
    doc["ranges_overlap"] = overlap
    doc["recommended"] = "b" if overlap or doc["b_total_median"] <= a["median"] else "a"
    doc["rule"] = "the lower C4 median of (a) the call and (b) host build + install call; (b) when the ranges overlap"
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
