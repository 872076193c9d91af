#!/usr/bin/env python3
"""Times the BLAS refit of deforming meshes one call per mesh (tt_blas_refit) against one call for the frame
(tt_blas_refit_many), device pointers, asynchronous calls:

  (a) the one 262k-triangle mesh of bench.py's blas_refit_c2 figure: tt_blas_refit against tt_blas_refit_many
      with one item of one part -- what the batch form costs the one-mesh case, which launches tt_blas_refit's own
      Construct kernel -- and with the same mesh cut into two parts, which takes the staged form
      (blas_construct_many) every other list takes;
  (b) 64 props of about 4,000 triangles, two parts each: a loop of 64 tt_blas_refit calls, each over the prop's
      concatenated vertex buffer (the same arithmetic), against one tt_blas_refit_many that also writes bounds_out
      and every prop's world box into mesh_aabbs (b_many), and against the same call without outputs.

Per route and repeat: the host wall time of the asynchronous call(s), then, after a sync, the device time
(tt_timing_read, summed over the route's entries). One warm-up, then --reps repeats with the routes in turn
inside each repeat; medians with min-max. --parent-lib names another build of libtruetrace_hip.so (the parent
commit's): its single-call figures of (a) and (b) are taken in a child process and reported beside this one's.

    python tools/refit_bench.py [--out profiles/r19/refit_batch/bench.json] [--reps 7] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "truetrace-unity-pathtracer_amd", "python"))


def stat(v, digits=4):
    import numpy as np

    return {"median": round(float(np.median(v)), digits), "min": round(float(min(v)), digits), "max": round(float(max(v)), digits)}


def vertex_buffer(pos, nrm, t):
    import numpy as np

    p = pos.astype(np.float64).copy()
    p[:, 0] += 0.05 * np.sin(1.7 * p[:, 1] + t)
    p[:, 2] += 0.05 * np.cos(1.3 * p[:, 0] - t)
    v = np.zeros((len(pos), 10), np.float32)  # Unity-like stride: position, normal, tangent
    v[:, 0:3], v[:, 3:6] = p.astype(np.float32), nrm
    return v


def two_parts(v, idx):
    """A mesh cut into two renderers at an odd triangle: each part's own compacted vertex buffer and local indices,
    and the concatenated buffer with shifted indices that the per-mesh call takes."""
    import numpy as np

    tri = idx.reshape(-1, 3)
    cut = len(tri) // 2 + 1
    parts, vc, ic, off = [], [], [], 0
    for a, b in ((0, cut), (cut, len(tri))):
        uniq, inv = np.unique(tri[a:b], return_inverse=True)
        local = np.ascontiguousarray(inv.reshape(-1), np.int32)
        parts.append((np.ascontiguousarray(v[uniq]), local, a))
        vc.append(v[uniq])
        ic.append(local + off)
        off += len(uniq)
    return parts, np.ascontiguousarray(np.vstack(vc)), np.concatenate(ic).astype(np.int32)


def measure(eng, routes, warmup, reps):
    """routes: {name: callable issuing the route's asynchronous calls}. {name: {"wall_ms": [...], "device_ms": [...]}}"""
    out = {k: {"wall_ms": [], "device_ms": []} for k in routes}
    for it in range(warmup + reps):
        for name, issue in routes.items():
            eng.sync()
            eng.timing_reset()
            t0 = time.perf_counter()
            issue()
            wall = (time.perf_counter() - t0) * 1e3
            eng.sync()
            dev = float(eng.timing_read().sum())
            if it >= warmup:
                out[name]["wall_ms"].append(wall)
                out[name]["device_ms"].append(dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r19", "refit_batch", "bench.json"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--props", type=int, default=64)
    ap.add_argument("--prop-tris", type=int, default=4000)
    ap.add_argument("--small", action="store_true", help="a 20k-triangle mesh and 8 props: for checking the tool itself")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--single-only", action="store_true", help="(the child run of --parent-lib) no tt_blas_refit_many")
    args = ap.parse_args()
    parent = None
    if args.parent_lib and not args.single_only:
        env = dict(os.environ, TT_HIP_LIB=os.path.abspath(args.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--single-only", "--out", "-", "--reps", str(args.reps),
               "--warmup", str(args.warmup), "--props", str(args.props), "--prop-tris", str(args.prop_tris)]
        r = subprocess.run(cmd + (["--small"] if args.small else []), env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr)
            return 1
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    import numpy as np
    import torch

    import tthip

    dev = torch.device("cuda:0")
    L = tthip.hip_lib()
    many = hasattr(L, "tt_blas_refit_many") and not args.single_only
    flags = tthip.TT_TRACE_DEVICE_PTRS | tthip.TT_TRACE_ASYNC
    keep = []

    def to_dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t

    def single_params(record, n_tris, n_vertices):
        p = tthip.BlasRefitParams(mesh_index=record, n_tris=n_tris, n_vertices=n_vertices, vertex_stride=10, flags=flags)
        p.transform[:] = tthip.unity_colmajor(np.eye(4))
        return p

    doc = {"reps": args.reps, "warmup": args.warmup, "library": os.environ.get("TT_HIP_LIB", "this tree")}
    eng = tthip.Engine(0)
    # ---------------------------------------------------------------- (a) one large mesh
    mesh = tthip.Mesh.sponza(n_tris=20000) if args.small else tthip.Mesh.sponza()
    blas = tthip.Blas(mesh)
    am = tthip.AssetManager()
    am.add_parent(blas, None, np.zeros(7, tthip.MAT_DTYPE))
    sc = am.build()
    eng.upload(sc)
    pos, nrm, idx = mesh.arrays()
    n_tris = len(idx) // 3
    v_t, i_t, l_t = to_dev(vertex_buffer(pos, nrm, 0.4)), to_dev(np.ascontiguousarray(idx, np.int32)), to_dev(blas.leaf_order())
    p_a = single_params(0, n_tris, len(pos))

    def a_single():
        st = L.tt_blas_refit(eng.h, C.byref(p_a), v_t.data_ptr(), i_t.data_ptr(), l_t.data_ptr())
        assert st == 0, st

    routes = {"a_single": a_single}
    if many:
        item = tthip.RefitItem(0, n_tris, l_t, [tthip.RefitPart(v_t, i_t, 0, n_vertices=len(pos), vertex_stride=10, n_tris=n_tris)])
        arr_a, keep_a = tthip.refit_item_array([item])

        def a_many():
            st = L.tt_blas_refit_many(eng.h, arr_a, 1, flags, None, None)
            assert st == 0, st

        routes["a_many"] = a_many
        # the same mesh as two parts over the concatenated buffer: the staged form (descriptors through the pinned
        # slot, blas_construct_many), which one item of one part does not take
        parts2, vcat, icat = two_parts(vertex_buffer(pos, nrm, 0.4), np.ascontiguousarray(idx, np.int32))
        item2 = tthip.RefitItem(0, n_tris, l_t, [
            tthip.RefitPart(to_dev(pv), to_dev(pi), first, n_vertices=len(pv), vertex_stride=10, n_tris=len(pi) // 3)
            for pv, pi, first in parts2])
        arr_a2, keep_a2 = tthip.refit_item_array([item2])

        def a_many_two_parts():
            st = L.tt_blas_refit_many(eng.h, arr_a2, 1, flags, None, None)
            assert st == 0, st

        routes["a_many_two_parts"] = a_many_two_parts
        a_single()
        eng.sync()
        want = eng.scene_nodes(0, len(sc.nodes)).tobytes(), eng.scene_tris(0, len(sc.tris)).tobytes()
        eng.upload(sc)
        a_many()
        eng.sync()
        doc["a_identical_bytes"] = want == (eng.scene_nodes(0, len(sc.nodes)).tobytes(), eng.scene_tris(0, len(sc.tris)).tobytes())
        eng.upload(sc)
        a_many_two_parts()
        eng.sync()
        doc["a_two_parts_identical_bytes"] = want == (eng.scene_nodes(0, len(sc.nodes)).tobytes(),
                                                      eng.scene_tris(0, len(sc.tris)).tobytes())
    res = measure(eng, routes, args.warmup, args.reps)
    doc["a"] = {"tris": int(n_tris), **{k: {m: stat(v) for m, v in r.items()} for k, r in res.items()}}
    if many:
        s, m = doc["a"]["a_single"]["device_ms"], doc["a"]["a_many"]["device_ms"]
        doc["a"]["many_device_median_inside_single_min_max"] = bool(s["min"] <= m["median"] <= s["max"])
    # ---------------------------------------------------------------- (b) many props, two parts each
    n_props = 8 if args.small else args.props
    meshes = [tthip.Mesh.prop(900 + k, args.prop_tris) for k in range(n_props)]
    blases = [tthip.Blas(m) for m in meshes]
    am = tthip.AssetManager()
    l2w = [tthip.trs_matrix((3.0 * (k % 8), 0.0, 3.0 * (k // 8)), 10.0 * k, 1.0) for k in range(n_props)]
    for b, m in zip(blases, l2w):
        am.add_parent(b, m, np.zeros(1, tthip.MAT_DTYPE))
    sc = am.build()
    eng.upload(sc)
    singles, items = [], []
    for k, (m, b) in enumerate(zip(meshes, blases)):
        pos, nrm, idx = m.arrays()
        parts, vcat, icat = two_parts(vertex_buffer(pos, nrm, 0.1 * k), np.ascontiguousarray(idx, np.int32))
        leaf = to_dev(b.leaf_order())
        singles.append((single_params(k, b.n_tris, len(vcat)), to_dev(vcat).data_ptr(), to_dev(icat).data_ptr(), leaf.data_ptr()))
        items.append(tthip.RefitItem(k, b.n_tris, leaf, [
            tthip.RefitPart(to_dev(pv), to_dev(pi), first, n_vertices=len(pv), vertex_stride=10, n_tris=len(pi) // 3)
            for pv, pi, first in parts], l2w[k]))

    def b_loop():
        for p, v, i, l in singles:
            st = L.tt_blas_refit(eng.h, C.byref(p), v, i, l)
            assert st == 0, st

    routes = {"b_loop": b_loop}
    if many:
        arr_b, keep_b = tthip.refit_item_array(items)
        d_boxes = to_dev(np.ascontiguousarray(sc.meta["mesh_aabbs"], np.float32))
        d_bounds = to_dev(np.zeros((len(items), 6), np.float32))

        def b_many():  # with both outputs, as the refit -> TLAS refit -> trace chain calls it
            st = L.tt_blas_refit_many(eng.h, arr_b, len(items), flags, d_bounds.data_ptr(), d_boxes.data_ptr())
            assert st == 0, st

        def b_many_no_outputs():  # the loop's work exactly: no root boxes, no world boxes
            st = L.tt_blas_refit_many(eng.h, arr_b, len(items), flags, None, None)
            assert st == 0, st

        routes["b_many"] = b_many
        routes["b_many_no_outputs"] = b_many_no_outputs
        b_loop()
        eng.sync()
        want = eng.scene_nodes(0, len(sc.nodes)).tobytes(), eng.scene_tris(0, len(sc.tris)).tobytes()
        eng.upload(sc)
        b_many()
        eng.sync()
        doc["b_identical_bytes"] = want == (eng.scene_nodes(0, len(sc.nodes)).tobytes(), eng.scene_tris(0, len(sc.tris)).tobytes())
    res = measure(eng, routes, args.warmup, args.reps)
    doc["b"] = {"props": n_props, "tris_per_prop": int(blases[0].n_tris), "parts_per_prop": 2,
                **{k: {m: stat(v) for m, v in r.items()} for k, r in res.items()}}
    if many:
        for m in ("wall_ms", "device_ms"):
            doc["b"][f"loop_over_many_{m}"] = round(doc["b"]["b_loop"][m]["median"] / doc["b"]["b_many"][m]["median"], 2)
    eng.close()
    if parent is not None:
        doc["parent_library"] = {"a_single": parent["a"]["a_single"], "b_loop": parent["b"]["b_loop"]}
    print(json.dumps(doc), flush=True)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    ok = (not many) or (doc.get("a_identical_bytes") and doc.get("b_identical_bytes"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
