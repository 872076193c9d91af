"""Float64 pin of the light-BVH refit: what tt_lights_refit / tt_lights_refit_host must leave in LightNodes and
LightTriangles. Numpy only, written from the HLSL text (LightBVHRefitter.compute:6-22, :39-111, :120-157, :174-209;
BVHRefitter.compute:135-147); it shares nothing with csrc/tt_light_refit_core.h.

pin(before, after, scene, records, transforms, conservative): `before` / `after` are the lights around one refit,
`scene` holds the 88-byte triangles the refit read, `records` the listed _MeshData records, `transforms` the
LightBVHTransform rows (None: no TLAS pass).

Mesh leaves (LightRefitKernel's leaf branch behind TransferKernel)
  * transfer: the row's pos0 / posedge1 / posedge2 are the bytes of the triangle at TriTarget + TriOffset; TriTarget
    stays.
  * box: float32 arithmetic has one answer, so the box is compared exactly: max / min of p0, p0 + e1, p0 + e2 formed
    in float32, and an axis with |max - min| < 1e-4f moved out by 1e-4f each way.
  * w decodes to -normalize(cross(normalize(e1), normalize(e2))) within E_OCT (tests/lights.py: half a code step on
    the L1 sphere, as an angle) plus the float32 cross product's error, 8 x 2^-24 (1 + its cancellation ratio).
  * phi = max(area, 1e-8) with area = |cross(e1, e2)| / 2, within Heron's bound: the three lengths are float32
    distances between float32 corners, each off by rho = 2 sqrt(3) 2^-24 max|corner| / length + 4 x 2^-24 relatively
    (the corners p0 + e are rounded sums), and Heron's s (s - a)(s - b)(s - c) amplifies a relative length error by
    cond = s / min(s - a, s - b, s - c): bound = area (1 + cond) (8 x 2^-24 + 4 rho). A triangle whose bound exceeds
    its area is marginal; at most 1% of a tree may be.
  * cosTheta_oe and left are the bytes from before.
Interior nodes (Union), mesh trees and the TLAS alike
  * box: exactly the max / min of the two children; phi: exactly their float32 sum; left: kept.
  * cos_e: the smaller child code, or one below it: decoding c -> 2 (c / 32767) - 1 and encoding floor(32767 (x + 1)
    / 2) in float32 lands on c or just under it.
  * the cone, from the children's decoded axes and cos_o codes by DoCone's own branches, in float64. An angle is a
    float32 result of the pinned acos / asin (1 ulp of at most pi: 2.4e-7 each), of a length of a difference of two
    float32 unit vectors (3.6e-7 into asin's argument, slope at most 1.42 up to 0.708), and of three float32 sums:
    ANGLE_ERR = 3e-6 covers an angle of the union. A branch decided within ANGLE_ERR is marginal (skipped, counted).
      A contains B / B contains A: the child's cone re-encoded: axis within E_OCT, cos_o code the child's or one
        below.
      the general case, default mode: Rotate returns m transpose(m), the identity up to rounding, so the axis is
        child A's decoded axis within the re-encoding bound E_OCT + 4e-6; conservative mode: A's axis turned by
        theta_o - theta_a toward B, within E_OCT + ANGLE_ERR + 4e-6. cos_o: the code of cos((theta_a + theta_d +
        theta_b) / 2), x = 32767 (cos + 1) / 2 known to d = 16383.5 ANGLE_ERR |sin| + 0.01 (three float32 roundings
        at magnitude 32767 are 0.006): any code in [floor(x - d), floor(x + d)].
      theta_o >= 3.14159: the full sphere, w = 0 (octahedral_32 of the zero vector: NaN -> 0) and cos_o code 0.
  * containment, per node with a cos_o code above 0: every leaf cone below (axis, half angle; a triangle leaf: the
    model's normal, 0) lies within acos(cos_o) + slack of w. slack = 2^-22 / max(sin_o, E_OCT) (the float32 product
    before the floor) + E_OCT (this node's re-encoding) + height x (E_OCT + 2 ANGLE_ERR): each level below re-encodes
    its axis once and decides and sums angles within ANGLE_ERR; cos_o is stored by floor, which only widens.
    Conservative mode asserts it; the default mode counts the failures (its union cone keeps A's axis and need not
    contain B's).
TLAS leaves (RefitKernel's leaf branch)
  * box: the eight corners of the root box under the matrix (float64), equal to the leaf box within 2^-22 of the
    magnitudes summed, both ways (the text's centre +- extent is exactly that box).
  * phi = max(root phi, 0) and cosTheta_oe = the root's, exactly; left kept.
  * axis: default mode the matrix of absolute values times the root's decoded axis (direction only: the encoder
    divides by the L1 norm); conservative mode the matrix itself. Within E_OCT + 16 x 2^-24 x (sum of the terms'
    magnitudes / the result's length). Where the two differ by more than twice that, the default-mode axis is
    checked to be the absolute-value one and not the rotated one: "abs exception pinned".
Everything else -- unreachable slots, trees not listed, the TLAS without transforms, rows not transferred -- keeps its
bytes.

MUTANTS change one thing of the model each; the pin must then fail, in the named category, on correct output.
"""
from dataclasses import dataclass, field

import numpy as np

import producers as P
from lights import E_OCT, U24

PI_TEXT = float(np.float32(3.14159))
ANGLE_ERR = 3e-6
MARGINAL_CAP = 0.01
MUTANTS = {"leaf_phi_0.1": "leaf phi", "no_pad": "leaf box", "phi_max": "node phi", "cos_e_max": "node cos_e",
           "axis_of_b": "node axis", "no_translation": "tlas box", "row_major": "tlas box", "stale_child": "node box"}
F32 = np.float32


@dataclass
class Report:
    failures: dict = field(default_factory=dict)
    worst: dict = field(default_factory=dict)
    leaves: int = 0
    marginal_phi: int = 0
    marginal_phi_worst_tree: float = 0.0
    interior: int = 0
    branch: dict = field(default_factory=lambda: {"A": 0, "B": 0, "union": 0, "full": 0, "marginal": 0, "nan": 0})
    tlas_leaves: int = 0
    containment_checked: int = 0
    containment_failures: int = 0
    full_sphere: int = 0
    abs_exception: int = 0

    def fail(self, cat, what):
        self.failures.setdefault(cat, []).append(what)

    def frac(self, cat, value, bound, what):
        f = float(value / bound) if bound > 0 else (0.0 if value == 0 else np.inf)
        self.worst[cat] = max(self.worst.get(cat, 0.0), f)
        if not f <= 1.0:
            self.fail(cat, f"{what}: {f:.3g} of the bound")

    @property
    def ok(self):
        return not self.failures and self.marginal_phi_worst_tree <= MARGINAL_CAP

    def lines(self):
        b = self.branch
        return [f"leaves {self.leaves} marginal phi {self.marginal_phi} interior {self.interior} (A {b['A']} B {b['B']} union "
                f"{b['union']} full {b['full']} marginal {b['marginal']} nan {b['nan']}) tlas leaves {self.tlas_leaves}",
                f"containment checked {self.containment_checked} failures {self.containment_failures} full sphere "
                f"{self.full_sphere} abs exception pinned {self.abs_exception}",
                "worst fractions " + " ".join(f"{k}={v:.3f}" for k, v in sorted(self.worst.items())),
                "failures " + "; ".join(f"{k}: {v[0]} (+{len(v) - 1})" for k, v in sorted(self.failures.items()))]


def _bfs(left, base):
    """[(node, height)] of the tree at `base`, the root first; height = levels of interior nodes below, + 0 at a leaf."""
    order, at = [base], 0
    while at < len(order):
        l = int(left[order[at]])
        if l >= 0:
            order += [base + l, base + l + 1]
        at += 1
    height = {}
    for n in reversed(order):
        l = int(left[n])
        height[n] = 0 if l < 0 else 1 + max(height[base + l], height[base + l + 1])
    return order, height


def _angle(a, b):
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


def _lo(nd):
    return int(nd["cosTheta_oe"]) & 0xFFFF


def _hi(nd):
    return int(nd["cosTheta_oe"]) >> 16


def _cos_of(code):
    return 2.0 * (code / 32767.0) - 1.0


def _union_checks(rep, A, B, nd, k, conservative, mutant):
    """The cone of node k from its children, by DoCone's branches."""
    wa, wb = P.oct_decode(np.uint32(A["w"])), P.oct_decode(np.uint32(B["w"]))
    ca, cb = _cos_of(_lo(A)), _cos_of(_lo(B))
    if not (-1.0 <= ca <= 1.0 and -1.0 <= cb <= 1.0):
        rep.branch["nan"] += 1
        return
    ta, tb = np.arccos(ca), np.arccos(cb)
    if wa @ wb < 0:
        td = PI_TEXT - 2.0 * np.arcsin(min(np.linalg.norm(wa + wb) / 2.0, 1.0))
    else:
        td = 2.0 * np.arcsin(min(np.linalg.norm(wb - wa) / 2.0, 1.0))
    g1, g2 = min(td + tb, PI_TEXT) - ta, min(td + ta, PI_TEXT) - tb
    w = P.oct_decode(np.uint32(nd["w"]))
    lo = _lo(nd)
    if abs(g1) <= ANGLE_ERR or (g1 > 0 and abs(g2) <= ANGLE_ERR):
        rep.branch["marginal"] += 1
        return
    if g1 <= 0 or g2 <= 0:
        which, src, wsrc = ("A", A, wa) if g1 <= 0 else ("B", B, wb)
        rep.branch[which] += 1
        rep.frac("node axis", _angle(w, wsrc), E_OCT + 4e-6, f"node {k} ({which} kept)")
        if lo not in (_lo(src), _lo(src) - 1):
            rep.fail("node cos_o", f"node {k}: code {lo}, child's {_lo(src)}")
        return
    to = (ta + td + tb) / 2.0
    if abs(to - PI_TEXT) <= ANGLE_ERR:
        rep.branch["marginal"] += 1
        return
    wr = np.cross(wa, wb)
    if to >= PI_TEXT or wr @ wr < 1e-24:
        rep.branch["full"] += 1
        if int(nd["w"]) != 0 or lo != 0:
            rep.fail("node axis", f"node {k}: the full sphere is w 0, cos_o code 0; got {int(nd['w'])}, {lo}")
        return
    rep.branch["union"] += 1
    if conservative:
        kx = wr / np.linalg.norm(wr)
        tr = to - ta
        want = wa * np.cos(tr) + np.cross(kx, wa) * np.sin(tr)
        tol = E_OCT + ANGLE_ERR + 4e-6
    else:
        want = wb if mutant == "axis_of_b" else wa
        tol = E_OCT + 4e-6
    rep.frac("node axis", _angle(w, want), tol, f"node {k}")
    x = 32767.0 * ((np.cos(to) + 1.0) / 2.0)
    d = 16383.5 * ANGLE_ERR * abs(np.sin(to)) + 0.01
    if not (np.floor(x - d) <= lo <= np.floor(x + d)):
        rep.fail("node cos_o", f"node {k}: code {lo}, want floor({x:.4f} +- {d:.4f})")
    rep.worst["node cos_o"] = max(rep.worst.get("node cos_o", 0.0), float(abs((lo + 0.5) - x) / (0.5 + d)))


def _interior(rep, nodes_b, nodes_a, base, k, conservative, mutant, stale):
    nd = nodes_a[k]
    l = int(nd["left"])
    A, B = nodes_a[base + l], nodes_a[base + l + 1]
    if mutant == "stale_child" and not stale["done"] and nodes_b[base + l].tobytes() != A.tobytes() and \
            not np.array_equal(nodes_b[base + l]["BBMax"], A["BBMax"]):
        A = nodes_b[base + l]
        stale["done"] = True
    rep.interior += 1
    if not (np.array_equal(nd["BBMax"], np.maximum(A["BBMax"], B["BBMax"])) and
            np.array_equal(nd["BBMin"], np.minimum(A["BBMin"], B["BBMin"]))):
        rep.fail("node box", f"node {k} is not the max / min of its children")
    want_phi = max(F32(A["phi"]), F32(B["phi"])) if mutant == "phi_max" else F32(A["phi"]) + F32(B["phi"])
    if F32(nd["phi"]) != F32(want_phi):
        rep.fail("node phi", f"node {k}: {nd['phi']} is not the float32 sum {want_phi}")
    m = max(_hi(A), _hi(B)) if mutant == "cos_e_max" else min(_hi(A), _hi(B))
    if _hi(nd) not in (m, m - 1):
        rep.fail("node cos_e", f"node {k}: code {_hi(nd)}, children {_hi(A)}, {_hi(B)}")
    _union_checks(rep, A, B, nd, k, conservative, mutant)


def _containment(rep, nodes_a, order, height, base, leaf_cone, conservative):
    """leaf_cone[node] = (axis, half angle) of the leaves; every interior node against the leaves below it."""
    below = {}
    for n in reversed(order):
        l = int(nodes_a["left"][n])
        below[n] = [n] if l < 0 else below[base + l] + below[base + l + 1]
        if l < 0:
            continue
        lo = _lo(nodes_a[n])
        if lo == 0:
            rep.full_sphere += 1
            continue
        cos_o = _cos_of(lo)
        theta = np.arccos(np.clip(cos_o, -1, 1))
        sin_o = max(np.sqrt(max(1 - cos_o * cos_o, 0.0)), E_OCT)
        slack = 2.0 ** -22 / sin_o + E_OCT + height[n] * (E_OCT + 2 * ANGLE_ERR)
        if any(leaf_cone[q] is None for q in below[n]):  # a full-sphere leaf below: nothing narrower to hold it
            continue
        w = P.oct_decode(np.uint32(nodes_a["w"][n]))
        worst = max(_angle(w, leaf_cone[q][0]) + leaf_cone[q][1] - theta for q in below[n])
        rep.containment_checked += 1
        if worst > slack:
            rep.containment_failures += 1
            if conservative:
                rep.fail("containment", f"node {n}: a leaf cone leaves it by {worst:.3g} (slack {slack:.3g})")
        elif conservative:
            rep.worst["containment"] = max(rep.worst.get("containment", 0.0), float(max(worst, 0.0) / slack))


def pin(before, after, scene, records, transforms, conservative=False, mutant=None) -> Report:
    assert mutant is None or mutant in MUTANTS
    rep = Report()
    nb, na = before.nodes, after.nodes
    md, lm = scene.meshdata, after.meshes
    if not np.array_equal(nb["left"], na["left"]):
        rep.fail("kept", "a left changed")
        return rep
    touched = np.zeros(len(na), bool)
    rows_done = np.zeros(len(after.tris), bool)
    stale = {"done": False}
    for r in records:
        off = int(md["LightNodeOffset"][r])
        owner = [i for i in range(len(lm)) if int(md["LightNodeOffset"][int(lm["LockedMeshIndex"][i])]) == off]
        start, tri_off = int(lm["StartIndex"][owner[0]]), int(md["TriOffset"][r])
        order, height = _bfs(na["left"], off)
        touched[order] = True
        leaf_cone, marginal, n_leaves = {}, 0, 0
        for k in order:
            nd = na[k]
            l = int(nd["left"])
            if l >= 0:
                continue
            n_leaves += 1
            row = start + (-(l + 1))
            rows_done[row] = True
            T, S = after.tris[row], scene.tris[int(after.tris["TriTarget"][row]) + tri_off]
            if T["TriTarget"] != before.tris["TriTarget"][row] or any(T[f].tobytes() != S[f].tobytes() for f in ("pos0", "posedge1", "posedge2")):
                rep.fail("transfer", f"row {row} is not its aggregated triangle")
            p0, e1, e2 = F32(T["pos0"]), F32(T["posedge1"]), F32(T["posedge2"])
            c1, c2 = p0 + e1, p0 + e2  # float32
            mx, mn = np.maximum(np.maximum(p0, c1), c2), np.minimum(np.minimum(p0, c1), c2)
            thin = np.abs(mx - mn) < F32(0.0001)
            if mutant != "no_pad":
                mx, mn = np.where(thin, mx + F32(0.0001), mx).astype(F32), np.where(thin, mn - F32(0.0001), mn).astype(F32)
            if not (np.array_equal(nd["BBMax"], mx) and np.array_equal(nd["BBMin"], mn)):
                rep.fail("leaf box", f"node {k}: not the float32 box of its corners{' (thin axis)' if thin.any() else ''}")
            d1, d2 = e1.astype(np.float64), e2.astype(np.float64)
            cr = np.cross(d1, d2)
            axis = -cr / np.linalg.norm(cr)
            cancel = (np.abs(d1[[1, 2, 0]] * d2[[2, 0, 1]]) + np.abs(d1[[2, 0, 1]] * d2[[1, 2, 0]])).max() / np.linalg.norm(cr)
            rep.frac("leaf w", _angle(P.oct_decode(np.uint32(nd["w"])), axis), E_OCT + 8 * U24 * (1 + cancel) + 8 * U24, f"node {k}")
            leaf_cone[k] = (axis, 0.0)
            area = 0.5 * np.linalg.norm(cr)
            a, b, c = np.linalg.norm(d1), np.linalg.norm(d1 - d2), np.linalg.norm(d2)
            hs = (a + b + c) / 2
            cond = hs / min(hs - a, hs - b, hs - c)
            cmax = max(np.abs(p0).max(), np.abs(c1).max(), np.abs(c2).max())
            rho = 2 * np.sqrt(3.0) * U24 * cmax / min(a, b, c) + 4 * U24
            bound = area * (1 + cond) * (8 * U24 + 4 * rho)
            if not bound <= area:
                marginal += 1
            else:
                want = np.float64(F32(0.1)) if mutant == "leaf_phi_0.1" else max(area, 1e-8)
                rep.frac("leaf phi", abs(float(nd["phi"]) - want), bound, f"node {k}: phi {nd['phi']} area {area:.6g}")
            if nd["cosTheta_oe"] != nb["cosTheta_oe"][k]:
                rep.fail("kept", f"leaf {k}: cosTheta_oe changed")
        rep.leaves += n_leaves
        rep.marginal_phi += marginal
        rep.marginal_phi_worst_tree = max(rep.marginal_phi_worst_tree, marginal / n_leaves)
        for k in order:
            if int(na["left"][k]) >= 0:
                _interior(rep, nb, na, off, k, conservative, mutant, stale)
        _containment(rep, na, order, height, off, leaf_cone, conservative)
    if transforms is not None:
        order, height = _bfs(na["left"], 0)
        touched[order] = True
        leaf_cone = {}
        for k in order:
            nd = na[k]
            l = int(nd["left"])
            if l >= 0:
                continue
            rep.tlas_leaves += 1
            X = transforms[-(l + 1)]
            M = X["Transform"].astype(np.float64).reshape(4, 4)
            M = M if mutant == "row_major" else M.T
            t = np.zeros(3) if mutant == "no_translation" else M[:3, 3]
            M3 = M[:3, :3]
            root = na[int(X["SolidOffset"])]
            lo_, hi_ = root["BBMin"].astype(np.float64), root["BBMax"].astype(np.float64)
            cs = np.array([[x, y, z] for x in (lo_[0], hi_[0]) for y in (lo_[1], hi_[1]) for z in (lo_[2], hi_[2])])
            wc = cs @ M3.T + t
            tol = 2.0 ** -22 * (np.abs(cs) @ np.abs(M3).T + np.abs(t)).max(0)
            off_by = np.maximum(np.abs(wc.max(0) - nd["BBMax"]), np.abs(wc.min(0) - nd["BBMin"]))
            rep.frac("tlas box", float((off_by / tol).max()), 1.0, f"TLAS leaf {k}")
            if F32(nd["phi"]) != max(F32(root["phi"]), F32(0)) or nd["cosTheta_oe"] != root["cosTheta_oe"]:
                rep.fail("tlas copy", f"TLAS leaf {k}: phi / codes are not the root's")
            wroot = P.oct_decode(np.uint32(root["w"]))
            va, vm = np.abs(M3) @ wroot, M3 @ wroot
            mag = np.abs(M3) @ np.abs(wroot)
            tol_a = E_OCT + 16 * U24 * np.linalg.norm(mag) / np.linalg.norm(va)
            tol_m = E_OCT + 16 * U24 * np.linalg.norm(mag) / np.linalg.norm(vm)
            w = P.oct_decode(np.uint32(nd["w"]))
            if conservative:
                rep.frac("tlas axis", _angle(w, vm), tol_m, f"TLAS leaf {k} (matrix)")
            else:
                rep.frac("tlas axis", _angle(w, va), tol_a, f"TLAS leaf {k} (absolute values)")
                if _angle(va, vm) > 2 * (tol_a + tol_m) and _angle(w, va) <= tol_a and _angle(w, vm) > tol_m:
                    rep.abs_exception += 1
            leaf_cone[k] = None if _lo(nd) == 0 else (w, float(np.arccos(np.clip(_cos_of(_lo(nd)), -1, 1))))
        for k in order:
            if int(na["left"][k]) >= 0:
                _interior(rep, nb, na, 0, k, conservative, mutant, stale)
        if any(v is not None for v in leaf_cone.values()):
            _containment(rep, na, order, height, 0, leaf_cone, conservative)
    if mutant == "stale_child" and not stale["done"]:
        rep.fail("setup", "no interior node has a child the refit changed")
    keep = ~touched
    if na[keep].tobytes() != nb[keep].tobytes():
        rep.fail("kept", "a node no refit reaches changed")
    if after.tris[~rows_done].tobytes() != before.tris[~rows_done].tobytes():
        rep.fail("kept", "a light triangle of an unlisted mesh changed")
    return rep
