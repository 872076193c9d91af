"""Float64 model of the light BVH: what the builders must guarantee, and what SampleLightBVH and the NEE emit compute.

Numpy only, written from the text (CommonData.cginc:1007-1043, :1126-1166, :824-839, :1911-1920;
RayTracingShader.compute:391-479); it calls nothing of the library but the dtypes and reads none of the host
reference's internals. The hit's frame (pos, norm) comes from tests/producers.py, the model of the enqueue.

1. check_build(case): invariants of LightNodes / LightTriangles / _LightMeshes as assembled.
   * box: every node box of a mesh tree holds every corner p0, p0 + e1, p0 + e2 of every light triangle below it.
     The builder forms the corners in float32, so a corner may lie half an ulp outside: LIMIT = 2^-23 max|coord|.
   * cone: the axis w decoded from its 16:16 octahedral code and cos_o from the low half of cosTheta_oe; every leaf
     axis (the negated triangle normal given to the builder) below the node lies within acos(cos_o) + slack of w.
       - the code's step is 1 / 32767.5 per coordinate, half a step of error each; on the L1 sphere a coordinate
         error (dx, dy) moves the point by at most sqrt(dx^2 + dy^2 + (|dx| + |dy|)^2) <= sqrt(6) / 65535, and the
         point is at least 1 / sqrt(3) from the origin: an angle of at most sqrt(18) / 65535 = 6.5e-5;
       - cos_o is stored by floor, which only widens the cone; the float32 product before it can round up by one
         part in 2^23 of 32767, below a tenth of a step: 2^-22 in cos, taken as an angle through 1 / sin floored
         at the same 6.5e-5;
       - the builder's angles are float32 sums of up to pi (ulp 2.4e-7), a handful per union, and its pi is
         3.14159, 2.7e-6 short: 4e-6 per level below the node.
     A node with cos_o = -1 (low half 0) is the full sphere: nothing to check; they are counted.
   * phi = 0.1f x leaves below, within the float32 sum's bound (leaves x 2^-24 x the sum).
   * leaves <-> light triangles of the parent and TLAS leaves <-> light meshes are bijections; every left is even, in
     range and greater than its node's index; rows: IndexEnd - StartIndex = the record's LightTriCount.
   * tlas: a TLAS leaf box holds the eight corners of its mesh tree's root box under the instance transform
     (float64), within 2^-22 of the magnitudes summed; every TLAS node box holds its leaves' boxes exactly.

2. pin(case, rays, ...): the sampler and the emitted ray. Every float32 operation of Importance is followed with a
   running error bound (class E: value, absolute bound; each operation adds 2^-24 |result| to the propagated
   bounds; sqrt(max(x, 0)) takes the interval's image). Branches that a value within its bound could take either
   way make the ray marginal, except the two clamps of cosSubClamped / sinSubClamped, which are continuous across
   their condition (cos a cos b + sin a sin b = 1 and sin a cos b - cos a sin b = 0 at cos a = cos b): there the
   bound is widened to reach the other branch's value. random() is integer arithmetic and one float32 product,
   reproduced exactly. A decision u >= cx / (cx + cy) is marginal when |u - ratio| is within the ratio's bound.
   Marginal rays are skipped and counted; at most 1% of a set may be marginal.
   The model walks from the root by its own decisions and must arrive where the sample says: the leaf (or the dead
   end), the mesh, Reps at return (interior steps, + 1 for the TLAS -> mesh transition, + 1 for the step that
   returns the leaf -- the loop increments Reps before it looks at the node), and the weight within its bound.
   Mutants (MUTANTS) change one thing of the model each; the pin must then fail on the host reference's output.
"""
from dataclasses import dataclass, field

import numpy as np

import producers as P
import tthip

U24 = 2.0 ** -24
E_OCT = np.sqrt(18.0) / 65535.0
MARGINAL_CAP = 0.01
MUTANTS = ["reps_const", "gt", "weight_mul", "normal_untransformed", "no_scale", "no_node_offset", "no_start_index",
           "cos_e_low_half", "d2_no_floor", "t_no_offset", "rand79_swapped", "sample_triangle_swapped"]


# ------------------------------------------------------------------ decoding
def oct_decode(code):
    return P.oct_decode(code)


def node_fields(nodes):
    return dict(bmax=nodes["BBMax"].astype(np.float64), bmin=nodes["BBMin"].astype(np.float64), w=nodes["w"],
                phi=nodes["phi"].astype(np.float64), lo=(nodes["cosTheta_oe"] & 0xFFFF).astype(np.float64),
                hi=(nodes["cosTheta_oe"] >> 16).astype(np.float64), left=nodes["left"].astype(np.int64))


def subtree(nodes, base, root=0):
    """(nodes below `root`, leaves below each of them) of the tree at `base`: {rel: [leaf values]}."""
    below = {}

    def walk(rel):
        left = int(nodes["left"][base + rel])
        if left < 0:
            below[rel] = [-(left + 1)]
        else:
            walk(left)
            walk(left + 1)
            below[rel] = below[left] + below[left + 1]
        return below[rel]

    walk(root)
    return below


def depth_below(nodes, base, rel):
    left = int(nodes["left"][base + rel])
    return 0 if left < 0 else 1 + max(depth_below(nodes, base, left), depth_below(nodes, base, left + 1))


# ------------------------------------------------------------------ 1. the build
@dataclass
class BuildReport:
    box: list = field(default_factory=list)
    cone: list = field(default_factory=list)
    phi: list = field(default_factory=list)
    bijection: list = field(default_factory=list)
    left: list = field(default_factory=list)
    rows: list = field(default_factory=list)
    tlas: list = field(default_factory=list)
    full_sphere: int = 0
    nodes_checked: int = 0

    @property
    def ok(self):
        return not (self.box or self.cone or self.phi or self.bijection or self.left or self.rows or self.tlas)

    def failed(self):
        return [k for k in ("box", "cone", "phi", "bijection", "left", "rows", "tlas") if getattr(self, k)]


def _check_left(nodes, base, end, rep, what):
    stack = [0]
    while stack:
        rel = stack.pop()
        left = int(nodes["left"][base + rel])
        if left < 0:
            continue
        if left % 2 or left <= rel or base + left + 1 >= end:
            rep.left.append((what, base + rel, left))
            continue
        stack += [left, left + 1]


def check_build(lights, scene, parents, instances) -> BuildReport:
    rep = BuildReport()
    nodes, ltris, lmeshes = lights.nodes, lights.tris, lights.meshes
    n_inst = len(lmeshes)
    md = scene.meshdata
    _check_left(nodes, 0, 2 * n_inst, rep, "tlas")
    if rep.left:
        return rep
    tl = subtree(nodes, 0)
    if sorted(tl[0]) != list(range(n_inst)):
        rep.bijection.append(("tlas", sorted(tl[0])))
    F = node_fields(nodes)
    seen_off = {}
    for i, (par, mesh_index, l2w) in enumerate(instances):
        row = lmeshes[i]
        off = int(md["LightNodeOffset"][mesh_index])
        lt, normals = parents[par]
        n = len(lt)
        if int(row["IndexEnd"]) - int(row["StartIndex"]) != int(md["LightTriCount"][mesh_index]) or int(row["LockedMeshIndex"]) != mesh_index \
                or int(md["LightTriCount"][mesh_index]) != n:
            rep.rows.append((i, int(row["StartIndex"]), int(row["IndexEnd"])))
            continue
        start = int(row["StartIndex"])
        if off not in seen_off:
            seen_off[off] = True
            _check_left(nodes, off, len(nodes), rep, "mesh")
            if rep.left:
                return rep
            below = subtree(nodes, off)
            if sorted(below[0]) != list(range(n)):
                rep.bijection.append(("mesh", i))
                continue
            T = ltris[start:start + n]
            p0 = T["pos0"].astype(np.float64)
            corners = np.stack([p0, p0 + T["posedge1"].astype(np.float64), p0 + T["posedge2"].astype(np.float64)], 1)
            if not np.array_equal(T, lt):
                rep.rows.append((i, "triangles"))
            axes = -P._unit(np.asarray(normals, np.float64))
            for rel, leaves in below.items():
                k = off + rel
                rep.nodes_checked += 1
                c = corners[leaves].reshape(-1, 3)
                lim = 2.0 ** -23 * np.abs(c).max()
                if (c > F["bmax"][k] + lim).any() or (c < F["bmin"][k] - lim).any():
                    rep.box.append(k)
                want = np.float64(np.float32(0.1)) * len(leaves)
                if abs(F["phi"][k] - want) > len(leaves) * U24 * want + U24 * want:
                    rep.phi.append((k, F["phi"][k], want))
                if F["lo"][k] == 0:
                    rep.full_sphere += 1
                    continue
                cos_o = 2.0 * (F["lo"][k] / 32767.0) - 1.0
                theta = np.arccos(np.clip(cos_o, -1, 1))
                w = oct_decode(np.array([F["w"][k]], np.uint32))[0]
                ang = np.arccos(np.clip(axes[leaves] @ w, -1, 1))
                sin_o = max(np.sqrt(max(1 - cos_o * cos_o, 0.0)), E_OCT)
                slack = E_OCT + 2.0 ** -22 / sin_o + 4e-6 * (1 + depth_below(nodes, off, rel))
                if (ang > theta + slack).any():
                    rep.cone.append((k, float((ang - theta).max()), slack))
        # the TLAS leaf of this instance
        leaf_nodes = [r for r, v in tl.items() if v == [i] and int(nodes["left"][r]) < 0]
        if len(leaf_nodes) != 1:
            rep.bijection.append(("tlas leaf", i))
            continue
        k = leaf_nodes[0]
        lo, hi = F["bmin"][off], F["bmax"][off]
        cs = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        M = np.asarray(l2w, np.float64)
        Mf = M.astype(np.float32).astype(np.float64)
        wc = cs @ Mf[:3, :3].T + Mf[:3, 3]
        mag = (np.abs(cs) @ np.abs(Mf[:3, :3]).T + np.abs(Mf[:3, 3])).max(0)
        if (wc > F["bmax"][k] + 2.0 ** -22 * mag).any() or (wc < F["bmin"][k] - 2.0 ** -22 * mag).any():
            rep.tlas.append((i, k))
    for rel, leaves in tl.items():
        lk = [r for r, v in tl.items() if len(v) == 1 and v[0] in leaves and int(nodes["left"][r]) < 0]
        if (F["bmax"][lk] > F["bmax"][rel]).any() or (F["bmin"][lk] < F["bmin"][rel]).any():
            rep.tlas.append(("node", rel))
    return rep


# ------------------------------------------------------------------ 2. running error arithmetic
class E:
    """Arrays of float32 quantities: v their float64 model value, e a bound on |float32 value - v|."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    def __getitem__(self, i):
        return E(self.v[i], self.e[i])


def _r(v, e):
    return E(v, e + U24 * np.abs(v))


def add(a, b):
    return _r(a.v + b.v, a.e + b.e)


def sub(a, b):
    return _r(a.v - b.v, a.e + b.e)


def mul(a, b):
    return _r(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)


def div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = a.v / b.v
        den = np.maximum(np.abs(b.v) - b.e, 0.0)
        e = (a.e + np.abs(v) * b.e) / den
    return _r(v, np.where(np.isfinite(e), e, np.inf))


def sqrt0(a):
    """sqrt(max(a, 0))"""
    v = np.sqrt(np.maximum(a.v, 0.0))
    hi = np.sqrt(np.maximum(a.v + a.e, 0.0))
    lo = np.sqrt(np.maximum(a.v - a.e, 0.0))
    return _r(v, np.maximum(hi - v, v - lo))


def sqrt_(a):
    return sqrt0(a)


def absE(a):
    return E(np.abs(a.v), a.e)


def maxE(a, b):
    return E(np.maximum(a.v, b.v), np.maximum(a.e, b.e))


def dot3(a, b):
    return add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]))


def sub3(a, b):
    return [sub(a[k], b[k]) for k in range(3)]


def const3(x):
    x = np.asarray(x, np.float64)
    return [E(x[..., k]) for k in range(3)]


def open_cmp(a, b):
    """a ? b cannot be decided within the bounds"""
    return np.abs(a.v - b.v) <= a.e + b.e


def cos_sub_clamped(sa, ca, sb, cb):
    f = add(mul(ca, cb), mul(sa, sb))
    clamp = ca.v > cb.v
    o = open_cmp(ca, cb)
    v = np.where(clamp, 1.0, f.v)
    e = np.where(clamp, 0.0, f.e)
    e = np.where(o, np.maximum(e, np.abs(1.0 - f.v) + f.e), e)  # continuous across the clamp
    return E(v, e)


def sin_sub_clamped(sa, ca, sb, cb):
    f = sub(mul(sa, cb), mul(ca, sb))
    clamp = ca.v > cb.v
    o = open_cmp(ca, cb)
    v = np.where(clamp, 0.0, f.v)
    e = np.where(clamp, 0.0, f.e)
    e = np.where(o, np.maximum(e, np.abs(f.v) + f.e), e)
    return E(v, e)


def importance(p, n, F, k, mutant=None):
    """Importance(p, n, LightNodes[k]) for arrays of nodes k: (E importance, marginal mask)."""
    one, two, half = E(np.ones(len(k))), E(np.full(len(k), 2.0)), E(np.full(len(k), 0.5))
    q = E(np.full(len(k), 32767.0))
    cos_o = sub(mul(two, div(E(F["lo"][k]), q)), one)
    thr_bits = F["lo"][k] if mutant == "cos_e_low_half" else F["hi"][k]
    cos_e = sub(mul(two, div(E(thr_bits), q)), one)
    bmax, bmin = const3(F["bmax"][k]), const3(F["bmin"][k])
    pc = [mul(add(bmax[c], bmin[c]), half) for c in range(3)]
    dp = sub3(p, pc)
    p_diff = dot3(dp, dp)
    ext = sub3(bmax, bmin)
    floor_ = mul(sqrt_(dot3(ext, ext)), half)
    d2 = p_diff if mutant == "d2_no_floor" else maxE(p_diff, floor_)
    s = sqrt_(p_diff)
    wi = [div(sub(pc[c], p[c]), s) for c in range(3)]
    wv = oct_decode(F["w"][k].astype(np.uint32))
    w = [E(wv[:, c], 4 * U24) for c in range(3)]
    cos_w = absE(dot3(w, wi))
    sin_w = sqrt0(sub(one, mul(cos_w, cos_w)))
    r = sub3(bmax, pc)
    radius = dot3(r, r)  # (the float32 midpoint of a box lies inside it: `inside` holds)
    inside_ball = p_diff.v < radius.v
    marginal = open_cmp(p_diff, radius)
    cb = sqrt0(sub(one, div(radius, p_diff)))
    cos_b = E(np.where(inside_ball, -1.0, cb.v), np.where(inside_ball, 0.0, cb.e))
    sin_b = sqrt0(sub(one, mul(cos_b, cos_b)))
    sin_o = sqrt0(sub(one, mul(cos_o, cos_o)))
    cos_x = cos_sub_clamped(sin_w, cos_w, sin_o, cos_o)
    sin_x = sin_sub_clamped(sin_w, cos_w, sin_o, cos_o)
    cos_p = cos_sub_clamped(sin_x, cos_x, sin_b, cos_b)
    cut = cos_p.v <= cos_e.v
    marginal |= open_cmp(cos_p, cos_e)
    imp = div(mul(E(F["phi"][k]), cos_p), d2)
    cos_i = dot3(wi, n)
    sin_i = sqrt0(sub(one, mul(cos_i, cos_i)))
    imp = mul(imp, cos_sub_clamped(sin_i, cos_i, sin_b, cos_b))
    marginal |= ~cut & (np.abs(imp.v) <= imp.e)  # zero or not decides the dead end: the sign must be certain
    imp = E(np.maximum(imp.v, 0.0), np.where(imp.v > 0, imp.e, 0.0))
    marginal |= ~np.isfinite(imp.v) | ~np.isfinite(imp.e)
    return E(np.where(cut, 0.0, imp.v), np.where(cut, 0.0, imp.e)), marginal


def random_x(samdim, pixel, frames, max_bounce, cur_bounce, y=False):
    pixel = np.asarray(pixel, np.uint64)
    seed = ((pixel * 258 + np.asarray(samdim, np.uint64)) * np.uint64(max_bounce + 1) + np.uint64(cur_bounce)) & np.uint64(0xFFFFFFFF)
    h = P.pcg_hash(seed)
    fr = (np.asarray(frames, np.uint64) + np.uint64(0xDEADBEEF if y else 0)) & np.uint64(0xFFFFFFFF)
    x = P.hash_with(fr, h)
    return (np.asarray(x, np.uint64).astype(np.float32) * np.uint32(0x2F7FFFFF).view(np.float32)).astype(np.float64)


def _abs_cofactor_bounds(W):
    """inverse(W) in float64 and a bound on the float32 cofactor inverse's error per entry: every cofactor is six
    triple products and five sums, the determinant four more products and three sums, then one reciprocal and one
    product: 12 roundings at most on the sum of the terms' magnitudes."""
    import itertools
    W = np.asarray(W, np.float64)
    inv = np.linalg.inv(W)
    A = np.abs(W)
    absdet = sum(np.prod([A[i, p[i]] for i in range(4)]) for p in itertools.permutations(range(4)))
    det = np.linalg.det(W)
    err = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            rows = [r for r in range(4) if r != j]
            cols = [c for c in range(4) if c != i]
            absc = sum(np.prod([A[rows[a], cols[p[a]]] for a in range(3)]) for p in itertools.permutations(range(3)))
            err[i, j] = 12 * U24 * (absc / abs(det) + abs(inv[i, j]) * absdet / abs(det)) + U24 * abs(inv[i, j])
    return inv, err


@dataclass
class PinReport:
    n: int = 0
    hits: int = 0
    marginal: int = 0
    found: int = 0
    dead_ends: int = 0
    emitted: int = 0
    worst_weight: float = 0.0
    worst_geometry: float = 0.0
    failures: list = field(default_factory=list)

    @property
    def ok(self):
        return not self.failures and self.marginal <= MARGINAL_CAP * max(self.n, 1)

    def lines(self):
        return [f"rays {self.n} hits {self.hits} marginal {self.marginal} found {self.found} dead ends {self.dead_ends} "
                f"emitted {self.emitted}",
                f"worst weight fraction {self.worst_weight:.3f} worst geometry fraction {self.worst_geometry:.3f}",
                "failures " + "; ".join(self.failures[:8])]


def pin(case, rays, bounce, far, frames, max_bounce, samples, shadow, frame_pixels=0, mutant=None, negative_t=False) -> PinReport:
    """rays: the n traced records; samples: n rows; shadow: the emitted rays."""
    rep = PinReport(n=len(rays))
    scene, lights = case.scene, case.lights
    F = node_fields(lights.nodes)
    t32 = rays["hits"][:, 2].copy().view(np.float32)
    hit = (t32 < np.float32(far)) & (rays["hits"][:, 1] < 0x80000000) & (rays["hits"][:, 0] < len(scene.meshdata))
    miss_ok = (samples["light_tri"][~hit] == -1) & (samples["steps"][~hit] == 0) & (samples["weight"][~hit] == 0)
    if not miss_ok.all():
        rep.failures.append("a miss carries a sample")
    idx = np.nonzero(hit)[0]
    rep.hits = len(idx)
    if len(idx) == 0:
        if len(shadow):
            rep.failures.append("rays emitted without hits")
        return rep
    s = rays[idx]
    o, d = s["origin"].astype(np.float64), s["direction"].astype(np.float64)
    t = t32[idx].astype(np.float64)
    pos = o + d * t[:, None]
    e_pos = 0.5 * (P.ulp32(d * t[:, None]) + P.ulp32(pos))
    mesh, tri = s["hits"][:, 0].astype(np.int64), s["hits"][:, 1].astype(np.int64)
    nm = P.restated_normals(scene.tris, scene.meshdata, mesh, tri, s["hits"][:, 3])
    dus = (d * nm.us).sum(1)
    flipped = dus > 0
    marginal = nm.marginal | (np.abs(dus) <= (nm.tol_us + 4 * U24) * np.linalg.norm(d, axis=1))
    g = np.where(flipped[:, None], -nm.g, nm.g)
    us = np.where(flipped[:, None], -nm.us, nm.us)
    codes, valid, slack = P.oct_round_trip(g, nm.tol_g)
    # the float32 code may be a neighbour of the float64 one (an axis-aligned normal sits on a rounding tie): the
    # normal is the float64 code's, with a bound that reaches every code the float32 chain may have produced
    norm = oct_decode(codes[:, 0])
    alt = np.stack([oct_decode(codes[:, j]) for j in range(1, 4)], 1)
    e_norm = 4 * U24 + slack[:, None] + np.where(valid[:, 1:, None], np.abs(alt - norm[:, None, :]), 0.0).max(1)
    px = s["PixelIndex"].astype(np.uint64)
    fr = np.full(len(idx), frames, np.uint64)
    if frame_pixels:
        fr = fr + px // np.uint64(frame_pixels)
        px = px % np.uint64(frame_pixels)
    # per light mesh: W2L, the float64 inverse and the float32 inverse's bound, Scale
    lm = lights.meshes
    W_all = P.w2l_rows(scene.meshdata)
    inv_of, inv_err, scale_of = {}, {}, {}
    for m in np.unique(lm["LockedMeshIndex"]):
        inv, err = _abs_cofactor_bounds(W_all[m])
        inv_of[m], inv_err[m] = inv, err
        col = np.sqrt((inv[:3, :3] ** 2).sum(0))
        col_e = np.sqrt((err[:3, :3] ** 2).sum(0)) + 4 * U24 * col
        x = 1.0 / col
        rel = col_e / col + U24 * (4 + 3 * np.abs(np.log2(x)))
        scale_of[m] = (x * x, 2 * rel * x * x + 4 * U24 * x * x)
    n_r = len(idx)
    p_w = [E(pos[:, c], e_pos[:, c]) for c in range(3)]
    n_w = [E(norm[:, c], e_norm[:, c]) for c in range(3)]
    p_l = [E(np.zeros(n_r)) for _ in range(3)]
    n_l = [E(np.zeros(n_r)) for _ in range(3)]
    left = np.full(n_r, F["left"][0])
    off = np.zeros(n_r, np.int64)
    start = np.zeros(n_r, np.int64)
    in_mesh = np.zeros(n_r, bool)
    active = ~marginal
    result = np.full(n_r, -1, np.int64)
    mesh_idx = np.full(n_r, -1, np.int64)
    reps = np.zeros(n_r, np.int64)
    wv, we = np.ones(n_r), np.zeros(n_r)
    for _ in range(tthip.TT_LIGHT_MAX_REPS):
        if not active.any():
            break
        reps[active] += 1
        a = np.nonzero(active & (left >= 0))[0]
        if len(a):
            first = left[a] + (0 if mutant == "no_node_offset" else off[a])
            first = np.clip(first, 0, len(lights.nodes) - 2)
            pa = [E(np.where(in_mesh[a], p_l[c].v[a], p_w[c].v[a]), np.where(in_mesh[a], p_l[c].e[a], p_w[c].e[a])) for c in range(3)]
            na = [E(np.where(in_mesh[a], n_l[c].v[a], n_w[c].v[a]), np.where(in_mesh[a], n_l[c].e[a], n_w[c].e[a])) for c in range(3)]
            cx, mx = importance(pa, na, F, first, mutant)
            cy, my = importance(pa, na, F, first + 1, mutant)
            m = mx | my
            dead = ~m & (cx.v == 0) & (cy.v == 0)
            tot = add(cx, cy)
            ratio = div(cx, tot)
            sam = 264 + (0 if mutant == "reps_const" else reps[a])
            u = random_x(sam, px[a], fr[a], max_bounce, bounce)
            # twin children (every field but `left` equal) have bit-identical importances x: x + x and x / (x + x)
            # are exact, the ratio is 0.5 with no error, and the decision against it is certain even at u = 0.5
            nd = lights.nodes
            twin = np.ones(len(first), bool)
            for fld in ("BBMax", "BBMin", "w", "phi", "cosTheta_oe"):
                eq = nd[fld][first] == nd[fld][first + 1]
                twin &= eq.all(1) if eq.ndim > 1 else eq
            twin &= ~dead & ~m & (cx.v > 0) & np.isfinite(cx.v)
            ratio = E(np.where(twin, 0.5, ratio.v), np.where(twin, 0.0, ratio.e))
            m |= ~dead & ~twin & ~(np.abs(u - ratio.v) > ratio.e)
            pick = (u > ratio.v) if mutant == "gt" else (u >= ratio.v)
            taken = E(np.where(pick, cy.v, cx.v), np.where(pick, cy.e, cx.e))
            prob = div(taken, tot)
            W_ = E(wv[a], we[a])
            nw = mul(W_, prob) if mutant == "weight_mul" else div(W_, prob)
            go = ~m & ~dead
            wv[a[go]], we[a[go]] = nw.v[go], nw.e[go]
            left[a[go]] = F["left"][first[go] + pick[go]]
            marginal[a[m]] = True
            active[a[m | dead]] = False
        b = np.nonzero(active & (left < 0))[0]
        b = np.setdiff1d(b, a)  # a lane that just stepped looks at its new node in the next iteration
        if len(b):
            fin = b[in_mesh[b]]
            result[fin] = -(left[fin] + 1) + (0 if mutant == "no_start_index" else start[fin])
            active[fin] = False
            tr = b[~in_mesh[b]]
            if len(tr):
                row = lm[-(left[tr] + 1)]
                start[tr] = row["StartIndex"]
                mi = row["LockedMeshIndex"].astype(np.int64)
                mesh_idx[tr] = mi
                for m_ in np.unique(mi):
                    sel = tr[mi == m_]
                    Wm = W_all[m_]
                    pw = [p_w[c][sel] for c in range(3)]
                    nw_ = [n_w[c][sel] for c in range(3)]
                    rows_p, rows_n = [], []
                    for r_ in range(3):
                        cW = [E(np.full(len(sel), Wm[r_, c])) for c in range(4)]
                        rows_p.append(add(add(add(mul(cW[0], pw[0]), mul(cW[1], pw[1])), mul(cW[2], pw[2])), cW[3]))
                        rows_n.append(add(add(mul(cW[0], nw_[0]), mul(cW[1], nw_[1])), mul(cW[2], nw_[2])))
                    sc_v, sc_e = scale_of[m_]
                    if mutant == "no_scale":
                        sc_v, sc_e = np.ones(3), np.zeros(3)
                    tn = [div(rows_n[c], E(np.full(len(sel), sc_v[c]), sc_e[c])) for c in range(3)]
                    if mutant == "normal_untransformed":
                        tn = nw_
                    ln = sqrt_(dot3(tn, tn))
                    for c in range(3):
                        q = div(tn[c], ln)
                        p_l[c].v[sel], p_l[c].e[sel] = rows_p[c].v, rows_p[c].e
                        n_l[c].v[sel], n_l[c].e[sel] = q.v, q.e
                off[tr] = scene.meshdata["LightNodeOffset"][mi]
                left[tr] = F["left"][off[tr]]
                in_mesh[tr] = True
    sm = samples[idx]
    firm = ~marginal
    rep.marginal = int(marginal.sum())
    found = firm & (result >= 0)
    rep.found, rep.dead_ends = int(found.sum()), int((firm & (result < 0)).sum())
    if (sm["light_tri"][firm] != result[firm]).any():
        bad = np.nonzero(firm & (sm["light_tri"] != result))[0]
        rep.failures.append(f"{len(bad)} rays end elsewhere, first ray {idx[bad[0]]}: sample {sm['light_tri'][bad[0]]} model {result[bad[0]]}")
    if (sm["steps"][firm] != reps[firm]).any():
        rep.failures.append("steps differ from Reps at return")
    if (sm["mesh_index"][firm] != mesh_idx[firm]).any():
        rep.failures.append("mesh_index differs")
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.abs(sm["weight"].astype(np.float64) - wv) / (we + U24 * np.abs(wv))
    frac = np.where(firm, frac, 0.0)
    rep.worst_weight = float(np.nanmax(frac)) if len(frac) else 0.0
    if (frac > 1).any() or np.isnan(frac[firm]).any():
        rep.failures.append(f"weight outside its bound ({rep.worst_weight:.3g} of it)")
    # ---- geometry of the chosen light and of the emitted ray (firm, found rays)
    f = np.nonzero(found & (sm["light_tri"] == result))[0]
    worst = 0.0
    expected_emit = np.zeros(n_r, bool)
    open_emit = np.zeros(n_r, bool)
    if len(f):
        LT = lights.tris[result[f]]
        mi = mesh_idx[f]
        r1 = random_x(79, px[f], fr[f], max_bounce, bounce).astype(np.float32)
        r2 = random_x(79, px[f], fr[f], max_bounce, bounce, y=True).astype(np.float32)
        if mutant == "rand79_swapped":
            r1, r2 = r2, r1
        first_branch = (r2 > r1) if mutant != "sample_triangle_swapped" else ~(r2 > r1)
        h = np.float32(0.5)
        u1 = np.where(first_branch, r1 * h, r1 - r2 * h).astype(np.float32)
        u2 = np.where(first_branch, r2 - r1 * h, r2 * h).astype(np.float32)
        local = LT["pos0"].astype(np.float64) + LT["posedge1"].astype(np.float64) * u1[:, None].astype(np.float64) \
            + LT["posedge2"].astype(np.float64) * u2[:, None].astype(np.float64)
        agg = LT["TriTarget"].astype(np.int64) + scene.meshdata["TriOffset"][mi]
        if (sm["agg_tri"][f] != agg).any():
            rep.failures.append("agg_tri differs")
        T = scene.tris[agg]
        inv = np.stack([inv_of[m_] for m_ in mi])
        ierr = np.stack([inv_err[m_] for m_ in mi])
        e1, e2 = T["posedge1"].astype(np.float64), T["posedge2"].astype(np.float64)
        wpos = np.einsum("nij,nj->ni", inv[:, :3, :3], local) + inv[:, :3, 3]
        mag = np.einsum("nij,nj->ni", np.abs(inv[:, :3, :3]), np.abs(local)) + np.abs(inv[:, :3, 3])
        tol_pos = 8 * U24 * mag + np.einsum("nij,nj->ni", ierr[:, :3, :3], np.abs(local)) + ierr[:, :3, 3] + 4 * U24 * np.abs(local).max(1)[:, None]
        gp = np.abs(sm["position"][f].astype(np.float64) - wpos) / tol_pos
        worst = max(worst, float(gp.max()))
        if (gp > 1).any():
            rep.failures.append(f"position off its triangle point ({gp.max():.3g} of the bound)")
        a1 = np.einsum("nij,nj->ni", inv[:, :3, :3], e1)
        a2 = np.einsum("nij,nj->ni", inv[:, :3, :3], e2)
        rel_inv = (np.einsum("nij,nj->ni", ierr[:, :3, :3], np.abs(e1)).max(1) / np.linalg.norm(a1, axis=1)
                   + np.einsum("nij,nj->ni", ierr[:, :3, :3], np.abs(e2)).max(1) / np.linalg.norm(a2, axis=1))
        area = 0.5 * np.linalg.norm(np.cross(a1, a2), axis=1)
        la, lb, lc = np.linalg.norm(a1, axis=1), np.linalg.norm(a1 - a2, axis=1), np.linalg.norm(a2, axis=1)
        hs = (la + lb + lc) / 2
        cond = hs / np.minimum(np.minimum(hs - la, hs - lb), hs - lc)  # Heron's conditioning
        ga = np.abs(sm["area"][f] - area) / (area * (8 * U24 * (1 + cond) + 4 * rel_inv * (1 + cond)))
        worst = max(worst, float(ga.max()))
        if (ga > 1).any():
            rep.failures.append(f"area differs from half the cross product of the world edges ({ga.max():.3g} of the bound)")
        # inside the world triangle: barycentrics of the reported position
        wp0 = np.einsum("nij,nj->ni", inv[:, :3, :3], LT["pos0"].astype(np.float64)) + inv[:, :3, 3]
        we1 = np.einsum("nij,nj->ni", inv[:, :3, :3], LT["posedge1"].astype(np.float64))
        we2 = np.einsum("nij,nj->ni", inv[:, :3, :3], LT["posedge2"].astype(np.float64))
        rel = sm["position"][f].astype(np.float64) - wp0
        G = np.stack([np.stack([(we1 * we1).sum(1), (we1 * we2).sum(1)], 1), np.stack([(we1 * we2).sum(1), (we2 * we2).sum(1)], 1)], 1)
        bc = np.linalg.solve(G, np.stack([(rel * we1).sum(1), (rel * we2).sum(1)], 1)[:, :, None])[:, :, 0]
        tol_b = (tol_pos.max(1) / np.minimum(np.linalg.norm(we1, axis=1), np.linalg.norm(we2, axis=1))) * (1 + cond)
        if (bc[:, 0] < -tol_b).any() or (bc[:, 1] < -tol_b).any() or (bc.sum(1) > 1 + tol_b).any():
            rep.failures.append("position outside its triangle")
        # LightNorm as the text forms it: normalize(mul((float3x3)Minv, normalize(cross(e1, e2)))); unit
        ln = P._unit(np.einsum("nij,nj->ni", inv[:, :3, :3], P._unit(np.cross(e1, e2))))
        c12 = np.cross(e1, e2)
        cond_n = (np.abs(e1[:, [1, 2, 0]] * e2[:, [2, 0, 1]]) + np.abs(e1[:, [2, 0, 1]] * e2[:, [1, 2, 0]])).max(1) / np.linalg.norm(c12, axis=1)
        kap = np.array([np.linalg.cond(inv_of[m_][:3, :3]) for m_ in mi])
        tol_n = (8 * U24 * (1 + cond_n) + 2 * rel_inv) * kap + 8 * U24
        gn = np.linalg.norm(sm["normal"][f].astype(np.float64) - ln, axis=1) / tol_n
        worst = max(worst, float(gn.max()))
        if (gn > 1).any() or (np.abs(np.linalg.norm(sm["normal"][f].astype(np.float64), axis=1) - 1) > 4 * U24).any():
            rep.failures.append(f"normal is not the unit LightNorm ({gn.max():.3g} of the bound)")
        # which rays exist: SurfaceCos > 0 and bsdf_pdf > 1e-4, from the reported position and the modelled origin
        origin = pos[f] + 1e-4 * us[f]
        to = sm["position"][f].astype(np.float64) - origin
        dist = np.linalg.norm(to, axis=1)
        sc = (to / dist[:, None] * norm[f]).sum(1)
        tol_sc = 16 * U24 + e_norm[f].sum(1) + (tol_pos.max(1) + e_pos[f].max(1)) / dist
        pdf = sc / np.pi
        expected_emit[f] = (sc > 0) & (pdf > 1e-4)
        open_emit[f] = (np.abs(sc) <= tol_sc) | (np.abs(pdf - 1e-4) <= tol_sc)
    rep.worst_geometry = worst
    rep.marginal += int((open_emit & ~marginal).sum())
    sure = firm & ~open_emit
    # source order: the emitted rays are the expected sources, in order, by pixel
    src_px = s["PixelIndex"]
    exp_idx = np.nonzero(expected_emit & sure)[0]
    maybe = np.nonzero(~sure & hit[idx])[0]
    got_px = shadow["PixelIndex"]
    rep.emitted = len(shadow)
    pos_of = {}
    for k, p_ in enumerate(src_px):
        pos_of.setdefault(int(p_), []).append(k)
    cursor, order_ok, src_of = -1, True, []
    for p_ in got_px:
        cand = [k for k in pos_of.get(int(p_), []) if k > cursor]
        if not cand:
            order_ok = False
            break
        cursor = cand[0]
        src_of.append(cursor)
    if not order_ok:
        rep.failures.append("emitted rays are not in source order")
        return rep
    src_of = np.array(src_of, np.int64)
    missing = np.setdiff1d(exp_idx, src_of)
    extra = np.setdiff1d(np.setdiff1d(src_of, exp_idx), maybe)
    if len(missing) or len(extra):
        rep.failures.append(f"{len(missing)} expected rays missing, {len(extra)} unexpected rays")
        return rep
    if len(src_of) == 0:
        return rep
    # the record of every emitted ray whose source is firm
    keep = sure[src_of] & found[src_of]
    R, k = shadow[keep], src_of[keep]
    smk = sm[k]
    org = R["origin"].astype(np.float64)
    want_o = pos[k] + 1e-4 * us[k]
    tol_o = np.sqrt((e_pos[k] ** 2).sum(1)) + 1e-4 * (nm.tol_us[k] + 8 * U24) + P.ulp32(want_o).max(1)
    go = np.linalg.norm(org - want_o, axis=1) / tol_o
    if (go > 1).any():
        rep.failures.append(f"origin is not pos + 1e-4 USGNorm ({go.max():.3g} of the bound)")
    to = smk["position"].astype(np.float64) - org
    dist = np.linalg.norm(to, axis=1)
    dr = R["direction"].astype(np.float64)
    if (np.abs(np.linalg.norm(dr, axis=1) - 1) > 4 * U24).any() or (np.linalg.norm(dr - to / dist[:, None], axis=1) > 8 * U24 + 2 * P.ulp32(to).max(1) / dist).any():
        rep.failures.append("direction is not the unit vector from origin to position")
    want_t = dist - (0.0 if mutant == "t_no_offset" else np.float64(np.float32(0.01)))
    tt = R["t"].astype(np.float64) * (-1 if negative_t else 1)
    if (np.abs(tt - want_t) > 4 * P.ulp32(dist)).any():
        rep.failures.append("|t| is not distance - 0.01")
    sc = (dr * norm[k]).sum(1)
    bsdf = sc * np.float64(np.float32(0.318309886548))
    lnm, ar, wt = smk["normal"].astype(np.float64), smk["area"].astype(np.float64), smk["weight"].astype(np.float64)
    nee = (1.0 / ((np.abs((dr * lnm).sum(1)) * ar) / (dist * dist))) / wt
    illum = (bsdf / nee) * (nee * nee) / (nee * nee + bsdf * bsdf)
    cos_l = np.abs((dr * lnm).sum(1))
    # bsdf enters the value and the heuristic; it carries the normal's bound (the float32 code may be a neighbour's)
    rel_b = (e_norm[k].sum(1) + 12 * U24) / np.maximum(sc, 1e-30)
    rel_i = 32 * U24 + 3 * rel_b + 8 * U24 / np.maximum(cos_l, 1e-30)
    gi = np.abs(R["illumination"][:, 0].astype(np.float64) - illum) / (illum * rel_i)
    rep.worst_geometry = max(rep.worst_geometry, float(gi.max()) if len(gi) else 0.0)
    if (gi > 1).any() or not (R["illumination"][:, 0] == R["illumination"][:, 1]).all() or not (R["illumination"][:, 1] == R["illumination"][:, 2]).all():
        rep.failures.append(f"illumination is not (bsdf / NEE_pdf) * power_heuristic ({gi.max():.3g} of the bound)")
    code = R["LuminanceIncomming"].copy().view(np.uint32).astype(np.int64)  # unpackRGBE, CommonData.cginc:498-509
    lum = (code & 0x1FF) * 2.0 ** ((code >> 27) - 20) / 256.0
    if not ((code & 0x1FF) == ((code >> 9) & 0x1FF)).all() or not ((code & 0x1FF) == ((code >> 18) & 0x1FF)).all():
        rep.failures.append("LuminanceIncomming is not grey")
    if (np.abs(lum - bsdf) > bsdf * (2.0 ** -9 + 2.0 ** -20 + rel_b)).any():  # 9 mantissa bits on a shared exponent
        rep.failures.append("LuminanceIncomming is not packRGBE of the Lambert value")
    return rep


# ------------------------------------------------------------------ 3. selection probabilities
def leaf_probabilities(case, pos, norm):
    """Float64 probability that SampleLightBVH(pos, norm) returns each light triangle, and the mass that dead-ends:
    (p [n light triangles], p_dead). One world point; the product of the branch probabilities along each path."""
    scene, lights = case.scene, case.lights
    F = node_fields(lights.nodes)
    n_nodes = len(lights.nodes)
    W_all = P.w2l_rows(scene.meshdata)
    out = np.zeros(len(lights.tris))
    dead = [0.0]

    def imps(p, n):
        k = np.arange(n_nodes)
        pe = [E(np.full(n_nodes, p[c])) for c in range(3)]
        ne = [E(np.full(n_nodes, n[c])) for c in range(3)]
        with np.errstate(all="ignore"):
            return importance(pe, ne, F, k)[0].v

    def walk(imp, node, off, mass, leaf):
        left = int(F["left"][node])
        if left < 0:
            leaf(-(left + 1), mass)
            return
        a, b = left + off, left + off + 1
        if imp[a] == 0 and imp[b] == 0:
            dead[0] += mass
            return
        tot = imp[a] + imp[b]
        if imp[a] > 0:
            walk(imp, a, off, mass * imp[a] / tot, leaf)
        if imp[b] > 0:
            walk(imp, b, off, mass * imp[b] / tot, leaf)

    def tlas_leaf(m, mass):
        row = lights.meshes[m]
        mi = int(row["LockedMeshIndex"])
        Wm = W_all[mi]
        inv = np.linalg.inv(Wm)
        scale = (1.0 / np.sqrt((inv[:3, :3] ** 2).sum(0))) ** 2
        pl = Wm[:3, :3] @ pos + Wm[:3, 3]
        nl = (Wm[:3, :3] @ norm) / scale
        nl /= np.linalg.norm(nl)
        off = int(scene.meshdata["LightNodeOffset"][mi])
        start = int(row["StartIndex"])

        def mesh_leaf(k, mass2):
            out[start + k] += mass2

        walk(imps(pl, nl), off, off, mass, mesh_leaf)

    walk(imps(np.asarray(pos, np.float64), np.asarray(norm, np.float64)), 0, 0, 1.0, tlas_leaf)
    return out, dead[0]


def chi_square(counts, probs, min_expected=5.0):
    """(statistic, degrees of freedom) of observed counts against probabilities; bins with an expectation below
    min_expected are pooled into one."""
    counts, probs = np.asarray(counts, np.float64), np.asarray(probs, np.float64)
    n = counts.sum()
    exp = probs * n
    small = exp < min_expected
    o = np.append(counts[~small], counts[small].sum())
    e = np.append(exp[~small], exp[small].sum())
    keep = e > 0
    if (o[~keep] > 0).any():
        return np.inf, int(keep.sum()) - 1
    o, e = o[keep], e[keep]
    return float(((o - e) ** 2 / e).sum()), len(o) - 1


def chi_square_limit(dof, alpha=0.001):
    """The Wilson-Hilferty limit k (1 - 2 / (9 k) + z sqrt(2 / (9 k)))^3 with z = 3.0902 at alpha = 0.001 (the normal
    quantile); within a percent of the exact quantile from 3 degrees of freedom on."""
    assert alpha == 0.001
    z, k = 3.0902, float(dof)
    return k * (1 - 2 / (9 * k) + z * np.sqrt(2 / (9 * k))) ** 3
