"""Float64 model of the ray producers and of the normal resolve (test infrastructure: numpy only, no GPU, no
oracle): Generate (tt_generate_kernel), the triangle branch of the normal resolve (tt_resolve_kernel) and the
triangle branch of the diffuse-bounce enqueue (tt_bounce_kernel<false>). Nothing here passes through
oracle/tt_oracle.c; the random numbers are restated in integer arithmetic and are exact, everything geometric is
float64 and is compared within bounds derived below (u = 2^-24, the unit roundoff of float32).

Random numbers. pcg_hash, hash_with and random() (the non-ASVGF branch) in uint64 masked to 32 bits; random() is
float32(hash) * float32(bits 0x2f7fffff), one correctly rounded conversion and one correctly rounded product, which
numpy's float32 reproduces bit for bit. With frame_pixels = n a ray with PixelIndex p draws at pixel p mod n and
frame frames + p // n.

Generate, from the camera's parameters (position, forward, up, vertical fov, aspect, lens shift), never from the
matrices: v = f + (uvx + sx) A r + (uvy + sy) B u with B = tan(fov / 2), A = aspect B, r = up x f, u = f x r
(Unity's left-handed frame), uv = (pixel + jitter) / (W, H) * 2 - 1, direction v / |v|, origin position + near *
direction. The jitter is random(0, pixel) - 0.5: the footprint is centred on the pixel's corner, as in the
reference (kept departure). Float32 chain of the direction: uv 3 roundings (add, divide, subtract); the camera-space
components 5 (two rounded matrix entries, product, add, and the uv error passes through); the rotation 4 per
component on a sum of three terms, at most 4 sqrt(3) on the vector; normalize 4 (fused dot, sqrt, reciprocal,
product): 3 + 5 + 7 + 4 = 19, K_GEN = 20 with one for slack. They act on the terms' magnitudes, and the uv
error is absolute on 1 + |uv| (the subtraction of 1 cancels in mid-screen): S = |(1, A (1 + |uvx| + |sx|),
B (1 + |uvy| + |sy|))|, so |direction32 - direction64| <= K_GEN u S / |v|. Origin: the rounded position, the
product and the add, 1.5 ulp(|origin|) per component, plus near times the direction's bound; ORIGIN_ULPS = 2.

Normals of a triangle record, three models.
  restated: the shader chain in float64 -- i_octahedral_32 of the three packed normals, u and v from the packed
    16:16 barycentrics, w0 = 1 - u - v, transpose(W2L 3x3) (the float32 entries as stored), normalize; the
    unsmoothed normal -normalize(W2L^T cross(normalize e1, normalize e2)) turned to the smooth normal's side.
    Float32 chain of the smooth normal: each decoded normal 8 (divide, subtract, two for z, the fold, normalize 4 --
    absolute, on components <= 1), the weights 3, the interpolation 5: 16 roundings on the sum of |terms|; the
    matrix product 3 on its own sum of |terms|; normalize 4. With cond_i = |sum |w_k| |n_k|| / |n_i| (cancellation
    of the interpolation), amp = ||W||_2 |n_i| / |W^T n_i| (what the matrix does to an error of n_i) and cond_m =
    ||W|^T |n_i|| / |W^T n_i| (cancellation of the product): |g32 - g64| <= K_NORMAL u (cond_i amp + cond_m + 1),
    K_NORMAL = 16. The unsmoothed normal likewise with cond_x of the cross product (two normalizes 8, cross 2: 10
    roundings on the sum of |terms| of the cross) in the place of cond_i. A hit whose number cond_i amp + cond_m
    (or cond_x amp + cond_m) exceeds COND_MAX = 1000 is marginal (its bound would exceed 1e-3).
  geometric: the face normal from the world corners, cross(L2W e1, L2W e2) with L2W = inv(W2L) in float64; the
    transpose of W2L never enters. Its sign is the smooth normal's, as the shader fixes it (so a mirrored
    record, where W2L^T cross(e1, e2) points against the cross product of the world edges, is covered).
  analytic: a unit sphere whose vertex normals are its positions, placed by L2W = T R S. The smooth normal at the
    world hit point p is normalize(R S^-2 R^T (p - c)), from the TRS parameters alone. The model leaves the packed
    data: bound = kappa (e_oct + e_bary + e_pos / min|s|) / |x|, kappa = max|s| / min|s|, x the local point;
    e_oct = sqrt(18) / 32767.5 (a mesh's vertex normals are packed by truncation, as CommonFunctions.PackOctahedral
    does: up to one 16:16 grid step per coordinate, sqrt(6) on the decoded vector, sqrt(3) from its normalisation;
    the shading-side round trip rounds and has half of it, E_OCT_HALF), e_bary = (|e1| + |e2|) / 65535 (one
    1/65535 step in u and in v), e_pos = 8 ulp(|o| + |t|) (the hit point's own float32 error in object space).

Bounce. pos = o + d t; both normals negated where d . us > 0 (marginal where |d . us| is within the bound of us);
norm = the 16:16 octahedral round trip of the smooth normal in float64 with round-half-even. The float32 value
that is rounded, 32767.5 + x 32767.5, carries 32767.5 (bound of g + 4 u) + 2^-8 (its own ulp below 65536), far
more than a float64 tie-break can decide; so where a coordinate lies that close to a half both codes are
candidates (at most four per ray), and a check on norm passes if one candidate passes. Nothing is left open by
this. On the octahedron's fold (z < 0 and x or y within the bound e of 0) the code jumps with the sign of that
component, but both codes decode to normals whose component is +-|x| / (|x| + |y| + |z|): they differ by at most 2 e,
which is added to the bounds on norm there (norm_slack); nothing is left open.
omega_o = (r cos phi, sqrt(|1 - r^2|), r sin phi) with true sin / cos, from the exact random numbers: a = 2 rx - 1,
b = 2 ry - 1, zero replaced by 1e-5, r = a or b (the larger square), phi as sample_disc. sqrt(abs(...)) follows the
reference (kept departure). omega_o.y depends on r^2 = max(a^2, b^2) alone. Float32: sincos_pinned is within 5 u
(tests/test_enqueue.py), so dx^2 + dz^2 = r^2 (1 + e), |e| <= 14 u + 7 u (five products and adds), the subtraction
and the root 2 more: |om.y32 - om.y64| <= 12 u r^2 / om.y + 2 u; a ray with 1 - r^2 <= 24 u has a marginal pdf.
direction = omega_o in an orthonormal frame about norm; only azimuth-free quantities are compared:
  |direction| = 1                        4 u (normalize)
  direction . norm = last_pdf pi         K_FRAME u + 3 u: the decoded norm 8, T . norm 2, B . norm 3, lengths 8, the
                                         combination 5, normalize 4, the model's own decode against the kernel's 8:
                                         38, K_FRAME = 40; the pdf's product and pi 3
  direction . norm = sqrt(|1 - r^2|)     K_FRAME u + the bound of om.y
  direction_i . direction_j = omega_i . omega_j for two rays of one norm code: 2 K_FRAME u + 28 u + both om.y bounds
  origin: (origin' - pos) . n = 1e-4 with n the geometric normal on the side the ray came from, within
          |e|_2 + 1e-4 (bound of us + 8 u), e per component 0.5 ulp(d t) + 0.5 ulp(pos) + 0.5 ulp(origin').
|norm.x| within roundings of 0.99 only picks GetTangentSpace's other helper, the frame's azimuth: no comparison reads it
(the pair check takes rays of one norm code, hence of one helper), so such rays need no class of their own.
pdf = omega_o.y / pi, hits copied, PixelIndex kept; survivors t < far, (int) triangle_id >= 0, pdf > 0 in source order.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

U24 = 2.0 ** -24
K_GEN = 20
ORIGIN_ULPS = 2
K_NORMAL = 16
COND_MAX = 1000.0
K_FRAME = 40
OFFSET = 1e-4
E_OCT = np.sqrt(18.0) / 32767.5
E_OCT_HALF = E_OCT / 2
_M = np.uint64(0xFFFFFFFF)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


# ------------------------------------------------------------------ random numbers (exact)
def pcg_hash(seed):
    s = np.asarray(seed, np.uint64) & _M
    state = (s * np.uint64(747796405) + np.uint64(2891336453)) & _M
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & _M
    return (word >> np.uint64(22)) ^ word


def hash_with(seed, h):
    s = ((np.asarray(seed, np.uint64) & _M) ^ np.uint64(61)) ^ h
    s = (s + (s << np.uint64(3))) & _M
    s = s ^ (s >> np.uint64(4))
    return (s * np.uint64(0x27D4EB2D)) & _M


def random2(samdim, pixel, frames, max_bounce, cur_bounce, frame_pixels=0):
    """random(samdim, pixel) as float32 (rx, ry), bit for bit. frames: the int32 frames_accumulated."""
    px = np.asarray(pixel, np.uint64) & _M
    fr = np.full(px.shape, int(frames) & 0xFFFFFFFF, np.uint64)
    if frame_pixels:
        j = px // np.uint64(frame_pixels)
        px = px - j * np.uint64(frame_pixels)
        fr = (fr + j) & _M
    h = pcg_hash((px * np.uint64(258) + np.uint64(samdim)) * np.uint64(max_bounce + 1) + np.uint64(cur_bounce))
    k = np.array([0x2F7FFFFF], np.uint32).view(np.float32)[0]
    rx = hash_with(fr, h).astype(np.float32) * k
    ry = hash_with((fr + np.uint64(0xDEADBEEF)) & _M, h).astype(np.float32) * k
    return rx, ry


# ------------------------------------------------------------------ Generate
@dataclass(frozen=True)
class Camera:
    position: tuple
    forward: tuple
    up: tuple
    vfov_deg: float
    shift: tuple = (0.0, 0.0)
    near: float = 0.05
    far: float = 1000.0

    def basis(self):
        f = _unit(np.asarray(self.forward, np.float64))
        r = _unit(np.cross(np.asarray(self.up, np.float64), f))
        return r, np.cross(f, r), f


@dataclass
class GenExpect:
    direction: np.ndarray
    origin: np.ndarray
    tol_d: np.ndarray
    tol_o: np.ndarray
    jitter: np.ndarray   # (n, 2), the exact random(0, pixel) - 0.5 (zeros without jitter)


def generate(cam: Camera, W, H, jitter=0, frames=0, max_bounce=3, aspect=None) -> GenExpect:
    n = W * H
    p = np.arange(n)
    x, y = (p % W).astype(np.float64), (p // W).astype(np.float64)
    j = np.zeros((n, 2))
    if jitter:
        rx, ry = random2(0, p, frames, max_bounce, 0)
        j = np.stack([rx.astype(np.float64) - 0.5, ry.astype(np.float64) - 0.5], 1)
    uvx, uvy = (x + j[:, 0]) / W * 2 - 1, (y + j[:, 1]) / H * 2 - 1
    r, u, f = cam.basis()
    B = np.tan(np.deg2rad(cam.vfov_deg) / 2)
    A = (W / H if aspect is None else aspect) * B
    sx, sy = cam.shift
    v = f[None, :] + ((uvx + sx) * A)[:, None] * r[None, :] + ((uvy + sy) * B)[:, None] * u[None, :]
    vn = np.sqrt((v * v).sum(1))
    d = v / vn[:, None]
    S = np.sqrt(1 + (A * (1 + np.abs(uvx) + abs(sx))) ** 2 + (B * (1 + np.abs(uvy) + abs(sy))) ** 2)
    tol_d = K_GEN * U24 * S / vn
    o = np.asarray(cam.position, np.float64)[None, :] + cam.near * d
    tol_o = ORIGIN_ULPS * np.sqrt(3.0) * ulp32(np.abs(o).max(1)) + cam.near * tol_d
    return GenExpect(d, o, tol_d, tol_o, j)


def screen_jitter(cam: Camera, W, H, directions, aspect=None):
    """The sub-pixel offsets (n, 2) a set of W H camera directions was drawn with, from the camera's parameters."""
    r, u, f = cam.basis()
    d = np.asarray(directions, np.float64)
    B = np.tan(np.deg2rad(cam.vfov_deg) / 2)
    A = (W / H if aspect is None else aspect) * B
    z = d @ f
    uvx, uvy = (d @ r) / z / A - cam.shift[0], (d @ u) / z / B - cam.shift[1]
    p = np.arange(W * H)
    return np.stack([(uvx + 1) / 2 * W - p % W, (uvy + 1) / 2 * H - p // W], 1)


# ------------------------------------------------------------------ octahedral codes
def oct_decode(code):
    code = np.asarray(code, np.uint32)
    vx = (code & 65535).astype(np.float64) / 32767.5 - 1.0
    vy = (code >> 16).astype(np.float64) / 32767.5 - 1.0
    z = 1.0 - np.abs(vx) - np.abs(vy)
    t = np.maximum(-z, 0.0)
    return _unit(np.stack([vx + np.where(vx > 0, -t, t), vy + np.where(vy > 0, -t, t), z], -1))


def oct_encode_pre(n):
    """The two values octahedral_32 rounds, 32767.5 + (x, y) 32767.5, in float64."""
    n = np.asarray(n, np.float64)
    sx, sy = np.where(n[..., 0] >= 0, 1.0, -1.0), np.where(n[..., 1] >= 0, 1.0, -1.0)
    den = n[..., 0] * sx + n[..., 1] * sy + np.abs(n[..., 2])
    x, y = n[..., 0] / den, n[..., 1] / den
    neg = ~(n[..., 2] >= 0)
    x, y = np.where(neg, (1 - y * sy) * sx, x), np.where(neg, (1 - x * sx) * sy, y)
    return 32767.5 + x * 32767.5, 32767.5 + y * 32767.5


def oct_round_trip(n, tol):
    """The codes octahedral_32 may give a float32 normal within `tol` of n: (codes (k, 4) uint32, valid (k, 4),
    slack (k,): what the fold adds to a bound on the decoded normal). Column 0 is the float64 round-half-even code."""
    fx, fy = oct_encode_pre(n)
    delta = 32767.5 * (np.asarray(tol) + 4 * U24) + 2.0 ** -8
    cols = []
    for f in (fx, fy):
        c0 = np.rint(f)
        other = np.where(f >= c0, c0 + 1, c0 - 1)
        near = np.abs(np.abs(f - c0) - 0.5) <= delta
        cols.append((c0, np.clip(other, 0, 65535), near))
    (x0, x1, nx), (y0, y1, ny) = cols
    codes = np.stack([x0 + 65536 * y0, x1 + 65536 * y0, x0 + 65536 * y1, x1 + 65536 * y1], 1).astype(np.uint32)
    valid = np.stack([np.ones_like(nx), nx, ny, nx & ny], 1)
    n = np.asarray(n, np.float64)
    lim = np.asarray(tol) + 4 * U24
    slack = np.where((n[:, 2] < 0) & ((np.abs(n[:, 0]) <= lim) | (np.abs(n[:, 1]) <= lim)), 2 * lim, 0.0)
    return codes, valid, slack


# ------------------------------------------------------------------ normals
def w2l_rows(meshdata):
    """The mesh records' W2L as (n, 4, 4) row-major float64 (the float32 entries as stored)."""
    return meshdata["W2L"].astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)


def _apply(M, x):
    return np.einsum("nij,nj->ni", M, x)


def _matrix(W, form):
    if form == "inverse transpose":   # mul_inv: transpose(W2L 3x3)
        return W[:, :3, :3].transpose(0, 2, 1)
    if form == "W2L":
        return W[:, :3, :3]
    assert form == "L2W"
    return np.linalg.inv(W)[:, :3, :3]


@dataclass
class Normals:
    g: np.ndarray        # smooth normal
    us: np.ndarray       # unsmoothed normal on the smooth normal's side
    tol_g: np.ndarray
    tol_us: np.ndarray
    cond: np.ndarray     # the larger conditioning number of the two
    side: np.ndarray     # us . g before the sign was fixed (0 within tol: the sign is open)

    @property
    def marginal(self):
        return (self.cond > COND_MAX) | (np.abs(self.side) <= self.tol_g + self.tol_us)


def restated_normals(tris, meshdata, mesh, tri, uvcode, form="inverse transpose") -> Normals:
    """The shader chain in float64 for records (mesh, tri, packed uv). form: the matrix applied to both normals --
    "inverse transpose" is the shader's; "W2L" and "L2W" are the control mutants."""
    T = tris[np.asarray(tri, np.int64)]
    W = w2l_rows(meshdata)[np.asarray(mesh, np.int64)]
    M = _matrix(W, form)
    code = np.asarray(uvcode, np.uint32)
    u, v = (code & 0xFFFF) / 65535.0, (code >> 16) / 65535.0
    w = np.stack([1.0 - u - v, u, v], 1)
    nk = np.stack([oct_decode(T["norms"][:, k]) for k in range(3)], 1)          # (n, 3 corners, 3)
    ni = (w[:, :, None] * nk).sum(1)
    lni = np.sqrt((ni * ni).sum(1))
    absum = (np.abs(w)[:, :, None] * np.abs(nk)).sum(1)
    cond_i = np.sqrt((absum * absum).sum(1)) / lni
    s2 = np.linalg.norm(M, 2, axis=(1, 2))

    def through(x, cond_in):
        y = _apply(M, x)
        ly = np.sqrt((y * y).sum(1))
        ay = _apply(np.abs(M), np.abs(x))
        num = cond_in * s2 * np.sqrt((x * x).sum(1)) / ly + np.sqrt((ay * ay).sum(1)) / ly
        return y / ly[:, None], num

    g, num_g = through(ni, cond_i)
    a, b = _unit(T["posedge1"].astype(np.float64)), _unit(T["posedge2"].astype(np.float64))
    c = np.cross(a, b)
    ac = np.abs(a[:, [1, 2, 0]] * b[:, [2, 0, 1]]) + np.abs(a[:, [2, 0, 1]] * b[:, [1, 2, 0]])
    cond_x = np.sqrt((ac * ac).sum(1)) / np.sqrt((c * c).sum(1))
    us, num_us = through(c, cond_x)
    us = -us
    side = (us * g).sum(1)
    us = np.where(side[:, None] < 0, -us, us)
    return Normals(g, us, K_NORMAL * U24 * (num_g + 1), K_NORMAL * U24 * (num_us + 1), np.maximum(num_g, num_us), side)


def geometric_normal(tris, meshdata, mesh, tri, towards):
    """The unit normal of the world triangle, cross product of its world edges, on the side of `towards`; and
    a world corner of the triangle."""
    T = tris[np.asarray(tri, np.int64)]
    L = np.linalg.inv(w2l_rows(meshdata))[np.asarray(mesh, np.int64)]
    n = _unit(np.cross(_apply(L[:, :3, :3], T["posedge1"].astype(np.float64)),
                       _apply(L[:, :3, :3], T["posedge2"].astype(np.float64))))
    n = np.where(((n * towards).sum(1) < 0)[:, None], -n, n)
    return n, _apply(L[:, :3, :3], T["pos0"].astype(np.float64)) + L[:, :3, 3]


def analytic_ellipsoid_normal(p, centre, R, scale):
    """normalize(R S^-2 R^T (p - c)): the smooth normal of the unit sphere under L2W = T R S at world point p."""
    x = (np.asarray(p, np.float64) - np.asarray(centre, np.float64)) @ R        # R^T (p - c), row vectors
    return _unit((x / np.asarray(scale, np.float64) ** 2) @ R.T)


def analytic_ellipsoid_bound(tris, tri, p, o, t, centre, R, scale):
    s = np.abs(np.asarray(scale, np.float64))
    T = tris[np.asarray(tri, np.int64)]
    e_bary = (np.linalg.norm(T["posedge1"].astype(np.float64), axis=1)
              + np.linalg.norm(T["posedge2"].astype(np.float64), axis=1)) / 65535.0
    e_pos = 8 * ulp32(np.abs(o).max(1) + np.abs(t))
    x = ((np.asarray(p, np.float64) - np.asarray(centre, np.float64)) @ R) / np.asarray(scale, np.float64)
    return (s.max() / s.min()) * (E_OCT + e_bary + e_pos / s.min()) / np.linalg.norm(x, axis=1)


# ------------------------------------------------------------------ the cosine lobe
@dataclass
class Lobe:
    om: np.ndarray        # (n, 3) omega_o
    r2: np.ndarray        # max(a^2, b^2)
    tol_y: np.ndarray     # bound of om.y
    pdf_marginal: np.ndarray
    branch_marginal: np.ndarray  # |a| and |b| within roundings of each other: the azimuth may take either branch


def lobe(pixel, frames, max_bounce, cur_bounce, frame_pixels=0) -> Lobe:
    rx, ry = random2(1, pixel, frames, max_bounce, cur_bounce, frame_pixels)
    a, b = 2.0 * rx.astype(np.float64) - 1.0, 2.0 * ry.astype(np.float64) - 1.0
    a, b = np.where(a == 0, 1e-5, a), np.where(b == 0, 1e-5, b)
    first = a * a > b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        rr = np.where(first, a, b)
        phi = np.where(first, 0.25 * np.pi * (b / a), 0.25 * np.pi * (a / b) + 0.5 * np.pi)
    r2 = rr * rr
    y = np.sqrt(np.abs(1.0 - r2))
    om = np.stack([rr * np.cos(phi), y, rr * np.sin(phi)], 1)
    with np.errstate(divide="ignore"):
        tol_y = 12 * U24 * r2 / y + 2 * U24
    return Lobe(om, r2, tol_y, np.abs(1.0 - r2) <= 24 * U24, np.abs(np.abs(a) - np.abs(b)) <= 8 * U24)


def tangent_frame(n):
    """GetTangentSpace(n) in float64: (tangent, binormal)."""
    helper = np.where((np.abs(n[:, 0]) > 0.99)[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    t = _unit(np.cross(n, helper))
    return t, np.cross(n, t)


# ------------------------------------------------------------------ the bounce
@dataclass
class Bounce:
    """The model of one enqueue over n source rays. Per source ray: `firm` survives whatever the rounding, `open_pdf`
    may or may not. Per candidate (firm or open_pdf) row k of `idx`: everything below."""
    firm: np.ndarray
    open_pdf: np.ndarray
    idx: np.ndarray         # source indices of the candidates, ascending
    pos: np.ndarray
    normals: Normals        # before the flip
    flipped: np.ndarray
    marginal: np.ndarray    # a class-dependent check is left open (flip, conditioning)
    marginal_flip: np.ndarray
    norm: np.ndarray        # (k, 4, 3) candidate norms (flipped smooth normal after the round trip)
    norm_valid: np.ndarray  # (k, 4)
    norm_code: np.ndarray   # (k,) the float64 code
    norm_slack: np.ndarray  # (k,) added to a bound on norm (the fold)
    n_side: np.ndarray      # geometric normal on the side the ray came from
    corner: np.ndarray
    lobe: Lobe
    tol_origin: np.ndarray
    mesh: np.ndarray
    helper_z: np.ndarray    # |norm.x| > 0.99 (GetTangentSpace's other helper)


def bounce(tris, meshdata, src, far, cur_bounce, frames, max_bounce, frame_pixels=0, geometry=True) -> Bounce:
    """src: the n source rays (RayData) as traced. geometry=False: the survivor rule alone (order-only cases)."""
    t32 = src["hits"][:, 2].copy().view(np.float32)
    hit = (t32 < np.float32(far)) & (src["hits"][:, 1] < 0x80000000)  # t < far, (int) triangle_id >= 0
    lb_all = lobe(src["PixelIndex"], frames, max_bounce, cur_bounce, frame_pixels)
    alive = hit & (lb_all.om[:, 1] > 0)
    open_pdf = hit & lb_all.pdf_marginal
    firm = alive & ~open_pdf
    idx = np.nonzero(firm | open_pdf)[0]
    if not geometry:
        return Bounce(firm, open_pdf, idx, *([None] * 15))
    s = src[idx]
    lb = Lobe(lb_all.om[idx], lb_all.r2[idx], lb_all.tol_y[idx], lb_all.pdf_marginal[idx], lb_all.branch_marginal[idx])
    o, d = s["origin"].astype(np.float64), s["direction"].astype(np.float64)
    t = t32[idx].astype(np.float64)
    pos = o + d * t[:, None]
    mesh, tri = s["hits"][:, 0].astype(np.int64), s["hits"][:, 1].astype(np.int64)
    assert (mesh < len(meshdata)).all() and (tri < len(tris)).all(), "a record names no triangle of the scene"
    nm = restated_normals(tris, meshdata, mesh, tri, s["hits"][:, 3])
    dus = (d * nm.us).sum(1)
    flipped = dus > 0
    marginal_flip = np.abs(dus) <= (nm.tol_us + 4 * U24) * np.linalg.norm(d, axis=1)
    g = np.where(flipped[:, None], -nm.g, nm.g)
    codes, valid, slack = oct_round_trip(g, nm.tol_g)
    norm = oct_decode(codes)
    n_side, corner = geometric_normal(tris, meshdata, mesh, tri, -d)
    new_o = pos + OFFSET * n_side
    e = 0.5 * (ulp32(d * t[:, None]) + ulp32(pos) + ulp32(new_o))
    tol_origin = np.sqrt((e * e).sum(1)) + OFFSET * (nm.tol_us + 8 * U24)
    return Bounce(firm, open_pdf, idx, pos, nm, flipped, nm.marginal | marginal_flip, marginal_flip, norm, valid,
                  codes[:, 0], slack, n_side, corner, lb, tol_origin, mesh, np.abs(norm[:, 0, 0]) > 0.99)


# ------------------------------------------------------------------ statistics
def ks_statistic(x):
    """The one-sample Kolmogorov-Smirnov statistic of x against U(0, 1)."""
    x = np.sort(np.asarray(x, np.float64))
    n = len(x)
    i = np.arange(1, n + 1)
    return float(max((i / n - x).max(), (x - (i - 1) / n).max()))


def ks_limit(n, alpha=0.001):
    """The asymptotic limit sqrt(-ln(alpha / 2) / 2) / sqrt(n): 1.95 / sqrt(n) at alpha = 0.001."""
    return float(np.sqrt(-np.log(alpha / 2) / 2) / np.sqrt(n))
