// tt_light_refit_core.h — the arithmetic of the light-BVH refit, LightBVHRefitter.compute restated: RefitKernel
// (:136-157, the light TLAS under each light mesh's current matrix) and LightRefitKernel (:183-209, the light tree
// of a deforming mesh), with the TransferKernel copy in front of it (BVHRefitter.compute:135-147). One text, two
// compilers, as tt_lights_core.h: the kernels (tt_light_refit.hip, hipcc for gfx950) and the scalar host reference
// (host/tt_lights.cpp, g++) both build this header under the Makefile's numerics contract, so "bit for bit"
// between them is a statement about the two compilers' arithmetic. The independent check of what is computed is
// the float64 model of tests/lights_refit.py.
//
// Pins: those of tt_lights_core.h -- dot(a, b) = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)),
// cross as its fmaf form, normalize(v) = v * (1 / sqrt(dot)), length = sqrt(dot), distance(a, b) = length(a - b),
// mul(M, v) rows as fmaf chains (the zero fourth terms of Rotate's float4 products are dropped) -- and: max / min =
// IEEE maxNum / minNum written as compares (a NaN loses; of two equal operands the second is returned, so signed
// zeros come out the same from both compilers); float -> uint = D3D's (NaN -> 0, saturating); round =
// round-half-to-even; floor exact; transform_position / transform_direction and the entries of Rotate are written
// out in the text and so evaluated as written, left to right, unfused. asin / acos / sin / cos are driver-defined
// in HLSL and differ between glibc and the device math library: they are the fixed double-precision sequences
// below (+ - * / sqrt and floor only, no libm call on either side), rounded to float once.
//
// TT_LIGHT_REFIT_CONSERVATIVE is a compile-time branch (kCons) of the same functions: Rotate applies m itself
// (the reference returns m * transpose(m), the identity up to rounding: the union cone keeps A's axis), and a
// TLAS leaf's axis is the matrix times the root's axis, normalized (the reference multiplies by the matrix of
// absolute values and does not normalize).
#ifndef TT_LIGHT_REFIT_CORE_H
#define TT_LIGHT_REFIT_CORE_H
#include "tt_lights_core.h"

#if defined(__HIPCC__)
#define TT_LR_UNROLL _Pragma("unroll")
#else
#define TT_LR_UNROLL
#endif

namespace tt_lr {

using tt_lt::V3;
using tt_lt::absf;
using tt_lt::cross;
using tt_lt::dot;
using tt_lt::fma_;
using tt_lt::from_bits;
using tt_lt::length;
using tt_lt::normalize;
using tt_lt::sub;

TT_LT_FN float qnan() { return from_bits(0x7fc00000u); }
TT_LT_FN float maxnum(float a, float b) {
    if (a != a) return b;
    if (b != b) return a;
    return a > b ? a : b;
}
TT_LT_FN float minnum(float a, float b) {
    if (a != a) return b;
    if (b != b) return a;
    return a < b ? a : b;
}
TT_LT_FN uint32_t ftou_d3d(float f) {
    if (!(f > 0.0f)) return 0u;
    if (f >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)f;
}
TT_LT_FN V3 add(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }

// ------------------------------------------------------------------ the pinned asin / acos / sin / cos
// pi / 2 in two doubles; pi / 2 with 33 significant bits and its tail (the first step of the classic
// two-constant argument reduction: k * kPio2A is exact for the small k a float angle in [0, pi) gives)
#define TT_LR_PIO2_HI 1.5707963267948966
#define TT_LR_PIO2_LO 6.123233995736766e-17
#define TT_LR_PIO2_A 1.57079632673412561417
#define TT_LR_PIO2_AT 6.07710050650619224932e-11

// asin on [0, 1 / 2]: the Maclaurin series sum_n (2n)! / (4^n n!^2 (2n + 1)) a^(2n + 1), 30 terms after the first
// (z = a^2 <= 1 / 4, so the first term left out is below 2^-60 of the sum). z is passed in: the caller of the
// half-angle form has it before the square root. The divisions are of constants: both compilers fold them to the
// same correctly rounded doubles (or divide at run time, to the same bits).
TT_LT_FN double asin_series(double a, double z) {
    double t = a, sum = a;
    TT_LR_UNROLL
    for (int n = 1; n <= 30; n++) {
        t = t * z * ((double)(2 * n - 1) / (double)(2 * n));
        sum = sum + t * (1.0 / (double)(2 * n + 1));
    }
    return sum;
}
TT_LT_FN float asin_pinned(float xf) {
    const double x = (double)xf;
    if (!(x >= -1.0 && x <= 1.0)) return qnan();
    const double a = x < 0.0 ? -x : x;
    double r;
    if (a <= 0.5) {
        r = asin_series(a, a * a);
    } else {  // asin(a) = pi / 2 - 2 asin(sqrt((1 - a) / 2))
        const double z = (1.0 - a) / 2.0;
        r = TT_LR_PIO2_HI - (2.0 * asin_series(__builtin_sqrt(z), z) - TT_LR_PIO2_LO);
    }
    return (float)(x < 0.0 ? -r : r);
}
TT_LT_FN float acos_pinned(float xf) {
    const double x = (double)xf;
    if (!(x >= -1.0 && x <= 1.0)) return qnan();
    double r;
    if (x >= -0.5 && x <= 0.5) {
        r = TT_LR_PIO2_HI - (asin_series(x, x * x) - TT_LR_PIO2_LO);
    } else if (x > 0.0) {  // acos(x) = 2 asin(sqrt((1 - x) / 2))
        const double z = (1.0 - x) / 2.0;
        r = 2.0 * asin_series(__builtin_sqrt(z), z);
    } else {  // acos(x) = pi - 2 asin(sqrt((1 + x) / 2))
        const double z = (1.0 + x) / 2.0;
        r = 2.0 * TT_LR_PIO2_HI - (2.0 * asin_series(__builtin_sqrt(z), z) - 2.0 * TT_LR_PIO2_LO);
    }
    return (float)r;
}
// sin and cos of |x| <= 2^20 (the text's angles lie in [0, pi); beyond 2^20, where k * TT_LR_PIO2_A stops being
// exact, the answer is NaN like every other argument outside a domain): r = x - k pi / 2 with k = floor(x 2 / pi +
// 1 / 2), |r| <= pi / 4, the Maclaurin polynomials to r^23 and r^22 in Horner form, the quadrant from k mod 4.
TT_LT_FN void sincos_double(double x, double& s, double& c) {
    const double k = __builtin_floor(x * 0.63661977236758134 + 0.5);
    const double r = (x - k * TT_LR_PIO2_A) - k * TT_LR_PIO2_AT;
    const double r2 = r * r;
    double ps = 1.0, pc = 1.0;
    TT_LR_UNROLL
    for (int n = 11; n >= 1; n--) {
        ps = 1.0 - ps * r2 * (1.0 / (double)((2 * n) * (2 * n + 1)));
        pc = 1.0 - pc * r2 * (1.0 / (double)((2 * n - 1) * (2 * n)));
    }
    ps = r * ps;
    const double q = k - 4.0 * __builtin_floor(k / 4.0);
    if (q == 0.0) {
        s = ps;
        c = pc;
    } else if (q == 1.0) {
        s = pc;
        c = -ps;
    } else if (q == 2.0) {
        s = -ps;
        c = -pc;
    } else {
        s = -pc;
        c = ps;
    }
}
TT_LT_FN float sin_pinned(float xf) {
    const double x = (double)xf;
    if (!(x >= -1048576.0 && x <= 1048576.0)) return qnan();
    double s, c;
    sincos_double(x, s, c);
    return (float)s;
}
TT_LT_FN float cos_pinned(float xf) {
    const double x = (double)xf;
    if (!(x >= -1048576.0 && x <= 1048576.0)) return qnan();
    double s, c;
    sincos_double(x, s, c);
    return (float)c;
}

// ------------------------------------------------------------------ LightBVHRefitter.compute, helpers
// octahedral_32 — :6-12 (tt_lights_core.h's text with D3D's float -> uint conversion). A zero vector (the
// full-sphere cone) divides by zero: the NaNs convert to 0 as in D3D, not guarded, as the text.
TT_LT_FN uint32_t octahedral_32_d3d(V3 nor) {
    const float sx = nor.x >= 0.0f ? 1.0f : -1.0f, sy = nor.y >= 0.0f ? 1.0f : -1.0f;
    const float den = nor.x * sx + nor.y * sy + absf(nor.z);
    float x = nor.x / den, y = nor.y / den;
    if (!(nor.z >= 0.0f)) {
        const float ox = x;
        x = (1.0f - (y * sy)) * sx;
        y = (1.0f - (ox * sx)) * sy;
    }
    const uint32_t dx = ftou_d3d(__builtin_rintf(32767.5f + x * 32767.5f)), dy = ftou_d3d(__builtin_rintf(32767.5f + y * 32767.5f));
    return dx | (dy << 16u);
}
// i_octahedral_32 — :14-22: the text of CommonData.cginc's, which tt_lights_core.h restates
using tt_lt::i_octahedral_32;

// GetCosThetaO / GetCosThetaE / CompCosTheta — :74-82 (full uints shifted and OR-ed, as the text)
TT_LT_FN float get_cos_theta_o(uint32_t c) { return 2.0f * ((float)(c & 0x0000ffffu) / 32767.0f) - 1.0f; }
TT_LT_FN float get_cos_theta_e(uint32_t c) { return 2.0f * ((float)(c >> 16) / 32767.0f) - 1.0f; }
TT_LT_FN uint32_t comp_cos_theta(float cos_o, float cos_e) {
    return ftou_d3d(__builtin_floorf(32767.0f * ((cos_o + 1.0f) / 2.0f))) |
           (ftou_d3d(__builtin_floorf(32767.0f * ((cos_e + 1.0f) / 2.0f))) << 16);
}

// AngleBetween — :39-42. length / 2 is at most about sqrt(2) / 2 for unit vectors (the branch picks the shorter
// of v1 + v2 and v2 - v1); beyond 1 the pinned asin answers NaN and it flows as written.
TT_LT_FN float angle_between(V3 v1, V3 v2) {
    if (dot(v1, v2) < 0.0f) return 3.14159f - 2.0f * asin_pinned(length(add(v1, v2)) / 2.0f);
    return 2.0f * asin_pinned(length(sub(v2, v1)) / 2.0f);
}

// mul(Rotate(theta, axis), float4(v, 0)).xyz — :45-73, :100. Rotate returns mul(m, transpose(m)) (:68): element
// (i, j) is the dot of rows i and j of m, whose fourth entries are zero. kCons applies m itself.
template <bool kCons>
TT_LT_FN V3 rotate_apply(float theta, V3 axis, V3 v) {
    const float sinTheta = sin_pinned(theta), cosTheta = cos_pinned(theta);
    const V3 a = normalize(axis);
    const V3 r0 = {a.x * a.x + (1.0f - a.x * a.x) * cosTheta, a.x * a.y * (1.0f - cosTheta) - a.z * sinTheta,
                   a.x * a.z * (1.0f - cosTheta) + a.y * sinTheta};
    const V3 r1 = {a.x * a.y * (1.0f - cosTheta) + a.z * sinTheta, a.y * a.y + (1.0f - a.y * a.y) * cosTheta,
                   a.y * a.z * (1.0f - cosTheta) - a.x * sinTheta};
    const V3 r2 = {a.x * a.z * (1.0f - cosTheta) - a.y * sinTheta, a.y * a.z * (1.0f - cosTheta) + a.x * sinTheta,
                   a.z * a.z + (1.0f - a.z * a.z) * cosTheta};
    if (kCons) return V3{dot(r0, v), dot(r1, v), dot(r2, v)};
    const V3 t0 = {dot(r0, r0), dot(r0, r1), dot(r0, r2)};
    const V3 t1 = {dot(r1, r0), dot(r1, r1), dot(r1, r2)};
    const V3 t2 = {dot(r2, r0), dot(r2, r1), dot(r2, r2)};
    return V3{dot(t0, v), dot(t1, v), dot(t2, v)};
}

struct Cone {
    V3 w;
    float c;
};
// DoCone — :84-102
template <bool kCons>
TT_LT_FN Cone do_cone(Cone A, Cone B) {
    if (A.w.x == 0.0f && A.w.y == 0.0f && A.w.z == 0.0f) return B;
    if (B.w.x == 0.0f && B.w.y == 0.0f && B.w.z == 0.0f) return A;
    const float theta_a = acos_pinned(A.c);
    const float theta_b = acos_pinned(B.c);
    const float theta_d = angle_between(A.w, B.w);
    if (minnum(theta_d + theta_b, 3.14159f) <= theta_a) return A;
    if (minnum(theta_d + theta_a, 3.14159f) <= theta_b) return B;
    const float theta_o = (theta_a + theta_d + theta_b) / 2.0f;
    if (theta_o >= 3.14159f) return Cone{V3{0.0f, 0.0f, 0.0f}, -1.0f};
    const float theta_r = theta_o - theta_a;
    const V3 wr = cross(A.w, B.w);
    if (dot(wr, wr) == 0.0f) return Cone{V3{0.0f, 0.0f, 0.0f}, -1.0f};
    return Cone{rotate_apply<kCons>(theta_r, wr, A.w), cos_pinned(theta_o)};
}

// Union — :105-111
template <bool kCons>
TT_LT_FN tt_light_node union_node(const tt_light_node& A, const tt_light_node& B, int32_t left) {
    const Cone cone = do_cone<kCons>(Cone{i_octahedral_32(A.w), get_cos_theta_o(A.cosTheta_oe)},
                                     Cone{i_octahedral_32(B.w), get_cos_theta_o(B.cosTheta_oe)});
    const float cos_e = minnum(get_cos_theta_e(A.cosTheta_oe), get_cos_theta_e(B.cosTheta_oe));
    tt_light_node d;
    for (int k = 0; k < 3; k++) {
        d.BBMax[k] = maxnum(A.BBMax[k], B.BBMax[k]);
        d.BBMin[k] = minnum(A.BBMin[k], B.BBMin[k]);
    }
    d.w = octahedral_32_d3d(cone.w);
    d.phi = A.phi + B.phi;
    d.cosTheta_oe = comp_cos_theta(cone.c, cos_e);
    d.left = left;
    return d;
}

// HLSL mat[r][c] of a column-major Transform: element (r, c) at m[c * 4 + r]
TT_LT_FN float E_(const float* m, int r, int c) { return m[c * 4 + r]; }
// transform_position — :120-126
TT_LT_FN V3 transform_position(const float* m, V3 p) {
    return V3{E_(m, 0, 0) * p.x + E_(m, 0, 1) * p.y + E_(m, 0, 2) * p.z + E_(m, 0, 3),
              E_(m, 1, 0) * p.x + E_(m, 1, 1) * p.y + E_(m, 1, 2) * p.z + E_(m, 1, 3),
              E_(m, 2, 0) * p.x + E_(m, 2, 1) * p.y + E_(m, 2, 2) * p.z + E_(m, 2, 3)};
}
// transform_direction — :127-134: the matrix of absolute values (right for a box's half extent)
TT_LT_FN V3 transform_direction(const float* m, V3 d) {
    return V3{absf(E_(m, 0, 0)) * d.x + absf(E_(m, 0, 1)) * d.y + absf(E_(m, 0, 2)) * d.z,
              absf(E_(m, 1, 0)) * d.x + absf(E_(m, 1, 1)) * d.y + absf(E_(m, 1, 2)) * d.z,
              absf(E_(m, 2, 0)) * d.x + absf(E_(m, 2, 1)) * d.y + absf(E_(m, 2, 2)) * d.z};
}
// the same sums without the absolute values (kCons: a direction under the matrix)
TT_LT_FN V3 transform_vector(const float* m, V3 d) {
    return V3{E_(m, 0, 0) * d.x + E_(m, 0, 1) * d.y + E_(m, 0, 2) * d.z, E_(m, 1, 0) * d.x + E_(m, 1, 1) * d.y + E_(m, 1, 2) * d.z,
              E_(m, 2, 0) * d.x + E_(m, 2, 1) * d.y + E_(m, 2, 2) * d.z};
}

// RefitKernel's leaf branch — :143-151. `root` is LightNodes[SolidOffset]; nd.left stays.
template <bool kCons>
TT_LT_FN void tlas_leaf(const float* m, const tt_light_node& root, tt_light_node& nd) {
    const V3 bmax = tt_lt::ld3(root.BBMax), bmin = tt_lt::ld3(root.BBMin);
    const V3 center = transform_position(m, V3{(bmax.x + bmin.x) / 2.0f, (bmax.y + bmin.y) / 2.0f, (bmax.z + bmin.z) / 2.0f});
    const V3 extent = transform_direction(m, V3{(bmax.x - bmin.x) / 2.0f, (bmax.y - bmin.y) / 2.0f, (bmax.z - bmin.z) / 2.0f});
    nd.BBMax[0] = center.x + extent.x;
    nd.BBMax[1] = center.y + extent.y;
    nd.BBMax[2] = center.z + extent.z;
    nd.BBMin[0] = center.x - extent.x;
    nd.BBMin[1] = center.y - extent.y;
    nd.BBMin[2] = center.z - extent.z;
    const V3 axis = i_octahedral_32(root.w);
    nd.w = kCons ? octahedral_32_d3d(normalize(transform_vector(m, axis))) : octahedral_32_d3d(transform_direction(m, axis));
    nd.phi = maxnum(root.phi, 0.000000f);
    nd.cosTheta_oe = root.cosTheta_oe;
}

// AreaOfTriangle — :174-180
TT_LT_FN float area_of_triangle(V3 pt1, V3 pt2, V3 pt3) {
    const float a = length(sub(pt1, pt2)), b = length(sub(pt2, pt3)), c = length(sub(pt3, pt1));
    const float s = (a + b + c) / 2.0f;
    return TT_LT_SQRT(s * (s - a) * (s - b) * (s - c));
}

// LightRefitKernel's leaf branch — :190-203. nd.cosTheta_oe and nd.left stay.
TT_LT_FN void mesh_leaf(const tt_light_tri& T, tt_light_node& nd) {
    const V3 p0 = tt_lt::ld3(T.pos0), e1 = tt_lt::ld3(T.posedge1), e2 = tt_lt::ld3(T.posedge2);
    const V3 p1 = add(p0, e1), p2 = add(p0, e2);
    float mx[3] = {maxnum(maxnum(p0.x, p1.x), p2.x), maxnum(maxnum(p0.y, p1.y), p2.y), maxnum(maxnum(p0.z, p1.z), p2.z)};
    float mn[3] = {minnum(minnum(p0.x, p1.x), p2.x), minnum(minnum(p0.y, p1.y), p2.y), minnum(minnum(p0.z, p1.z), p2.z)};
    for (int i = 0; i < 3; i++)
        if (absf(mx[i] - mn[i]) < 0.0001f) {
            mx[i] += 0.0001f;
            mn[i] -= 0.0001f;
        }
    for (int i = 0; i < 3; i++) {
        nd.BBMax[i] = mx[i];
        nd.BBMin[i] = mn[i];
    }
    const V3 n = normalize(cross(normalize(e1), normalize(e2)));
    nd.w = octahedral_32_d3d(V3{-n.x, -n.y, -n.z});
    nd.phi = maxnum(area_of_triangle(p0, p1, p2), 0.00000001f);
}

// TransferKernel (BVHRefitter.compute:135-147): the deformed positions out of the aggregated triangle
TT_LT_FN void transfer_tri(const tt_cuda_triangle& S, tt_light_tri& T) {
    for (int k = 0; k < 3; k++) {
        T.pos0[k] = S.pos0[k];
        T.posedge1[k] = S.posedge1[k];
        T.posedge2[k] = S.posedge2[k];
    }
}

}  // namespace tt_lr
#endif
