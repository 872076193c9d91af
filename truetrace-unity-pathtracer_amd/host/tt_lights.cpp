// tt_lights.cpp — the host side of the light BVH (include/truetrace_scene.h, "lights"):
//  * LightBVHBuilder.cs restated: LightBounds Union / UnionCone, EvaluateCost, partition_sah over three presorted
//    index lists, the recursive build (children allocated in pre-order, so every `left` is even and greater than
//    its node's index), the 40-byte packing; both constructors;
//  * the layout of LightNodes / LightTriangles / _LightMeshes (AssetManager.cs:998-1040, :1100-1204, :1681-1707);
//  * tt_emit_nee_host, the scalar reference of tt_emit_nee: csrc/tt_lights_core.h built by the host compiler;
//  * tt_lights_refit_host, the scalar reference of tt_lights_refit (LightBVHRefitter.compute, level by level as the
//    reference dispatches it): csrc/tt_light_refit_core.h built by the host compiler; tt_light_refit_math.
// Where this differs from the reference on purpose (each stated at its place): a stable presort; the merged cone's
// axis is really rotated (the reference multiplies the rotation by its transpose, which is the identity, and so
// leaves the axis where it was: the merged cone then need not contain the second cone); asin's argument is
// clamped to 1; a split with no finite cost falls back to the middle; unused node slots are zero bytes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/truetrace_scene.h"
#include "../csrc/tt_light_refit_core.h"
#include "../csrc/tt_light_refit_plan_host.h"
#include "../csrc/tt_lights_check_host.h"
#include "../csrc/tt_lights_core.h"

namespace {

const float kPi = 3.14159f;  // the builder's own constant

struct Vec {
    float x, y, z;
};
inline Vec operator+(Vec a, Vec b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline Vec operator-(Vec a, Vec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline float dotv(Vec a, Vec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline float lengthv(Vec a) { return (float)std::sqrt((double)dotv(a, a)); }
inline Vec normalized(Vec a) {  // Vector3.normalized: zero below 1e-5
    const float m = lengthv(a);
    if (m > 1e-5f) return {a.x / m, a.y / m, a.z / m};
    return {0.0f, 0.0f, 0.0f};
}
inline Vec crossv(Vec a, Vec b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline float facos(float c) { return (float)std::acos((double)c); }
inline float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

using LB = tt_light_bounds;

inline Vec w_of(const LB& b) { return {b.w[0], b.w[1], b.w[2]}; }
inline void set_w(LB& b, Vec w) {
    b.w[0] = w.x;
    b.w[1] = w.y;
    b.w[2] = w.z;
}
inline bool cone_empty(const LB& b) { return b.w[0] == 0.0f && b.w[1] == 0.0f && b.w[2] == 0.0f; }

float angle_between(Vec v1, Vec v2) {
    if (dotv(v1, v2) < 0) return kPi - 2.0f * (float)std::asin((double)std::min(lengthv(v1 + v2) / 2.0f, 1.0f));
    return 2.0f * (float)std::asin((double)std::min(lengthv(v2 - v1) / 2.0f, 1.0f));
}

// Rotate(theta, axis) applied to v (LightBVHBuilder.cs:51-75, the matrix itself: see the file comment)
Vec rotate(float theta, Vec axis, Vec v) {
    const float s = (float)std::sin((double)theta), c = (float)std::cos((double)theta);
    const Vec a = normalized(axis);
    const float m00 = a.x * a.x + (1 - a.x * a.x) * c, m01 = a.x * a.y * (1 - c) - a.z * s, m02 = a.x * a.z * (1 - c) + a.y * s;
    const float m10 = a.x * a.y * (1 - c) + a.z * s, m11 = a.y * a.y + (1 - a.y * a.y) * c, m12 = a.y * a.z * (1 - c) - a.x * s;
    const float m20 = a.x * a.z * (1 - c) - a.y * s, m21 = a.y * a.z * (1 - c) + a.x * s, m22 = a.z * a.z + (1 - a.z * a.z) * c;
    return {m00 * v.x + m01 * v.y + m02 * v.z, m10 * v.x + m11 * v.y + m12 * v.z, m20 * v.x + m21 * v.y + m22 * v.z};
}

void union_cone(LB& A, const LB& B) {
    if (cone_empty(A)) {
        set_w(A, w_of(B));
        A.cosTheta_o = B.cosTheta_o;
        return;
    }
    if (cone_empty(B)) return;
    const float theta_a = facos(clampf(A.cosTheta_o, -1.0f, 1.0f));
    const float theta_b = facos(clampf(B.cosTheta_o, -1.0f, 1.0f));
    const float theta_d = angle_between(w_of(A), w_of(B));
    if (std::min(theta_d + theta_b, kPi) <= theta_a) return;
    if (std::min(theta_d + theta_a, kPi) <= theta_b) {
        set_w(A, w_of(B));
        A.cosTheta_o = B.cosTheta_o;
        return;
    }
    const float theta_o = (theta_a + theta_d + theta_b) / 2.0f;
    if (theta_o >= kPi) {  // the full-sphere fallback
        set_w(A, {0, 0, 0});
        A.cosTheta_o = -1;
        return;
    }
    const float theta_r = theta_o - theta_a;
    const Vec wr = crossv(w_of(A), w_of(B));
    if (dotv(wr, wr) == 0) {
        set_w(A, {0, 0, 0});
        A.cosTheta_o = -1;
        return;
    }
    set_w(A, rotate(theta_r, wr, w_of(A)));
    A.cosTheta_o = (float)std::cos((double)theta_o);
}

void union_bounds(LB& A, const LB& B) {
    if (A.phi == 0) {
        A = B;
        return;
    }
    if (B.phi == 0) return;
    union_cone(A, B);
    A.cosTheta_e = std::min(A.cosTheta_e, B.cosTheta_e);
    for (int k = 0; k < 3; k++) {
        if (B.BBMin[k] < A.BBMin[k]) A.BBMin[k] = B.BBMin[k];
        if (B.BBMax[k] > A.BBMax[k]) A.BBMax[k] = B.BBMax[k];
    }
    A.phi += B.phi;
    A.LightCount += B.LightCount;
}

float evaluate_cost(const LB& b, float Kr) {
    const float theta_o = facos(b.cosTheta_o), theta_e = facos(b.cosTheta_e);
    const float theta_w = std::min(theta_o + theta_e, kPi);
    const float sin_o = std::sqrt(1.0f - b.cosTheta_o * b.cosTheta_o);
    const float M_omega = 2.0f * kPi * (1.0f - b.cosTheta_o) +
                          kPi / 2.0f * (2.0f * theta_w * sin_o - (float)std::cos((double)(theta_o - 2.0f * theta_w)) -
                                        2.0f * theta_o * sin_o + b.cosTheta_o);
    const float sx = b.BBMax[0] - b.BBMin[0], sy = b.BBMax[1] - b.BBMin[1], sz = b.BBMax[2] - b.BBMin[2];
    const float area = 2.0f * ((sx * sy) + (sx * sz) + (sy * sz));
    return b.phi * M_omega * Kr * area / (float)std::max(b.LightCount, 1);
}

struct Builder {
    uint32_t n;
    std::vector<LB> prims;
    std::vector<LB> bounds;     // per node
    std::vector<int32_t> left;  // per node
    std::vector<uint8_t> leaf;  // per node
    std::vector<int32_t> dim;   // DimensionedIndices: three presorted lists
    std::vector<float> sah;
    std::vector<uint8_t> going_left;
    std::vector<int32_t> temp;

    struct Split {
        int32_t index = -1, dimension = -1;
        float cost = 0;
        LB left{}, right{};
    };

    Split partition_sah(uint32_t first, uint32_t count, const LB& parent) {
        Split sp;
        sp.cost = 3.402823466e+38f;
        const float dx = parent.BBMax[0] - parent.BBMin[0], dy = parent.BBMax[1] - parent.BBMin[1], dz = parent.BBMax[2] - parent.BBMin[2];
        const float diag[3] = {dx, dy, dz};
        const float Kr1 = std::max(std::max(dx, dy), dz);
        for (int d = 0; d < 3; d++) {
            const float Kr = Kr1 / diag[d];
            const size_t off = (size_t)n * d + first;
            LB l = prims[dim[off]];
            sah[1] = evaluate_cost(l, Kr);
            for (uint32_t i = 2; i < count; i++) {
                union_bounds(l, prims[dim[off + i - 1]]);
                sah[i] = evaluate_cost(l, Kr) * (float)i;
            }
            LB r = prims[dim[off + count - 1]];
            {
                const float cost = sah[count - 1] + evaluate_cost(r, Kr) * 1.0f;
                if (cost <= sp.cost) {
                    sp.cost = cost;
                    sp.index = (int32_t)(first + count - 1);
                    sp.dimension = d;
                    sp.right = r;
                }
            }
            for (uint32_t i = count - 2; i > 0; i--) {
                union_bounds(r, prims[dim[off + i]]);
                const float cost = sah[i] + evaluate_cost(r, Kr) * (float)(count - i);
                if (cost <= sp.cost) {
                    sp.cost = cost;
                    sp.index = (int32_t)(first + i);
                    sp.dimension = d;
                    sp.right = r;
                }
            }
        }
        if (sp.index < 0) {  // no finite cost on any axis (the reference would index with -1): the middle of axis 0
            sp.dimension = 0;
            sp.index = (int32_t)(first + count / 2);
            sp.right = prims[dim[sp.index]];
            for (uint32_t i = (uint32_t)sp.index + 1; i < first + count; i++) union_bounds(sp.right, prims[dim[i]]);
        }
        const size_t off = (size_t)sp.dimension * n;
        sp.left = prims[dim[off + first]];
        for (uint32_t i = first + 1; i < (uint32_t)sp.index; i++) union_bounds(sp.left, prims[dim[off + i]]);
        return sp;
    }

    // both constructors from here on: prims are set, bounds[0] is their union
    void build(tt_light_node* out) {
        bounds.assign(2 * (size_t)n, LB{});
        left.assign(2 * (size_t)n, 0);
        leaf.assign(2 * (size_t)n, 0);
        dim.resize(3 * (size_t)n);
        sah.assign(std::max<size_t>(n, 2), 0.0f);
        going_left.assign(n, 0);
        temp.resize(n);
        std::vector<uint8_t> used(2 * (size_t)n, 0);
        for (uint32_t i = 0; i < n; i++) union_bounds(bounds[0], prims[i]);
        // the presort by box centre per axis; STABLE (System.Array.Sort is not: ties may fall either way there)
        for (int d = 0; d < 3; d++) {
            std::vector<float> centre(n);
            for (uint32_t i = 0; i < n; i++) centre[i] = (prims[i].BBMax[d] - prims[i].BBMin[d]) / 2.0f + prims[i].BBMin[d];
            int32_t* list = dim.data() + (size_t)n * d;
            for (uint32_t i = 0; i < n; i++) list[i] = (int32_t)i;
            std::stable_sort(list, list + n, [&](int32_t a, int32_t b) { return centre[a] < centre[b]; });
        }
        struct Job {
            uint32_t node, first, count;
        };
        std::vector<Job> stack;
        stack.push_back({0u, 0u, n});
        used[0] = 1;
        uint32_t next_node = 2;
        while (!stack.empty()) {  // BuildRecursive in its own order: a node, its left subtree, its right subtree
            const Job j = stack.back();
            stack.pop_back();
            if (j.count == 1) {
                left[j.node] = (int32_t)j.first;
                leaf[j.node] = 1;
                continue;
            }
            const Split sp = partition_sah(j.first, j.count, bounds[j.node]);
            const uint32_t end = j.first + j.count;
            size_t off = (size_t)sp.dimension * n;
            for (uint32_t i = j.first; i < end; i++) going_left[dim[off + i]] = i < (uint32_t)sp.index;
            for (int d = 0; d < 3; d++) {
                if (d == sp.dimension) continue;
                uint32_t l = 0, r = (uint32_t)sp.index - j.first;
                off = (size_t)d * n;
                for (uint32_t i = j.first; i < end; i++) {
                    const int32_t idx = dim[off + i];
                    temp[going_left[idx] ? (l++) : (r++)] = idx;
                }
                std::copy(temp.begin(), temp.begin() + j.count, dim.begin() + off + j.first);
            }
            left[j.node] = (int32_t)next_node;
            bounds[next_node] = sp.left;
            bounds[next_node + 1] = sp.right;
            used[next_node] = used[next_node + 1] = 1;
            const uint32_t lc = (uint32_t)sp.index - j.first;
            stack.push_back({next_node + 1, (uint32_t)sp.index, j.count - lc});
            stack.push_back({next_node, j.first, lc});
            next_node += 2;
        }
        for (size_t i = 0; i < 2 * (size_t)n; i++) {
            tt_light_node nd;
            std::memset(&nd, 0, sizeof nd);
            if (used[i]) {  // (an unused slot -- node 1 -- stays zero bytes)
                const LB& b = bounds[i];
                for (int k = 0; k < 3; k++) {
                    nd.BBMax[k] = b.BBMax[k];
                    nd.BBMin[k] = b.BBMin[k];
                }
                nd.w = tt_pack_octahedral(b.w[0], b.w[1], b.w[2]);
                nd.phi = b.phi;
                nd.cosTheta_oe = ((uint32_t)std::floor(32767.0f * ((b.cosTheta_o + 1.0f) / 2.0f))) |
                                 ((uint32_t)std::floor(32767.0f * ((b.cosTheta_e + 1.0f) / 2.0f)) << 16);
                nd.left = leaf[i] ? -(dim[left[i]]) - 1 : left[i];
            }
            out[i] = nd;
        }
    }
};

}  // namespace

extern "C" {

tt_status tt_light_tris_from_mesh(const tt_cuda_triangle* tris, uint32_t n, const uint32_t* targets, uint32_t n_targets,
                                  const float* normals, tt_light_tri* out_tris, float* out_normals) {
    if (!tris || !targets || !out_tris || !out_normals || !n_targets) return TT_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n_targets; i++) {
        if (targets[i] >= n) return TT_ERR_INVALID_ARG;
        const tt_cuda_triangle& T = tris[targets[i]];
        tt_light_tri& L = out_tris[i];
        std::memcpy(L.pos0, T.pos0, 12);
        std::memcpy(L.posedge1, T.posedge1, 12);
        std::memcpy(L.posedge2, T.posedge2, 12);
        L.TriTarget = targets[i];
        Vec nn;
        if (normals) {
            nn = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
        } else {
            const tt_lt::V3 a = tt_lt::i_octahedral_32(T.norms[0]), b = tt_lt::i_octahedral_32(T.norms[1]), c = tt_lt::i_octahedral_32(T.norms[2]);
            nn = normalized({(a.x + b.x + c.x) / 3.0f, (a.y + b.y + c.y) / 3.0f, (a.z + b.z + c.z) / 3.0f});
        }
        out_normals[3 * i] = nn.x;
        out_normals[3 * i + 1] = nn.y;
        out_normals[3 * i + 2] = nn.z;
    }
    return TT_OK;
}

tt_status tt_light_bvh_build_mesh(const tt_light_tri* tris, const float* normals, uint32_t n, tt_light_node* nodes,
                                  tt_light_bounds* root) {
    if (!tris || !normals || !nodes || n == 0 || n > 0x3fffffffu) return TT_ERR_INVALID_ARG;
    Builder B;
    B.n = n;
    B.prims.resize(n);
    const float cos_e = (float)std::cos((double)(kPi / 2.0f));
    for (uint32_t i = 0; i < n; i++) {
        LB b{};
        const Vec p0 = {tris[i].pos0[0], tris[i].pos0[1], tris[i].pos0[2]};
        const Vec p1 = p0 + Vec{tris[i].posedge1[0], tris[i].posedge1[1], tris[i].posedge1[2]};
        const Vec p2 = p0 + Vec{tris[i].posedge2[0], tris[i].posedge2[1], tris[i].posedge2[2]};
        const float px[3][3] = {{p0.x, p0.y, p0.z}, {p1.x, p1.y, p1.z}, {p2.x, p2.y, p2.z}};
        for (int k = 0; k < 3; k++) {
            b.BBMax[k] = std::max(px[0][k], std::max(px[1][k], px[2][k]));
            b.BBMin[k] = std::min(px[0][k], std::min(px[1][k], px[2][k]));
            if (b.BBMax[k] - b.BBMin[k] < 0.0001f) {  // AABB.Validate
                b.BBMin[k] -= 0.0001f;
                b.BBMax[k] += 0.0001f;
            }
        }
        b.w[0] = -normals[3 * i];
        b.w[1] = -normals[3 * i + 1];
        b.w[2] = -normals[3 * i + 2];
        b.phi = 0.1f;
        b.cosTheta_o = 1.0f;
        b.cosTheta_e = cos_e;
        b.LightCount = 1;
        B.prims[i] = b;
    }
    B.build(nodes);
    if (root) *root = B.bounds[0];
    return TT_OK;
}

tt_status tt_light_bvh_build_tlas(const tt_light_bounds* bounds, uint32_t n, tt_light_node* nodes) {
    if (!bounds || !nodes || n == 0 || n > 0x3fffffffu) return TT_ERR_INVALID_ARG;
    Builder B;
    B.n = n;
    B.prims.assign(bounds, bounds + n);
    B.build(nodes);
    return TT_OK;
}

tt_status tt_light_bounds_transform(const tt_light_bounds* root, const float* M, tt_light_bounds* out) {
    if (!root || !M || !out) return TT_ERR_INVALID_ARG;
    auto E = [&](int r, int c) { return M[c * 4 + r]; };
    *out = *root;
    const float c[3] = {(root->BBMax[0] + root->BBMin[0]) / 2.0f, (root->BBMax[1] + root->BBMin[1]) / 2.0f, (root->BBMax[2] + root->BBMin[2]) / 2.0f};
    const float e[3] = {(root->BBMax[0] - root->BBMin[0]) / 2.0f, (root->BBMax[1] - root->BBMin[1]) / 2.0f, (root->BBMax[2] - root->BBMin[2]) / 2.0f};
    Vec w;
    float wv[3];
    for (int r = 0; r < 3; r++) {
        const float nc = E(r, 0) * c[0] + E(r, 1) * c[1] + E(r, 2) * c[2] + E(r, 3);
        const float ne = std::fabs(E(r, 0)) * e[0] + std::fabs(E(r, 1)) * e[1] + std::fabs(E(r, 2)) * e[2];
        // one ulp of slack each way: the transformed corners are rounded sums of the same terms in another order
        out->BBMin[r] = std::nextafter(nc - ne, -INFINITY);
        out->BBMax[r] = std::nextafter(nc + ne, INFINITY);
        wv[r] = E(r, 0) * root->w[0] + E(r, 1) * root->w[1] + E(r, 2) * root->w[2];
    }
    w = normalized({wv[0], wv[1], wv[2]});
    set_w(*out, w);
    return TT_OK;
}

tt_status tt_lights_assemble(const tt_light_parent* parents, uint32_t n_parents, const tt_light_instance* instances,
                             uint32_t n_instances, tt_mesh_data* meshdata, uint32_t n_mesh, tt_light_node* nodes_out,
                             uint32_t* n_nodes, tt_light_tri* tris_out, uint32_t* n_tris, tt_light_mesh* meshes_out) {
    if (!parents || !instances || !meshdata || !nodes_out || !n_nodes || !tris_out || !n_tris || !meshes_out || !n_parents ||
        !n_instances || n_instances > 0x3fffffffu)
        return TT_ERR_INVALID_ARG;
    std::vector<uint32_t> node_off(n_parents), tri_off(n_parents);
    std::vector<LB> roots(n_parents);
    uint64_t nn = 2ull * n_instances, nt = 0;
    for (uint32_t k = 0; k < n_parents; k++) {
        if (!parents[k].tris || !parents[k].normals || !parents[k].n_tris) return TT_ERR_INVALID_ARG;
        node_off[k] = (uint32_t)nn;
        tri_off[k] = (uint32_t)nt;
        nn += 2ull * parents[k].n_tris;
        nt += parents[k].n_tris;
        if (nn > 0x7fffffffull) return TT_ERR_INVALID_ARG;
    }
    for (uint32_t k = 0; k < n_parents; k++) {
        const tt_status st = tt_light_bvh_build_mesh(parents[k].tris, parents[k].normals, parents[k].n_tris, nodes_out + node_off[k], &roots[k]);
        if (st != TT_OK) return st;
        std::memcpy(tris_out + tri_off[k], parents[k].tris, sizeof(tt_light_tri) * parents[k].n_tris);
    }
    std::vector<LB> world(n_instances);
    for (uint32_t i = 0; i < n_instances; i++) {
        const tt_light_instance& I = instances[i];
        if (I.parent >= n_parents || I.mesh_index < 0 || (uint32_t)I.mesh_index >= n_mesh) return TT_ERR_INVALID_ARG;
        tt_light_bounds_transform(&roots[I.parent], I.local_to_world, &world[i]);
        tt_mesh_data& MD = meshdata[I.mesh_index];
        MD.LightNodeOffset = (int32_t)node_off[I.parent];
        MD.LightTriCount = (int32_t)parents[I.parent].n_tris;
        tt_light_mesh& LM = meshes_out[i];
        for (int k = 0; k < 3; k++) LM.Center[k] = (world[i].BBMax[k] + world[i].BBMin[k]) / 2.0f;
        LM.StartIndex = (int32_t)tri_off[I.parent];
        LM.IndexEnd = (int32_t)(tri_off[I.parent] + parents[I.parent].n_tris);
        LM.MatOffset = MD.MaterialOffset;
        LM.LockedMeshIndex = I.mesh_index;
    }
    const tt_status st = tt_light_bvh_build_tlas(world.data(), n_instances, nodes_out);
    if (st != TT_OK) return st;
    *n_nodes = (uint32_t)nn;
    *n_tris = (uint32_t)nt;
    return TT_OK;
}

tt_status tt_emit_nee_host(const tt_light_node* nodes, uint32_t n_nodes, const tt_light_tri* ltris, uint32_t n_ltris,
                           const tt_light_mesh* lmeshes, uint32_t n_lmeshes, const tt_cuda_triangle* tris, uint32_t n_tris,
                           const tt_mesh_data* meshdata, uint32_t n_mesh, const tt_trace_params* p,
                           const tt_ray_data* global_rays, int32_t frames, int32_t max_bounce, uint32_t frame_pixels,
                           uint32_t terrains, tt_light_sample* samples, tt_shadow_ray* shadow_rays, uint32_t* n_shadow) {
    if (!tris || !p || !global_rays || !n_shadow || p->bounce < 0) return TT_ERR_INVALID_ARG;
    std::string why;
    if (tt_lcheck::validate(tt_lcheck::Lights{nodes, n_nodes, ltris, n_ltris, lmeshes, n_lmeshes}, meshdata, n_mesh, n_tris, why) != TT_OK)
        return TT_ERR_INVALID_ARG;
    const tt_lt::Scene S{nodes, ltris, lmeshes, tris, meshdata};
    const uint64_t wh = (uint64_t)p->screen_width * p->screen_height;
    const size_t off = (p->bounce % 2 == 1) ? (size_t)wh : 0u;
    const bool neg = (p->flags & TT_NEE_NEGATIVE_T) != 0;
    uint32_t cnt = 0;
    for (uint32_t i = 0; i < p->n_rays; i++) {
        const tt_ray_data& R = global_rays[off + i];
        tt_light_sample smp;
        tt_shadow_ray ray;
        bool ok = false;
        if (tt_lt::is_hit(R.hits, p->far_plane, terrains != 0) && R.hits[0] < n_mesh && R.hits[1] < n_tris) {
            const tt_lt::HitFrame H = tt_lt::hit_frame(R, tris, meshdata);
            const tt_lt::Rng rng = tt_lt::make_rng(R.PixelIndex, frame_pixels, frames, max_bounce, p->bounce);
            ok = tt_lt::emit_one(S, H.pos, H.norm, H.origin, rng, R.PixelIndex, neg, smp, ray);
        } else {
            tt_lt::miss_sample(smp);
        }
        if (samples) samples[i] = smp;
        if (ok) {
            if (shadow_rays) shadow_rays[cnt] = ray;
            cnt++;
        }
    }
    *n_shadow = cnt;
    return TT_OK;
}

}  // extern "C"

// One tree of the refit plan, the reference's way: its WorkingSet dispatches run from the deepest level up, and
// the plan's breadth-first order lists the levels top down, so the reverse order evaluates them as dispatched (a
// level's nodes do not read each other). `leaf` rewrites a leaf node in place.
template <bool kCons, class Leaf>
static void refit_tree_host(tt_light_node* nodes, const tt_lplan::Plan& P, const tt_lplan::Tree& T, Leaf&& leaf) {
    for (uint32_t k = T.bfs_count; k-- > 0;) {
        const int32_t n = P.bfs[T.bfs_first + k];
        tt_light_node& nd = nodes[n];
        if (nd.left < 0) {
            leaf(nd);
            continue;
        }
        const tt_light_node& a = nodes[T.base + nd.left];
        nd = tt_lr::union_node<kCons>(a, nodes[T.base + nd.left + 1], nd.left);
    }
}

template <bool kCons>
static void lights_refit_host(tt_light_node* nodes, uint32_t n_nodes, tt_light_tri* ltris, const tt_cuda_triangle* tris,
                              uint32_t n_tris, const tt_mesh_data* md, const tt_lplan::Plan& P, const uint32_t* mesh_indices,
                              uint32_t n_mesh_indices, const tt_light_transform* transforms) {
    for (uint32_t i = 0; i < n_mesh_indices; i++) {
        const tt_mesh_data& M = md[mesh_indices[i]];
        const tt_lplan::Tree& T = P.trees.at((uint32_t)M.LightNodeOffset);
        for (uint32_t k = 0; k < T.leaf_count; k++) {  // TransferKernel
            tt_light_tri& L = ltris[P.leaf_row[T.leaf_first + k]];
            const uint64_t agg = (uint64_t)L.TriTarget + (uint64_t)(uint32_t)M.TriOffset;
            tt_cuda_triangle zero;
            std::memset(&zero, 0, sizeof zero);
            tt_lr::transfer_tri(agg < n_tris ? tris[agg] : zero, L);
        }
        refit_tree_host<kCons>(nodes, P, T, [&](tt_light_node& nd) { tt_lr::mesh_leaf(ltris[T.start_index + (-(nd.left + 1))], nd); });
    }
    if (!transforms) return;
    tt_light_node zero;
    std::memset(&zero, 0, sizeof zero);
    refit_tree_host<kCons>(nodes, P, P.tlas, [&](tt_light_node& nd) {
        const tt_light_transform& X = transforms[-(nd.left + 1)];
        // (check_call: SolidOffset is the root of a mesh tree; the zero node stands for D3D's out-of-range read)
        const tt_light_node root = (uint32_t)X.SolidOffset < n_nodes ? nodes[X.SolidOffset] : zero;
        tt_lr::tlas_leaf<kCons>(X.Transform, root, nd);
    });
}

extern "C" {

tt_status tt_lights_refit_host(tt_light_node* nodes, uint32_t n_nodes, tt_light_tri* ltris, uint32_t n_ltris,
                               const tt_light_mesh* lmeshes, uint32_t n_lmeshes, const tt_cuda_triangle* tris, uint32_t n_tris,
                               const tt_mesh_data* meshdata, uint32_t n_mesh, const uint32_t* mesh_indices,
                               uint32_t n_mesh_indices, const tt_light_transform* transforms, uint32_t n_transforms,
                               uint32_t flags, char* why, uint32_t why_len) {
    std::string w;
    auto done = [&](tt_status st) {
        if (why && why_len) {
            std::strncpy(why, w.c_str(), why_len - 1);
            why[why_len - 1] = 0;
        }
        return st;
    };
    if (!tris) {
        w = "null triangles";
        return done(TT_ERR_INVALID_ARG);
    }
    const tt_lcheck::Lights L{nodes, n_nodes, ltris, n_ltris, lmeshes, n_lmeshes};
    if (tt_lcheck::validate(L, meshdata, n_mesh, n_tris, w) != TT_OK) return done(TT_ERR_INVALID_ARG);
    tt_lplan::Plan P;
    tt_lplan::build(L, meshdata, P);
    const tt_status st = tt_lplan::check_call(P, meshdata, n_mesh, n_lmeshes, n_nodes, mesh_indices, n_mesh_indices,
                                              transforms != nullptr, transforms, n_transforms, w);
    if (st != TT_OK) return done(st);
    if (flags & TT_LIGHT_REFIT_CONSERVATIVE)
        lights_refit_host<true>(nodes, n_nodes, ltris, tris, n_tris, meshdata, P, mesh_indices, n_mesh_indices, transforms);
    else
        lights_refit_host<false>(nodes, n_nodes, ltris, tris, n_tris, meshdata, P, mesh_indices, n_mesh_indices, transforms);
    return done(TT_OK);
}

tt_status tt_light_refit_math(uint32_t fn, const float* in, uint32_t n, float* out) {
    if (fn > 3u || (n && (!in || !out))) return TT_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; i++)
        out[i] = fn == 0u ? tt_lr::asin_pinned(in[i]) : fn == 1u ? tt_lr::acos_pinned(in[i]) : fn == 2u ? tt_lr::sin_pinned(in[i]) : tt_lr::cos_pinned(in[i]);
    return TT_OK;
}

}  // extern "C"
