// tt_build.hip — the BLAS builder's BVH2 stage on the GPU (builder half):
// BVH2Builder (BVH2Builder.cs:9-217) restated level by level, producing the SAME nodes and the
// same FinalIndices as the sequential C# recursion (and as host/tt_scene.cpp's restatement).
//
// The reference builds depth first: per node, a full SAH sweep over the node's primitives in each
// axis' presorted order (left-to-right running unions -> sah[i] = SA(left) * i, then right-to-left
// unions -> cost = sah[i] + SA(right) * (count - i), `cost <= best` so ties go to the lowest i and,
// across axes x, y, z, to the later axis), then a stable partition of the other two axes' index
// lists. Nothing in a node depends on its siblings, and a subtree of k primitives takes 2(k - 1)
// node slots of the depth-first numbering, so every node's slot is known when its parent splits.
// Here all nodes of one depth are split at once:
//  * the running unions are segmented scans (rocPRIM scan-by-key, one segment per node) whose
//    operator is AABB.Extend itself -- `if (b.min < a.min) a.min = b.min` keeps the EARLIER value
//    on ties (signed zeros included), which is associative, so the scan reproduces the sequential
//    unions bit for bit; NaN components never win an Extend, so they enter as the identity;
//  * the SAH cost is evaluated per position with the reference's expression (no contraction), and
//    the per-node argmin packs (order-preserving cost bits, position) into one 64-bit atomic min;
//  * the partition is a segmented exclusive count of left-going primitives (stable by construction).
// The three per-axis presorts (.NET's unstable introsort, whose tie order decides trees) stay on
// the host (tt_dotnet_sort_by_key); this file takes their output.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "tt_build.h"
#include "tt_ctx.h"

namespace {
thread_local char g_err[256];  // the failing step of the current build, for tt_last_error
}
const char* tt_build_error() { return g_err; }

namespace {

struct Box {
    float mx[3];  // BBMax (C# field order: BBMax then BBMin)
    float mn[3];  // BBMin
};

__host__ __device__ inline Box box_init() {
    Box b;
    for (int i = 0; i < 3; i++) {
        b.mx[i] = -FLT_MAX;  // float.MinValue
        b.mn[i] = FLT_MAX;
    }
    return b;
}

// CommonVars.AABB.Extend(AABB) (CommonVars.cs:304-402): `a` is the union so far, `b` the next box.
struct ExtendOp {
    __device__ Box operator()(const Box& a, const Box& b) const {
        Box r;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            r.mn[i] = b.mn[i] < a.mn[i] ? b.mn[i] : a.mn[i];
            r.mx[i] = b.mx[i] > a.mx[i] ? b.mx[i] : a.mx[i];
        }
        return r;
    }
};

// surface_area (BVH2Builder.cs): s = BBMax - BBMin; 2 * (s.x*s.y + s.x*s.z + s.y*s.z)
__device__ inline float surface_area(const Box& a) {
    const float sx = a.mx[0] - a.mn[0], sy = a.mx[1] - a.mn[1], sz = a.mx[2] - a.mn[2];
    return 2.0f * ((sx * sy) + (sx * sz) + (sy * sz));
}

// A primitive box as Extend sees it: a NaN component never replaces the running value, i.e. it acts
// like the identity's component.
__device__ inline Box prim_box(const Box& p) {
    Box b;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        b.mx[i] = p.mx[i] == p.mx[i] ? p.mx[i] : -FLT_MAX;
        b.mn[i] = p.mn[i] == p.mn[i] ? p.mn[i] : FLT_MAX;
    }
    return b;
}

struct Seg {
    int nodesi;      // BVH2Nodes slot of this node
    int node_index;  // first slot of its children's subtree (BuildRecursive's node_index)
    int first, count;
};

// position p -> the box of the primitive at p in axis order `idx` (identity outside live segments)
struct FwdBox {
    const int* idx;
    const Box* prims;
    const int* seg;
    __device__ Box operator()(int p) const { return seg[p] < 0 ? box_init() : prim_box(prims[idx[p]]); }
};
struct RevBox {
    const int* idx;
    const Box* prims;
    const int* seg;
    int n;
    __device__ Box operator()(int q) const {
        const int p = n - 1 - q;
        return seg[p] < 0 ? box_init() : prim_box(prims[idx[p]]);
    }
};
struct RevKey {
    const int* seg;
    int n;
    __device__ int operator()(int q) const { return seg[n - 1 - q]; }
};
// left-going flag of position p in axis d for segments that split on another axis (else 0)
struct LeftFlag {
    const int* idx;
    const int* seg;
    const int* dim;
    const unsigned char* going_left;
    int d;
    __device__ int operator()(int p) const {
        const int s = seg[p];
        return (s >= 0 && dim[s] != d) ? (int)going_left[idx[p]] : 0;
    }
};

__device__ inline uint32_t ordered_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float from_ordered(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

constexpr int kBlock = 256;

// A forest: M meshes over one concatenated primitive range, mesh m owning positions [starts[m], starts[m + 1]).
// Every stage below runs all meshes' nodes of one level together; a single build is the forest of one mesh.
struct Forest {
    const int* starts;  // M + 1
    int M;
};
__device__ inline int mesh_of(const Forest& F, int p) {  // the mesh that owns position p (no loads for M = 1)
    int lo = 0, hi = F.M - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (F.starts[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// a stage's failure: the stage-wide word the host reads every level, and the mesh that owns position p
__device__ inline void flag_mesh(int* err, int bit, int* mesh_err, const Forest& F, int p) {
    atomicOr(err, bit);
    atomicOr(mesh_err + mesh_of(F, p), 1);
}

// SAH cost of every split position of every live segment for one axis; per-segment argmin (lowest
// cost, then lowest relative index) by a 64-bit atomic min. pre[p] = union of the segment's
// positions [first, p]; sufr[n - 1 - p] = union of [p, end] (the reverse scan's output order).
__global__ void k_cost(int n, const int* __restrict__ seg, const Seg* __restrict__ segs, const Box* __restrict__ pre,
                       const Box* __restrict__ sufr, unsigned long long* __restrict__ best) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    int s = -1;
    unsigned long long key = ~0ull;
    if (p < n) {
        s = seg[p];
        if (s >= 0) {
            const Seg g = segs[s];
            const int rel = p - g.first;
            if (rel >= 1) {
                float cost = surface_area(pre[p - 1]) * (float)rel + surface_area(sufr[n - 1 - p]) * (float)(g.count - rel);
                if (cost <= FLT_MAX) {  // `cost <= split.cost` from float.MaxValue: +inf / NaN never split
                    if (cost == 0.0f) cost = 0.0f;  // -0 == +0 for the reference's compare
                    key = ((unsigned long long)ordered_bits(cost) << 32) | (uint32_t)rel;
                }
            }
        }
    }
    // one atomic per wave when the wave is inside one segment (the common case near the root)
    const int s0 = __builtin_amdgcn_readfirstlane(s);
    if (__ballot(s != s0) == 0ull) {
        if (s0 < 0) return;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(key, off, 64);
            key = o < key ? o : key;
        }
        if ((threadIdx.x & 63) == 0 && key != ~0ull) atomicMin(best + s0, key);
    } else if (s >= 0 && key != ~0ull) {
        atomicMin(best + s, key);
    }
}

// the best split of axis d of every segment: its cost, position and both unions
__global__ void k_candidate(int S, int n, const Seg* __restrict__ segs, const unsigned long long* __restrict__ best,
                            const Box* __restrict__ pre, const Box* __restrict__ sufr, float* __restrict__ c_cost,
                            int* __restrict__ c_pos, Box* __restrict__ c_left, Box* __restrict__ c_right) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const unsigned long long k = best[s];
    if (k == ~0ull) {
        c_pos[s] = -1;
        return;
    }
    const int p = segs[s].first + (int)(uint32_t)k;
    c_cost[s] = from_ordered((uint32_t)(k >> 32));
    c_pos[s] = p;
    c_left[s] = pre[p - 1];
    c_right[s] = sufr[n - 1 - p];
}

struct SplitOut {
    int split;  // first position of the right child, -1: no valid split (error)
    int dim;
    int n_next; // live children (count >= 2)
};

// partition_sah's axis choice (x, y, z in turn, `cost <= best`) and BuildRecursive's node writes:
// the node's child slots and boxes, leaf children (count 1) written at once.
__global__ void k_split(int S, const Seg* __restrict__ segs, const float* __restrict__ c_cost, const int* __restrict__ c_pos,
                        const Box* __restrict__ c_left, const Box* __restrict__ c_right, SplitOut* __restrict__ out,
                        Box* __restrict__ node_box, int* __restrict__ node_left, uint32_t* __restrict__ node_count,
                        int* __restrict__ err, Forest F, int level, int* __restrict__ mesh_depth,
                        int* __restrict__ mesh_err) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const int mesh = mesh_of(F, segs[s].first);
    mesh_depth[mesh] = level;  // the mesh has a live segment at this level (every writer stores the same value)
    float cost = FLT_MAX;
    int split = -1, dim = -1;
    Box L = box_init(), R = box_init();
    for (int d = 0; d < 3; d++) {
        const int pos = c_pos[d * S + s];
        if (pos >= 0 && c_cost[d * S + s] <= cost) {
            cost = c_cost[d * S + s];
            split = pos;
            dim = d;
            L = c_left[d * S + s];
            R = c_right[d * S + s];
        }
    }
    SplitOut o{split, dim, 0};
    if (split < 0) {  // the segment ends here (its positions leave every later level); its mesh fails
        atomicOr(err, 1);
        atomicOr(mesh_err + mesh, 1);
        out[s] = o;
        return;
    }
    const Seg g = segs[s];
    node_left[g.nodesi] = g.node_index;
    node_box[g.node_index] = L;
    node_box[g.node_index + 1] = R;
    const int n_left = split - g.first, n_right = g.first + g.count - split;
    if (n_left == 1) {
        node_left[g.node_index] = g.first;
        node_count[g.node_index] = 1u;
    }
    if (n_right == 1) {
        node_left[g.node_index + 1] = split;
        node_count[g.node_index + 1] = 1u;
    }
    o.n_next = (n_left >= 2 ? 1 : 0) + (n_right >= 2 ? 1 : 0);
    out[s] = o;
}

// next level's segments (children with >= 2 primitives, in parent order: left then right)
__global__ void k_children(int S, const Seg* __restrict__ segs, const SplitOut* __restrict__ so,
                           const int* __restrict__ base, Seg* __restrict__ next, int2* __restrict__ child_id) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const Seg g = segs[s];
    const SplitOut o = so[s];
    int b = base[s];
    const int n_left = o.split - g.first, n_right = g.first + g.count - o.split;
    int2 id = make_int2(-1, -1);
    if (o.split < 0) {  // no split (k_split flagged its mesh): no children
        child_id[s] = id;
        return;
    }
    if (n_left >= 2) {
        next[b] = Seg{g.node_index, g.node_index + 2, g.first, n_left};
        id.x = b++;
    }
    if (n_right >= 2) {
        next[b] = Seg{g.node_index + 1, g.node_index + 2 + 2 * (n_left - 1), o.split, n_right};
        id.y = b;
    }
    child_id[s] = id;
}

// indices_going_left[prim] = position < split, from the split axis' order
__global__ void k_flags(int n, const int* __restrict__ i0, const int* __restrict__ i1, const int* __restrict__ i2,
                        const int* __restrict__ seg, const SplitOut* __restrict__ so, unsigned char* __restrict__ going_left) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int s = seg[p];
    if (s < 0) return;
    const SplitOut o = so[s];
    const int* idx = o.dim == 0 ? i0 : (o.dim == 1 ? i1 : i2);
    going_left[idx[p]] = p < o.split ? 1 : 0;
}

// stable partition of axis d inside every segment that split on another axis
__global__ void k_scatter(int n, int d, const int* __restrict__ idx, const int* __restrict__ seg,
                          const Seg* __restrict__ segs, const SplitOut* __restrict__ so,
                          const unsigned char* __restrict__ going_left, const int* __restrict__ lrank,
                          int* __restrict__ out) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int s = seg[p];
    const int v = idx[p];
    if (s < 0 || so[s].dim == d || so[s].split < 0) {
        out[p] = v;
        return;
    }
    const int first = segs[s].first, split = so[s].split;
    const int r = lrank[p];
    out[going_left[v] ? first + r : split + (p - first - r)] = v;
}

__global__ void k_reseg(int n, int* __restrict__ seg, const SplitOut* __restrict__ so, const int2* __restrict__ child_id) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int s = seg[p];
    if (s < 0) return;
    const int2 id = child_id[s];
    seg[p] = p < so[s].split ? id.x : id.y;
}

// every position's first segment (seg_id: the mesh's root segment, -1 for a one-primitive mesh)
__global__ void k_seg_of_mesh(int n, Forest F, const int* __restrict__ seg_id, int* __restrict__ seg) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p < n) seg[p] = seg_id[mesh_of(F, p)];
}

__global__ void k_dim_of(int S, const SplitOut* __restrict__ so, int* __restrict__ dim) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s < S) dim[s] = so[s].dim;
}

template <class T>
struct DBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t k) {
        n = k;
        return hipMalloc(&p, std::max<size_t>(k, 1) * sizeof(T));
    }
    ~DBuf() {
        if (p) (void)hipFree(p);
    }
};

inline unsigned grid_of(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

// ------------------------------------------------------------------------------- BVH8 stage
// BVH8Builder (BVH8Builder.cs:30-392) restated for the GPU: the cost pass bottom up over the BVH2's
// depth levels, the collapse top down over the CWBVH8's levels. The sequential collapse numbers the
// nodes and the leaf triangles with two running counters in depth-first order; here each CWBVH8 node
// first learns how many nodes (A) and triangles (T) its subtree allocates (bottom up), then its
// counters on entry (top down), so every node is written independently with the reference's numbers.

__device__ inline float surface_area_h(const Box& a) { return surface_area(a); }

// BFS of the BVH2 from the root: lvl_out gets the internal children of the frontier's internal nodes
__global__ void k_bvh2_level(int m, const int* __restrict__ frontier, const int* __restrict__ left,
                             const uint32_t* __restrict__ count, int* __restrict__ next, int* __restrict__ n_next,
                             int cap) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= m) return;
    const int v = frontier[t];
    if (count[v] > 0) return;
    const int l = left[v];
    const int o = atomicAdd(n_next, 2);
    if (o + 1 >= cap) return;  // not a tree: the host sees the count and fails
    next[o] = l;
    next[o + 1] = l + 1;
}

struct Dec {
    int8_t type, dl, dr;  // 0 LEAF, 1 INTERNAL, 2 DISTRIBUTE
};

// calculate_cost (BVH8Builder.cs) of one BVH2 node whose children are done; nprim / firstpos: the
// subtree's primitive count and first leaf position (count_primitives' range)
__global__ void k_cost8(int m, const int* __restrict__ nodes_lvl, const Box* __restrict__ box, const int* __restrict__ left,
                        const uint32_t* __restrict__ count, float* __restrict__ cost, Dec* __restrict__ dec,
                        int* __restrict__ nprim, int* __restrict__ firstpos, int* __restrict__ err, Forest F,
                        int* __restrict__ mesh_err) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= m) return;
    const int v = nodes_lvl[t];
    const Box a = box[v];
    if (count[v] > 0) {
        const int np = (int)count[v];
        nprim[v] = np;
        firstpos[v] = left[v];
        if (np != 1) {
            flag_mesh(err, 2, mesh_err, F, v >> 1);  // node slot v belongs to the mesh of position v / 2
            return;
        }
        const float cl = surface_area(a) * (float)np;
        for (int i = 0; i < 7; i++) {
            cost[(size_t)v * 7 + i] = cl;
            dec[(size_t)v * 7 + i] = Dec{0, 0, 0};
        }
        return;
    }
    const int l = left[v], r = l + 1;
    const int np = nprim[l] + nprim[r];
    nprim[v] = np;
    firstpos[v] = firstpos[l];
    const float cost_leaf = np <= 3 ? (float)np * surface_area(a) : FLT_MAX;
    float cost_distribute = FLT_MAX;
    int dist_left = -1, dist_right = -1;
    for (int k = 0; k < 7; k++) {
        const float c = cost[(size_t)l * 7 + k] + cost[(size_t)r * 7 + 6 - k];
        if (c < cost_distribute) {
            cost_distribute = c;
            dist_left = k;
            dist_right = 6 - k;
        }
    }
    const float cost_internal = cost_distribute + surface_area(a);
    Dec d0;
    if (cost_leaf < cost_internal) {
        cost[(size_t)v * 7] = cost_leaf;
        d0.type = 0;
    } else {
        cost[(size_t)v * 7] = cost_internal;
        d0.type = 1;
    }
    d0.dl = (int8_t)dist_left;
    d0.dr = (int8_t)dist_right;
    dec[(size_t)v * 7] = d0;
    Dec prev = d0;
    for (int i = 1; i < 7; i++) {
        float cd = cost[(size_t)v * 7 + i - 1];
        int dl = -1, dr = -1;
        for (int k = 0; k < i; k++) {
            const float c = cost[(size_t)l * 7 + k] + cost[(size_t)r * 7 + i - k - 1];
            if (c < cd) {
                cd = c;
                dl = k;
                dr = i - k - 1;
            }
        }
        cost[(size_t)v * 7 + i] = cd;
        if (dl != -1) prev = Dec{2, (int8_t)dl, (int8_t)dr};
        dec[(size_t)v * 7 + i] = prev;
    }
}

struct Rec8 {
    int bvh2;       // the BVH2 node this CWBVH8 node collapses
    int child[8];   // BVH2 children by slot (order_children), -1 empty
    int crec[8];    // records of the internal children by internal rank
    int k, t;       // internal children, triangles of the leaf children
    int A, T;       // CWBVH8 nodes / triangles the subtree's collapse allocates
    int idx, C, Ct; // node index, node and triangle counters on entry to collapse()
};

// get_children + order_children + the child checks of collapse() for one CWBVH8 node; appends its
// internal children as records of the next level.
__global__ void k_expand8(int lo, int hi, int cap, Rec8* __restrict__ rec, int* __restrict__ n_rec, const Box* __restrict__ box,
                          const int* __restrict__ left, const uint32_t* __restrict__ count, const Dec* __restrict__ dec,
                          const int* __restrict__ nprim, int* __restrict__ err, Forest F, int* __restrict__ mesh_err) {
    const int x = lo + blockIdx.x * kBlock + threadIdx.x;
    if (x >= hi) return;
    Rec8& R = rec[x];
    const int N = R.bvh2;
    int children[8];
    int cc = 0;
    bool ok = true;
    if (count[N] > 0) {
        children[cc++] = N;
    } else {
        int stn[24], sti[24], sp = 0;  // pending (node, i) expansions, processed depth first
        stn[sp] = N;
        sti[sp] = 0;
        sp++;
        bool root = true;
        while (sp > 0 && ok) {
            sp--;
            const int v = stn[sp], i = sti[sp];
            if (!root && dec[(size_t)v * 7 + i].type != 2) {  // a plain child
                if (cc >= 8) { ok = false; break; }
                children[cc++] = v;
                continue;
            }
            root = false;
            const Dec d = dec[(size_t)v * 7 + i];
            if (!(d.dl >= 0 && d.dl < 7) || !(d.dr >= 0 && d.dr < 7) || cc >= 8) { ok = false; break; }
            const int l = left[v];
            stn[sp] = l + 1; sti[sp] = d.dr; sp++;  // right after left
            stn[sp] = l; sti[sp] = d.dl; sp++;
        }
    }
    if (!ok) { flag_mesh(err, 4, mesh_err, F, N >> 1); return; }
    // order_children: greedy slot assignment by octant direction costs
    const Box nb = box[N];
    const float px = (nb.mx[0] + nb.mn[0]) / 2.0f, py = (nb.mx[1] + nb.mn[1]) / 2.0f, pz = (nb.mx[2] + nb.mn[2]) / 2.0f;
    float cost2[8][8];
    for (int c = 0; c < cc; c++) {
        const Box ca = box[children[c]];
        const float dx = (ca.mx[0] + ca.mn[0]) / 2.0f - px, dy = (ca.mx[1] + ca.mn[1]) / 2.0f - py,
                    dz = (ca.mx[2] + ca.mn[2]) / 2.0f - pz;
        for (int s = 0; s < 8; s++) {
            const float sx = ((s >> 2) & 1) ? -1.0f : 1.0f, sy = ((s >> 1) & 1) ? -1.0f : 1.0f, sz = (s & 1) ? -1.0f : 1.0f;
            cost2[c][s] = dx * sx + dy * sy + dz * sz;
        }
    }
    int assignment[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    bool slot_filled[8] = {false, false, false, false, false, false, false, false};
    while (true) {
        float min_cost = FLT_MAX;
        int min_slot = -1, min_index = -1;
        for (int c = 0; c < cc; c++) {
            if (assignment[c] != -1) continue;
            for (int s = 0; s < 8; s++) {
                if (!slot_filled[s] && cost2[c][s] < min_cost) {
                    min_cost = cost2[c][s];
                    min_slot = s;
                    min_index = c;
                }
            }
        }
        if (min_slot == -1) break;
        slot_filled[min_slot] = true;
        assignment[min_index] = min_slot;
    }
    int slots[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    for (int c = 0; c < cc; c++) {
        if (assignment[c] < 0) { flag_mesh(err, 8, mesh_err, F, N >> 1); return; }  // a child no slot could take (NaN boxes)
        slots[assignment[c]] = children[c];
    }
    int k = 0, t = 0;
    for (int s = 0; s < 8; s++) {
        R.child[s] = slots[s];
        const int c = slots[s];
        if (c < 0) continue;
        const int ty = dec[(size_t)c * 7].type;
        if (ty == 0) {
            const int tc = nprim[c];
            if (!(tc > 0 && tc <= 3)) { flag_mesh(err, 16, mesh_err, F, N >> 1); return; }
            t += tc;
            if (t > 24) { flag_mesh(err, 16, mesh_err, F, N >> 1); return; }
        } else if (ty == 1) {
            const int o = atomicAdd(n_rec, 1);
            if (o >= cap) { flag_mesh(err, 128, mesh_err, F, N >> 1); return; }
            rec[o].bvh2 = c;
            R.crec[k++] = o;
        } else {
            flag_mesh(err, 32, mesh_err, F, N >> 1);
            return;
        }
    }
    R.k = k;
    R.t = t;
}

__global__ void k_up8(int lo, int hi, Rec8* __restrict__ rec) {
    const int x = lo + blockIdx.x * kBlock + threadIdx.x;
    if (x >= hi) return;
    Rec8& R = rec[x];
    int A = R.k, T = R.t;
    for (int r = 0; r < R.k; r++) {
        A += rec[R.crec[r]].A;
        T += rec[R.crec[r]].T;
    }
    R.A = A;
    R.T = T;
}

__global__ void k_down8(int lo, int hi, Rec8* __restrict__ rec) {
    const int x = lo + blockIdx.x * kBlock + threadIdx.x;
    if (x >= hi) return;
    const Rec8& R = rec[x];
    int C = R.C + R.k, Ct = R.Ct + R.t;
    for (int r = 0; r < R.k; r++) {
        Rec8& c = rec[R.crec[r]];
        c.idx = R.C + r;
        c.C = C;
        c.Ct = Ct;
        C += c.A;
        Ct += c.T;
    }
}

// Mathf.Log2 / Ceil / Floor / Pow: float wrappers over System.Math (double)
__device__ inline float mathf_log2(float f) { return (float)(log((double)f) / log(2.0)); }
__device__ inline float mathf_ceil(float f) { return (float)ceil((double)f); }
__device__ inline float mathf_floor(float f) { return (float)floor((double)f); }
__device__ inline float mathf_pow2(float p) { return (float)pow(2.0, (double)p); }
// (byte)(uint)x of a C# float (unchecked): truncate toward zero, wrap to 8 bits
__device__ inline uint32_t to_byte(float x) {
    if (!(x == x)) return 0u;
    if (x <= -1.0f || x >= 4294967296.0f) return 0u;
    return (uint32_t)x & 0xffu;
}

// Every mesh's node total (its root record's subtree plus the root; the first M records are the roots, in mesh
// order), their exclusive scan -- the meshes' node bases, node_base[M] the total -- and the root boxes. One block:
// each thread sums a contiguous run of meshes, the block scans the sums.
__global__ __launch_bounds__(kBlock) void k_mesh_totals(Forest F, const Rec8* __restrict__ rec, const Box* __restrict__ box,
                                                        int* __restrict__ node_base, Box* __restrict__ root_box) {
    using Scan = rocprim::block_scan<int, kBlock>;
    __shared__ typename Scan::storage_type tmp;
    const int per = (F.M + kBlock - 1) / kBlock;
    const int lo = min((int)threadIdx.x * per, F.M), hi = min(lo + per, F.M);
    int sum = 0;
    for (int m = lo; m < hi; m++) {
        sum += rec[m].A + 1;
        root_box[m] = box[2 * F.starts[m]];
    }
    int base = 0;
    Scan().exclusive_scan(sum, base, 0, tmp);
    for (int m = lo; m < hi; m++) {
        node_base[m] = base;
        base += rec[m].A + 1;
    }
    if (threadIdx.x == kBlock - 1) node_base[F.M] = base;  // (the threads past the last mesh add nothing)
}

// collapse()'s node body + Aggregate (CommonVars.cs:662-688): the 80-B node at R.idx, and the leaf
// children's primitives (count_primitives) at cwbvh_indices[R.Ct ...]; both numbered within the record's
// mesh, whose nodes start at node_base[mesh] and whose leaf positions start at starts[mesh]
__global__ void k_fill8(int m, const Rec8* __restrict__ rec, const Box* __restrict__ box, const Dec* __restrict__ dec,
                        const int* __restrict__ nprim, const int* __restrict__ firstpos, const int* __restrict__ final_idx,
                        tt_cwbvh_node* __restrict__ out, int* __restrict__ cwbvh_indices, int* __restrict__ err, Forest F,
                        const int* __restrict__ node_base, int* __restrict__ mesh_err) {
    const int x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= m) return;
    const Rec8& R = rec[x];
    const int mesh = mesh_of(F, R.bvh2 >> 1);
    const int leaf0 = F.starts[mesh] + R.Ct;
    const Box a = box[R.bvh2];
    const float denom = 1.0f / (float)((1 << 8) - 1);
    const float ex = mathf_pow2(mathf_ceil(mathf_log2((a.mx[0] - a.mn[0]) * denom)));
    const float ey = mathf_pow2(mathf_ceil(mathf_log2((a.mx[1] - a.mn[1]) * denom)));
    const float ez = mathf_pow2(mathf_ceil(mathf_log2((a.mx[2] - a.mn[2]) * denom)));
    const float ox = 1.0f / ex, oy = 1.0f / ey, oz = 1.0f / ez;
    const uint32_t ux = __float_as_uint(ex), uy = __float_as_uint(ey), uz = __float_as_uint(ez);
    if ((ux & 0x807FFFFFu) || (uy & 0x807FFFFFu) || (uz & 0x807FFFFFu)) {
        atomicOr(err, 64);
        atomicOr(mesh_err + mesh, 1);
        return;
    }
    uint32_t meta[2] = {0u, 0u}, qlx[2] = {0u, 0u}, qhx[2] = {0u, 0u}, qly[2] = {0u, 0u}, qhy[2] = {0u, 0u},
             qlz[2] = {0u, 0u}, qhz[2] = {0u, 0u};
    uint32_t imask = 0;
    int internal = 0, tri = 0;
    for (int s = 0; s < 8; s++) {
        const int c = R.child[s];
        if (c < 0) continue;
        const Box ca = box[c];
        const int w = s >> 2, sh = (s & 3) * 8;
        qlx[w] |= to_byte(mathf_floor((ca.mn[0] - a.mn[0]) * ox)) << sh;
        qly[w] |= to_byte(mathf_floor((ca.mn[1] - a.mn[1]) * oy)) << sh;
        qlz[w] |= to_byte(mathf_floor((ca.mn[2] - a.mn[2]) * oz)) << sh;
        qhx[w] |= to_byte(mathf_ceil((ca.mx[0] - a.mn[0]) * ox)) << sh;
        qhy[w] |= to_byte(mathf_ceil((ca.mx[1] - a.mn[1]) * oy)) << sh;
        qhz[w] |= to_byte(mathf_ceil((ca.mx[2] - a.mn[2]) * oz)) << sh;
        uint32_t mb;
        if (dec[(size_t)c * 7].type == 0) {
            const int tc = nprim[c], f = firstpos[c];
            mb = 0u;
            for (int j = 0; j < tc; j++) {
                mb |= 1u << (j + 5);
                cwbvh_indices[leaf0 + tri + j] = final_idx[f + j];
            }
            mb |= (uint32_t)tri;
            tri += tc;
        } else {
            mb = (uint32_t)((internal + 24) | 0x20);
            imask |= (1u << internal) & 0xffu;
            internal++;
        }
        meta[w] |= (mb & 0xffu) << sh;
    }
    tt_cwbvh_node o;
    o.p[0] = a.mn[0];
    o.p[1] = a.mn[1];
    o.p[2] = a.mn[2];
    o.e_imask = (ux >> 23) | ((uy >> 23) << 8) | ((uz >> 23) << 16) | (imask << 24);
    o.base_child = (uint32_t)R.C;
    o.base_tri = (uint32_t)R.Ct;
    o.meta[0] = meta[0]; o.meta[1] = meta[1];
    o.qlo_x[0] = qlx[0]; o.qlo_x[1] = qlx[1]; o.qhi_x[0] = qhx[0]; o.qhi_x[1] = qhx[1];
    o.qlo_y[0] = qly[0]; o.qlo_y[1] = qly[1]; o.qhi_y[0] = qhy[0]; o.qhi_y[1] = qhy[1];
    o.qlo_z[0] = qlz[0]; o.qlo_z[1] = qlz[1]; o.qhi_z[0] = qhz[0]; o.qhi_z[1] = qhz[1];
    out[node_base[mesh] + R.idx] = o;
}

// ------------------------------------------------------------------------ presort (introsort)
// .NET Framework's ArraySortHelper IntrospectiveSort with BVH2Builder's float-key Comparison
// (BVH2Builder.cs:137-147; host restatement DotNetSort in host/tt_scene.cpp), run level by level.
// The sort is unstable, so its output order of equal keys is whatever its exact sequence of swaps
// produces -- the GPU must replay that sequence, not just sort. Partitions of one recursion level are
// disjoint and independent, so they run together; within a partition, PickPivotAndPartition's
// two-pointer scan is replayed in closed form: after the median-of-three and the pivot parked at
// hi - 1, the k-th stop of the left pointer is the k-th position (from lo + 1) whose key is >= the
// pivot's (a_k), the k-th stop of the right pointer the k-th position (from hi - 2 down) whose key
// is <= it (b_k); pairs k < K swap, where K is the first k with a_k >= b_k, and the pivot lands at
// min(a_K, b_(K-1)) (b_0 = hi - 1). Small partitions (<= 16) and partitions whose depth limit ran
// out (heapsort) are finished by one thread each, exactly as the sequential code does them.
struct SortPart {
    int lo, hi, depth;
};

__device__ inline int key_cmp(const float* __restrict__ k, int a, int b) {  // KeyCmp
    const float sign = k[a] - k[b];
    return sign < 0 ? -1 : (sign == 0 ? 0 : 1);
}
// position p of the 3n-long index array -> the axis it sorts (keys of axis d at cent + d * n)
__device__ inline const float* axis_keys(const float* cent, int n, int p) { return cent + (size_t)(p / n) * n; }

__device__ void swap_if_greater(int* it, const float* k, int a, int b) {
    if (a != b && key_cmp(k, it[a], it[b]) > 0) {
        const int t = it[a];
        it[a] = it[b];
        it[b] = t;
    }
}
__device__ void small_sort(int* it, const float* k, int lo, int hi) {  // IntroSort's <= 16 branch
    const int size = hi - lo + 1;
    if (size <= 1) return;
    if (size == 2) {
        swap_if_greater(it, k, lo, hi);
        return;
    }
    if (size == 3) {
        swap_if_greater(it, k, lo, hi - 1);
        swap_if_greater(it, k, lo, hi);
        swap_if_greater(it, k, hi - 1, hi);
        return;
    }
    for (int i = lo; i < hi; i++) {  // InsertionSort
        int j = i;
        const int t = it[i + 1];
        while (j >= lo && key_cmp(k, t, it[j]) < 0) {
            it[j + 1] = it[j];
            j--;
        }
        it[j + 1] = t;
    }
}
__device__ void down_heap(int* it, const float* k, int i, int n, int lo) {
    const int d = it[lo + i - 1];
    while (i <= n / 2) {
        int child = 2 * i;
        if (child < n && key_cmp(k, it[lo + child - 1], it[lo + child]) < 0) child++;
        if (!(key_cmp(k, d, it[lo + child - 1]) < 0)) break;
        it[lo + i - 1] = it[lo + child - 1];
        i = child;
    }
    it[lo + i - 1] = d;
}
__device__ void heap_sort(int* it, const float* k, int lo, int hi) {
    const int n = hi - lo + 1;
    for (int i = n / 2; i >= 1; i--) down_heap(it, k, i, n, lo);
    for (int i = n; i > 1; i--) {
        const int t = it[lo];
        it[lo] = it[lo + i - 1];
        it[lo + i - 1] = t;
        down_heap(it, k, 1, i - 1, lo);
    }
}

// median of three, the pivot parked at hi - 1; pk = the pivot item
__global__ void k_pivot(int P, const SortPart* __restrict__ parts, int* __restrict__ it, const float* __restrict__ cent,
                        int n, int* __restrict__ pk) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= P) return;
    const SortPart q = parts[s];
    const float* k = axis_keys(cent, n, q.lo);
    const int middle = q.lo + ((q.hi - q.lo) >> 1);
    swap_if_greater(it, k, q.lo, middle);
    swap_if_greater(it, k, q.lo, q.hi);
    swap_if_greater(it, k, middle, q.hi);
    const int pivot = it[middle];
    if (middle != q.hi - 1) {
        it[middle] = it[q.hi - 1];
        it[q.hi - 1] = pivot;
    }
    pk[s] = pivot;
}

// left-pointer stops (ge: key >= pivot, over [lo+1, hi-1]) and right-pointer stops (le: key <=
// pivot, over [lo, hi-2]) as 0/1 flags
struct GeFlag {
    const int* it;
    const int* part;
    const SortPart* parts;
    const int* pk;
    const float* cent;
    int n;
    __device__ int operator()(int p) const {
        const int s = part[p];
        if (s < 0) return 0;
        const SortPart q = parts[s];
        if (p < q.lo + 1 || p > q.hi - 1) return 0;
        const float* k = axis_keys(cent, n, p);
        return key_cmp(k, it[p], pk[s]) < 0 ? 0 : 1;
    }
};
struct LeFlagRev {  // indexed by q = 3n - 1 - p (the right pointer's direction)
    const int* it;
    const int* part;
    const SortPart* parts;
    const int* pk;
    const float* cent;
    int n, n3;
    __device__ int operator()(int qi) const {
        const int p = n3 - 1 - qi;
        const int s = part[p];
        if (s < 0) return 0;
        const SortPart q = parts[s];
        if (p < q.lo || p > q.hi - 2) return 0;
        const float* k = axis_keys(cent, n, p);
        return key_cmp(k, pk[s], it[p]) < 0 ? 0 : 1;
    }
};
struct PartKeyRev {
    const int* part;
    int n3;
    __device__ int operator()(int qi) const { return part[n3 - 1 - qi]; }
};

// aList[lo + k] = k-th left stop, bList[lo + k] = k-th right stop (k from 0)
__global__ void k_stops(int n3, const int* __restrict__ part, const SortPart* __restrict__ parts, const int* __restrict__ it,
                        const int* __restrict__ pk, const float* __restrict__ cent, int n, const int* __restrict__ gerank,
                        const int* __restrict__ lerank_rev, int* __restrict__ alist, int* __restrict__ blist) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n3) return;
    const int s = part[p];
    if (s < 0) return;
    const SortPart q = parts[s];
    const float* k = axis_keys(cent, n, p);
    if (p >= q.lo + 1 && p <= q.hi - 1 && key_cmp(k, it[p], pk[s]) >= 0) alist[q.lo + gerank[p]] = p;
    if (p >= q.lo && p <= q.hi - 2 && key_cmp(k, pk[s], it[p]) >= 0) blist[q.lo + lerank_rev[n3 - 1 - p]] = p;
}

// K (first k with a_k >= b_k) by binary search; the swap count K - 1 and the pivot's final slot
__global__ void k_crossing(int P, const SortPart* __restrict__ parts, const int* __restrict__ gerank,
                           const int* __restrict__ lerank_rev, const int* __restrict__ alist, const int* __restrict__ blist,
                           int n3, int2* __restrict__ res) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= P) return;
    const SortPart q = parts[s];
    const int cnt_ge = gerank[q.hi - 1] + 1;       // hi - 1 (the pivot) is always a stop
    const int cnt_le = lerank_rev[n3 - 1 - q.lo] + 1;  // lo (<= pivot after the median of three) is too
    auto pred = [&](int K) {  // a_K >= b_K (1-based K); b_K = -1 past the last right stop
        const int a = alist[q.lo + K - 1];
        const int b = K <= cnt_le ? blist[q.lo + K - 1] : -1;
        return a >= b;
    };
    int lo = 1, hi = cnt_ge;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pred(mid)) hi = mid;
        else lo = mid + 1;
    }
    const int K = lo;
    const int aK = alist[q.lo + K - 1];
    const int bK1 = K >= 2 ? blist[q.lo + K - 2] : q.hi - 1;
    res[s] = make_int2(K - 1, aK < bK1 ? aK : bK1);
}

__global__ void k_pswap(int n3, const int* __restrict__ part, const SortPart* __restrict__ parts, const int2* __restrict__ res,
                        const int* __restrict__ alist, const int* __restrict__ blist, int* __restrict__ it) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n3) return;
    const int s = part[p];
    if (s < 0) return;
    const int kk = p - parts[s].lo;
    if (kk >= res[s].x) return;
    const int a = alist[p], b = blist[p];
    const int t = it[a];
    it[a] = it[b];
    it[b] = t;
}

// the pivot into its slot; children: finished here (<= 16, or heapsort at depth 0) or the next level
__global__ void k_children_sort(int P, const SortPart* __restrict__ parts, const int2* __restrict__ res, int* __restrict__ it,
                                const float* __restrict__ cent, int n, SortPart* __restrict__ next, int* __restrict__ n_next,
                                int2* __restrict__ child, int* __restrict__ err, Forest F, int* __restrict__ mesh_err) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= P) return;
    const SortPart q = parts[s];
    const int left = res[s].y;
    if (left != q.hi - 1) {
        const int t = it[left];
        it[left] = it[q.hi - 1];
        it[q.hi - 1] = t;
    }
    const float* k = axis_keys(cent, n, q.lo);
    const int d = q.depth - 1;
    int2 id = make_int2(-1, -1);
    const int bounds[2][2] = {{q.lo, left - 1}, {left + 1, q.hi}};
    for (int c = 0; c < 2; c++) {
        const int lo = bounds[c][0], hi = bounds[c][1];
        const int size = hi - lo + 1;
        if (size <= 16) {
            small_sort(it, k, lo, hi);
        } else if (d == 0) {
            if (size > 65536) flag_mesh(err, 1, mesh_err, F, lo - (lo / n) * n);  // left to the host: one thread would take too long
            else heap_sort(it, k, lo, hi);
        } else {
            const int o = atomicAdd(n_next, 1);
            next[o] = SortPart{lo, hi, d};
            if (c == 0) id.x = o;
            else id.y = o;
        }
    }
    child[s] = id;
}

__global__ void k_repart(int n3, int* __restrict__ part, const int2* __restrict__ res, const int2* __restrict__ child) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n3) return;
    const int s = part[p];
    if (s < 0) return;
    const int left = res[s].y;
    part[p] = p < left ? child[s].x : (p > left ? child[s].y : -1);
}

// BVH2Builder's centroids, (max - min) / 2 + min per axis, axis-major; flags non-finite keys. sorted (nullable:
// every mesh) marks the meshes this presort sorts: the others' lists are the caller's and stay untouched.
__global__ void k_centroids(int n, const Box* __restrict__ prims, float* __restrict__ cent, int* __restrict__ it,
                            int* __restrict__ bad, Forest F, const unsigned char* __restrict__ sorted,
                            int* __restrict__ mesh_err) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (sorted && !sorted[mesh_of(F, i)]) return;
    const Box b = prims[i];
    for (int d = 0; d < 3; d++) {
        const float c = (b.mx[d] - b.mn[d]) / 2.0f + b.mn[d];
        cent[(size_t)d * n + i] = c;
        it[(size_t)d * n + i] = i;
        if (!(c - c == 0.0f)) flag_mesh(bad, 1, mesh_err, F, i);  // NaN or infinity: the comparator is not an order there
    }
}

// the root partitions, one per (mesh, axis): position p of the 3n-long index array belongs to axis p / n and to
// the mesh of p % n; root_id is -1 where no partition is live (a caller's list, or at most 16 elements)
__global__ void k_part_of_root(int n3, int n, Forest F, const int* __restrict__ root_id, int* __restrict__ part) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n3) return;
    const int d = p / n;
    part[p] = root_id[d * F.M + mesh_of(F, p - d * n)];
}

// a root partition of at most 16 elements is IntroSort's small branch at once
__global__ void k_small_roots(int P, const SortPart* __restrict__ parts, int* __restrict__ it, const float* __restrict__ cent,
                              int n) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= P) return;
    const SortPart q = parts[s];
    small_sort(it, axis_keys(cent, n, q.lo), q.lo, q.hi);
}

// exclusive-scan input: live children per segment (0 past the last segment, so base[S] = total)
struct NextCount {
    const SplitOut* so;
    int S;
    __device__ int operator()(int q) const { return q < S ? so[q].n_next : 0; }
};

#define TT_BH(x)                                                                                  \
    do {                                                                                          \
        const hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) {                                                                   \
            std::snprintf(g_err, sizeof(g_err), "%s: %s", #x, hipGetErrorString(e_));             \
            return e_ == hipErrorOutOfMemory ? TT_ERR_OOM : TT_ERR_HIP;                            \
        }                                                                                         \
    } while (0)
#define TT_BFAIL(status, msg)                                  \
    do {                                                       \
        std::snprintf(g_err, sizeof(g_err), "%s", msg);        \
        return status;                                         \
    } while (0)

// A stage's failure per mesh: every flagged mesh gets `code` in mesh_status (nullable), and the stage's message
// names the lowest of them.
static tt_status report_meshes(hipStream_t st, const int* mesh_err_dev, int M, tt_status code, const char* what,
                               tt_status* mesh_status) {
    std::vector<int> f((size_t)M, 0);
    TT_BH(hipMemcpyAsync(f.data(), mesh_err_dev, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, st));
    TT_BH(hipStreamSynchronize(st));
    int first = -1;
    for (int m = 0; m < M; m++) {
        if (!f[m]) continue;
        if (first < 0) first = m;
        if (mesh_status) mesh_status[m] = code;
    }
    std::snprintf(g_err, sizeof(g_err), "%s (mesh %d)", what, first);
    return code;
}

// The BVH2 stage's result, left on the device for the BVH8 stage: BVH2Nodes (boxes, left, count; 2n slots, mesh
// m's at [2 * start_m, 2 * (start_m + n_m)), child slots and leaf positions global) and FinalIndices (global
// primitive indices).
struct Bvh2Dev {
    DBuf<Box> box;
    DBuf<int> left, final_idx;
    DBuf<int> per_mesh;  // one allocation for the four per-mesh arrays: starts, root segments, error flags, depths
    int* starts = nullptr;    // M + 1
    int* mesh_err = nullptr;  // M
    DBuf<uint32_t> count;
    std::vector<uint32_t> depth;  // per mesh: the levels at which it still had a live segment
};

// position i -> Extend(identity, primitive i): what the sequential union makes of one box
struct RootBox {
    const Box* prims;
    __device__ Box operator()(int i) const { return ExtendOp()(box_init(), prims[i]); }
};
// BVH2Nodes[0] of every mesh: the last element of its slice of the root scan; a one-primitive mesh's root is the
// leaf itself (BuildRecursive(0, 2, 0, 1, 0))
__global__ void k_mesh_roots(Forest F, const Box* __restrict__ prims, const Box* __restrict__ pre, Box* __restrict__ node_box,
                             int* __restrict__ node_left, uint32_t* __restrict__ node_count) {
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= F.M) return;
    const int s = F.starts[m], c = F.starts[m + 1] - s;
    if (c >= 2) {
        node_box[2 * s] = pre[s + c - 1];
    } else {
        node_box[2 * s] = RootBox{prims}(s);
        node_left[2 * s] = s;
        node_count[2 * s] = 1u;
    }
}

// prims (n boxes, n = start[M]) and presorted (3 x n, axis-major over n, global primitive indices) are device
// arrays; start (M + 1) is a host array. Everything the stage makes stays on the device.
static tt_status bvh2_stage(hipStream_t st, const Box* prims_p, const uint32_t* start, int M, const int32_t* presorted,
                            Bvh2Dev& R, tt_status* mesh_status) {
    const int n = (int)start[M];
    const size_t n2 = 2 * (size_t)n;
    int depth = 0;
    TT_BH(R.box.alloc(n2));
    TT_BH(R.left.alloc(n2));
    TT_BH(R.count.alloc(n2));
    TT_BH(R.final_idx.alloc(n));
    TT_BH(R.per_mesh.alloc(4 * (size_t)M + 1));
    R.starts = R.per_mesh.p;
    int* const seg_id = R.starts + M + 1;
    R.mesh_err = seg_id + M;
    int* const mesh_depth = R.mesh_err + M;
    // starts, then every mesh's root segment (one primitive: the root is a leaf, no segment): one upload
    std::vector<int> hmesh(start, start + M + 1);
    hmesh.resize(2 * (size_t)M + 1, -1);
    std::vector<Seg> roots;
    for (int m = 0; m < M; m++) {
        const int s = hmesh[m], c = hmesh[m + 1] - s;
        if (c < 2) continue;
        hmesh[(size_t)M + 1 + m] = (int)roots.size();
        roots.push_back(Seg{2 * s, 2 * s + 2, s, c});
    }
    const Forest F{R.starts, M};
    DBuf<Box> pre, sufr, c_left, c_right;
    DBuf<int> idxb[4], seg, lrank, c_pos, dimv, base, err;
    Box* box_p = R.box.p;
    int* nleft_p = R.left.p;
    uint32_t* ncount_p = R.count.p;
    DBuf<unsigned char> going_left;
    DBuf<Seg> segs, next;
    DBuf<SplitOut> so;
    DBuf<unsigned long long> best;
    DBuf<float> c_cost;
    DBuf<int2> child_id;
    const size_t smax = (size_t)n / 2 + 1;  // live segments per level (>= 2 primitives each)
    TT_BH(pre.alloc(n));
    TT_BH(sufr.alloc(n));
    for (auto& b : idxb) TT_BH(b.alloc(n));
    TT_BH(seg.alloc(n));
    TT_BH(lrank.alloc(n));
    TT_BH(going_left.alloc(n));
    TT_BH(segs.alloc(smax));
    TT_BH(next.alloc(smax));
    TT_BH(so.alloc(smax));
    TT_BH(best.alloc(3 * smax));
    TT_BH(c_cost.alloc(3 * smax));
    TT_BH(c_pos.alloc(3 * smax));
    TT_BH(c_left.alloc(3 * smax));
    TT_BH(c_right.alloc(3 * smax));
    TT_BH(dimv.alloc(smax));
    TT_BH(base.alloc(smax + 1));
    TT_BH(child_id.alloc(smax));
    TT_BH(err.alloc(1));
    int* idx[3] = {idxb[0].p, idxb[1].p, idxb[2].p};
    int* tmp = idxb[3].p;
    static_assert(sizeof(Box) == 24, "Box is BBMax xyz, BBMin xyz");
    for (int d = 0; d < 3; d++)
        TT_BH(hipMemcpyAsync(idx[d], presorted + (size_t)d * n, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
    TT_BH(hipMemcpyAsync(R.starts, hmesh.data(), hmesh.size() * sizeof(int), hipMemcpyHostToDevice, st));
    TT_BH(hipMemsetAsync(box_p, 0, n2 * sizeof(Box), st));  // NativeArrayOptions.ClearMemory
    TT_BH(hipMemsetAsync(nleft_p, 0, n2 * sizeof(int), st));
    TT_BH(hipMemsetAsync(ncount_p, 0, n2 * sizeof(uint32_t), st));
    TT_BH(hipMemsetAsync(err.p, 0, sizeof(int), st));
    TT_BH(hipMemsetAsync(R.mesh_err, 0, 2 * (size_t)M * sizeof(int), st));  // the error flags and the depths
    if (!roots.empty())
        TT_BH(hipMemcpyAsync(segs.p, roots.data(), roots.size() * sizeof(Seg), hipMemcpyHostToDevice, st));
    // every position in its mesh's root segment: adjacent meshes never share a scan key
    hipLaunchKernelGGL(k_seg_of_mesh, dim3(grid_of(n)), dim3(kBlock), 0, st, n, F, seg_id, seg.p);

    // rocPRIM temporary storage: the largest of the scans used per level (sizes depend on n only)
    auto cnt = rocprim::make_counting_iterator<int>(0);
    size_t tb = 0;
    {
        size_t t1 = 0;
        auto fwd = rocprim::make_transform_iterator(cnt, FwdBox{idx[0], prims_p, seg.p});
        TT_BH(rocprim::inclusive_scan_by_key(nullptr, t1, seg.p, fwd, pre.p, (size_t)n, ExtendOp(),
                                             rocprim::equal_to<int>(), st));
        tb = std::max(tb, t1);
        auto rk = rocprim::make_transform_iterator(cnt, RevKey{seg.p, n});
        auto rb = rocprim::make_transform_iterator(cnt, RevBox{idx[0], prims_p, seg.p, n});
        TT_BH(rocprim::inclusive_scan_by_key(nullptr, t1, rk, rb, sufr.p, (size_t)n, ExtendOp(),
                                             rocprim::equal_to<int>(), st));
        tb = std::max(tb, t1);
        auto fl = rocprim::make_transform_iterator(cnt, LeftFlag{idx[0], seg.p, dimv.p, going_left.p, 0});
        TT_BH(rocprim::exclusive_scan_by_key(nullptr, t1, seg.p, fl, lrank.p, 0, (size_t)n, rocprim::plus<int>(),
                                             rocprim::equal_to<int>(), st));
        tb = std::max(tb, t1);
        auto nc = rocprim::make_transform_iterator(cnt, NextCount{so.p, 1});
        TT_BH(rocprim::exclusive_scan(nullptr, t1, nc, base.p, 0, smax + 1, rocprim::plus<int>(), st));
        tb = std::max(tb, t1);
        auto rb0 = rocprim::make_transform_iterator(cnt, RootBox{prims_p});
        TT_BH(rocprim::inclusive_scan_by_key(nullptr, t1, seg.p, rb0, pre.p, (size_t)n, ExtendOp(),
                                             rocprim::equal_to<int>(), st));
        tb = std::max(tb, t1);
    }
    DBuf<unsigned char> tstore;
    TT_BH(tstore.alloc(tb));
    // root boxes: Extend over a mesh's primitives in index order (BVH2Builder.cs: BVH2Nodes[0].aabb). Extend keeps
    // the earlier value on ties, so the union is an order-preserving scan with Extend itself, keyed by the mesh's
    // root segment; the last element of a mesh's slice is its root.
    {
        size_t t = tb;
        auto rb0 = rocprim::make_transform_iterator(cnt, RootBox{prims_p});
        TT_BH(rocprim::inclusive_scan_by_key(tstore.p, t, seg.p, rb0, pre.p, (size_t)n, ExtendOp(),
                                             rocprim::equal_to<int>(), st));
        hipLaunchKernelGGL(k_mesh_roots, dim3(grid_of(M)), dim3(kBlock), 0, st, F, prims_p, pre.p, box_p, nleft_p, ncount_p);
    }

    int S = (int)roots.size(), bad = 0;
    while (S > 0) {
        depth++;  // the children created at this level sit one deeper (BuildRecursive's depth + 1)
        TT_BH(hipMemsetAsync(best.p, 0xff, 3 * (size_t)S * sizeof(unsigned long long), st));
        for (int d = 0; d < 3; d++) {
            size_t t = tb;
            auto fwd = rocprim::make_transform_iterator(cnt, FwdBox{idx[d], prims_p, seg.p});
            TT_BH(rocprim::inclusive_scan_by_key(tstore.p, t, seg.p, fwd, pre.p, (size_t)n, ExtendOp(),
                                                 rocprim::equal_to<int>(), st));
            t = tb;
            auto rk = rocprim::make_transform_iterator(cnt, RevKey{seg.p, n});
            auto rb = rocprim::make_transform_iterator(cnt, RevBox{idx[d], prims_p, seg.p, n});
            TT_BH(rocprim::inclusive_scan_by_key(tstore.p, t, rk, rb, sufr.p, (size_t)n, ExtendOp(),
                                                 rocprim::equal_to<int>(), st));
            hipLaunchKernelGGL(k_cost, dim3(grid_of(n)), dim3(kBlock), 0, st, n, seg.p, segs.p, pre.p, sufr.p,
                               best.p + (size_t)d * S);
            hipLaunchKernelGGL(k_candidate, dim3(grid_of(S)), dim3(kBlock), 0, st, S, n, segs.p, best.p + (size_t)d * S,
                               pre.p, sufr.p, c_cost.p + (size_t)d * S, c_pos.p + (size_t)d * S,
                               c_left.p + (size_t)d * S, c_right.p + (size_t)d * S);
        }
        hipLaunchKernelGGL(k_split, dim3(grid_of(S)), dim3(kBlock), 0, st, S, segs.p, c_cost.p, c_pos.p, c_left.p,
                           c_right.p, so.p, box_p, nleft_p, ncount_p, err.p, F, depth, mesh_depth, R.mesh_err);
        size_t t = tb;
        auto nc = rocprim::make_transform_iterator(cnt, NextCount{so.p, S});
        TT_BH(rocprim::exclusive_scan(tstore.p, t, nc, base.p, 0, (size_t)S + 1, rocprim::plus<int>(), st));
        int h[2] = {0, 0};
        TT_BH(hipMemcpyAsync(&h[0], base.p + S, sizeof(int), hipMemcpyDeviceToHost, st));
        TT_BH(hipMemcpyAsync(&h[1], err.p, sizeof(int), hipMemcpyDeviceToHost, st));
        TT_BH(hipStreamSynchronize(st));
        bad |= h[1];
        if (bad && M == 1) break;  // (a forest goes on: the other meshes' flags are the caller's to learn)
        hipLaunchKernelGGL(k_children, dim3(grid_of(S)), dim3(kBlock), 0, st, S, segs.p, so.p, base.p, next.p,
                           child_id.p);
        hipLaunchKernelGGL(k_dim_of, dim3(grid_of(S)), dim3(kBlock), 0, st, S, so.p, dimv.p);
        hipLaunchKernelGGL(k_flags, dim3(grid_of(n)), dim3(kBlock), 0, st, n, idx[0], idx[1], idx[2], seg.p, so.p,
                           going_left.p);
        for (int d = 0; d < 3; d++) {
            size_t t2 = tb;
            auto fl = rocprim::make_transform_iterator(cnt, LeftFlag{idx[d], seg.p, dimv.p, going_left.p, d});
            TT_BH(rocprim::exclusive_scan_by_key(tstore.p, t2, seg.p, fl, lrank.p, 0, (size_t)n, rocprim::plus<int>(),
                                                 rocprim::equal_to<int>(), st));
            hipLaunchKernelGGL(k_scatter, dim3(grid_of(n)), dim3(kBlock), 0, st, n, d, idx[d], seg.p, segs.p, so.p,
                               going_left.p, lrank.p, tmp);
            std::swap(idx[d], tmp);
        }
        hipLaunchKernelGGL(k_reseg, dim3(grid_of(n)), dim3(kBlock), 0, st, n, seg.p, so.p, child_id.p);
        TT_BH(hipGetLastError());
        std::swap(segs.p, next.p);
        S = h[0];
    }
    if (bad)  // the C# misbehaves too
        return report_meshes(st, R.mesh_err, M, TT_ERR_UNSUPPORTED, "BVH2 stage: a node has no finite SAH split", mesh_status);
    R.depth.assign((size_t)M, 0u);
    TT_BH(hipMemcpyAsync(R.final_idx.p, idx[0], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
    TT_BH(hipMemcpyAsync(R.depth.data(), mesh_depth, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, st));
    TT_BH(hipStreamSynchronize(st));
    return TT_OK;
}

static tt_status check_inputs(tt_ctx* ctx, const float* aabbs, uint32_t n, const int32_t* presorted) {
    if (!ctx || !aabbs || !n || !presorted || n >= (1u << 30)) return TT_ERR_INVALID_ARG;
    for (size_t i = 0; i < 3 * (size_t)n; i++)
        if (presorted[i] < 0 || (uint32_t)presorted[i] >= n) return TT_ERR_INVALID_ARG;
    return TT_OK;
}

// The exported forms take host arrays: copied to the device here, the results copied back below.
struct DevInputs {
    DBuf<Box> prims;
    DBuf<int> pre;
};
static tt_status upload_inputs(hipStream_t st, const float* aabbs, uint32_t n, const int32_t* presorted, DevInputs& D) {
    static_assert(sizeof(Box) == 24, "Box is BBMax xyz, BBMin xyz");
    TT_BH(D.prims.alloc(n));
    TT_BH(hipMemcpyAsync(D.prims.p, aabbs, (size_t)n * sizeof(Box), hipMemcpyHostToDevice, st));
    if (presorted) {
        TT_BH(D.pre.alloc(3 * (size_t)n));
        TT_BH(hipMemcpyAsync(D.pre.p, presorted, 3 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    }
    return TT_OK;
}

extern "C" tt_status tt_bvh2_build_device(tt_ctx* ctx, const float* aabbs, uint32_t n, const int32_t* presorted,
                                          int32_t* final_indices, float* node_aabbs, int32_t* node_left,
                                          uint32_t* node_count, uint32_t* max_depth) {
    tt_status s = check_inputs(ctx, aabbs, n, presorted);
    if (s != TT_OK || !final_indices) return s != TT_OK ? s : TT_ERR_INVALID_ARG;
    TT_BH(hipSetDevice(ctx->device));  // allocations and launches on the context's GPU
    hipStream_t st = ctx->stream;
    DevInputs D;
    Bvh2Dev R;
    const uint32_t start[2] = {0u, n};
    if ((s = upload_inputs(st, aabbs, n, presorted, D)) != TT_OK ||
        (s = bvh2_stage(st, D.prims.p, start, 1, D.pre.p, R, nullptr)) != TT_OK) {
        ctx->err = g_err;
        return s;
    }
    const size_t n2 = 2 * (size_t)n;
    TT_BH(hipMemcpyAsync(final_indices, R.final_idx.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (node_aabbs) TT_BH(hipMemcpyAsync(node_aabbs, R.box.p, n2 * sizeof(Box), hipMemcpyDeviceToHost, st));
    if (node_left) TT_BH(hipMemcpyAsync(node_left, R.left.p, n2 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (node_count) TT_BH(hipMemcpyAsync(node_count, R.count.p, n2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    TT_BH(hipStreamSynchronize(st));
    if (max_depth) *max_depth = R.depth[0];
    return TT_OK;
}

static tt_status blas_device(hipStream_t st, const Box* prims, const uint32_t* start, int M, const int32_t* presorted,
                             tt_forest_dev& out, tt_status* mesh_status);

// one mesh: the forest of one
static tt_status blas_device_one(hipStream_t st, const Box* prims, uint32_t n, const int32_t* presorted, tt_blas_dev& out) {
    const uint32_t start[2] = {0u, n};
    tt_forest_dev F;
    const tt_status s = blas_device(st, prims, start, 1, presorted, F, nullptr);
    if (s != TT_OK) return s;
    out.nodes = std::move(F.nodes);
    out.cwbvh_indices = std::move(F.cwbvh_indices);
    out.n_nodes = F.node_base[1];
    out.bvh2_depth = F.bvh2_depth[0];
    std::memcpy(out.root_box, F.root_box.data(), sizeof(out.root_box));
    return TT_OK;
}

static tt_status blas_host_io(tt_ctx* ctx, const float* aabbs, uint32_t n, const int32_t* presorted, tt_cwbvh_node* nodes,
                              uint32_t max_nodes, uint32_t* n_nodes, int32_t* cwbvh_indices, uint32_t* bvh2_depth) {
    tt_status s = check_inputs(ctx, aabbs, n, presorted);
    if (s != TT_OK) return s;
    if (!nodes || !n_nodes || !cwbvh_indices) return TT_ERR_INVALID_ARG;
    TT_BH(hipSetDevice(ctx->device));  // allocations and launches on the context's GPU
    hipStream_t st = ctx->stream;
    DevInputs D;
    tt_blas_dev B;
    if ((s = upload_inputs(st, aabbs, n, presorted, D)) != TT_OK) return s;
    if ((s = blas_device_one(st, D.prims.p, n, D.pre.p, B)) != TT_OK) return s;
    if (B.n_nodes > max_nodes) TT_BFAIL(TT_ERR_INVALID_ARG, "tt_blas_build_device: max_nodes too small");
    TT_BH(hipMemcpyAsync(nodes, B.nodes.p, (size_t)B.n_nodes * sizeof(tt_cwbvh_node), hipMemcpyDeviceToHost, st));
    TT_BH(hipMemcpyAsync(cwbvh_indices, B.cwbvh_indices.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    TT_BH(hipStreamSynchronize(st));
    *n_nodes = B.n_nodes;
    if (bvh2_depth) *bvh2_depth = B.bvh2_depth;
    return TT_OK;
}

extern "C" tt_status tt_blas_build_device(tt_ctx* ctx, const float* aabbs, uint32_t n, const int32_t* presorted,
                                          tt_cwbvh_node* nodes, uint32_t max_nodes, uint32_t* n_nodes,
                                          int32_t* cwbvh_indices, uint32_t* bvh2_depth) {
    g_err[0] = 0;
    const tt_status s = blas_host_io(ctx, aabbs, n, presorted, nodes, max_nodes, n_nodes, cwbvh_indices, bvh2_depth);
    if (s != TT_OK && ctx) ctx->err = g_err[0] ? g_err : "tt_blas_build_device: invalid argument";
    return s;
}

tt_status tt_build_blas_dev(hipStream_t st, const float* aabbs_dev, uint32_t n, const int32_t* presorted_dev,
                            tt_blas_dev& out) {
    g_err[0] = 0;
    return blas_device_one(st, reinterpret_cast<const Box*>(aabbs_dev), n, presorted_dev, out);
}

tt_status tt_build_blas_forest(hipStream_t st, const float* aabbs_dev, const uint32_t* start, uint32_t n_meshes,
                               const int32_t* presorted_dev, tt_forest_dev& out, tt_status* mesh_status) {
    g_err[0] = 0;
    return blas_device(st, reinterpret_cast<const Box*>(aabbs_dev), start, (int)n_meshes, presorted_dev, out, mesh_status);
}

// BVH2 + BVH8 + Aggregate over device-resident boxes and presorted lists of M meshes; the nodes (mesh after mesh,
// each numbered from 0), cwbvh_indices (global) and the root boxes (each BVH2's node 0) stay on the device.
static tt_status blas_device(hipStream_t st, const Box* prims, const uint32_t* start, int M, const int32_t* presorted,
                             tt_forest_dev& out, tt_status* mesh_status) {
    tt_status s;
    Bvh2Dev B;
    if ((s = bvh2_stage(st, prims, start, M, presorted, B, mesh_status)) != TT_OK) return s;
    const uint32_t n = start[M];
    const size_t n2 = 2 * (size_t)n;
    const Forest F{B.starts, M};
    // BVH2 levels, the M roots first (for the bottom-up cost pass)
    DBuf<int> order, cnt1, err;
    TT_BH(order.alloc(n2));
    TT_BH(cnt1.alloc(1));
    TT_BH(err.alloc(1));
    TT_BH(hipMemsetAsync(err.p, 0, sizeof(int), st));
    const int zero = 0;
    std::vector<int> root_slots((size_t)M);
    for (int m = 0; m < M; m++) root_slots[m] = 2 * (int)start[m];
    TT_BH(hipMemcpyAsync(order.p, root_slots.data(), (size_t)M * sizeof(int), hipMemcpyHostToDevice, st));
    std::vector<int> lvl{0, M};
    while (lvl.back() > lvl[lvl.size() - 2]) {
        const int lo = lvl[lvl.size() - 2], hi = lvl.back();
        TT_BH(hipMemcpyAsync(cnt1.p, &zero, sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_bvh2_level, dim3(grid_of(hi - lo)), dim3(kBlock), 0, st, hi - lo, order.p + lo, B.left.p,
                           B.count.p, order.p + hi, cnt1.p, (int)(n2 - (size_t)hi));
        int m = 0;
        TT_BH(hipMemcpyAsync(&m, cnt1.p, sizeof(int), hipMemcpyDeviceToHost, st));
        TT_BH(hipStreamSynchronize(st));
        if ((size_t)hi + (size_t)m > n2) TT_BFAIL(TT_ERR_INVALID_ARG, "BVH2 levels: not a binary tree");
        lvl.push_back(hi + m);
    }
    // cost pass, deepest level first
    DBuf<float> cost;
    DBuf<Dec> dec;
    DBuf<int> nprim, firstpos;
    TT_BH(cost.alloc(n2 * 7));
    TT_BH(dec.alloc(n2 * 7));
    TT_BH(nprim.alloc(n2));
    TT_BH(firstpos.alloc(n2));
    for (size_t L = lvl.size() - 1; L-- > 0;) {
        const int lo = lvl[L], hi = lvl[L + 1];
        if (hi > lo)
            hipLaunchKernelGGL(k_cost8, dim3(grid_of(hi - lo)), dim3(kBlock), 0, st, hi - lo, order.p + lo, B.box.p,
                               B.left.p, B.count.p, cost.p, dec.p, nprim.p, firstpos.p, err.p, F, B.mesh_err);
    }
    // collapse: CWBVH8 levels top down (records appended per level), from the M root records, each numbered
    // within its own mesh
    const size_t cap = std::max<size_t>((size_t)M, (size_t)n);
    DBuf<Rec8> rec;
    DBuf<int> nrec;
    TT_BH(rec.alloc(cap));
    TT_BH(nrec.alloc(1));
    std::vector<Rec8> roots((size_t)M, Rec8{});
    for (int m = 0; m < M; m++) {
        roots[m].bvh2 = root_slots[m];
        roots[m].idx = 0;
        roots[m].C = 1;
        roots[m].Ct = 0;
    }
    TT_BH(hipMemcpyAsync(rec.p, roots.data(), (size_t)M * sizeof(Rec8), hipMemcpyHostToDevice, st));
    TT_BH(hipMemcpyAsync(nrec.p, &M, sizeof(int), hipMemcpyHostToDevice, st));
    std::vector<int> r8{0, M};
    while (r8.back() > r8[r8.size() - 2]) {
        const int lo = r8[r8.size() - 2], hi = r8.back();
        hipLaunchKernelGGL(k_expand8, dim3(grid_of(hi - lo)), dim3(kBlock), 0, st, lo, hi, (int)cap, rec.p, nrec.p, B.box.p,
                           B.left.p, B.count.p, dec.p, nprim.p, err.p, F, B.mesh_err);
        int h[2] = {0, 0};
        TT_BH(hipMemcpyAsync(&h[0], nrec.p, sizeof(int), hipMemcpyDeviceToHost, st));
        TT_BH(hipMemcpyAsync(&h[1], err.p, sizeof(int), hipMemcpyDeviceToHost, st));
        TT_BH(hipStreamSynchronize(st));
        if (h[1])
            return report_meshes(st, B.mesh_err, M, TT_ERR_UNSUPPORTED, "BVH8 stage: BVH8Builder.build fails on this tree",
                                 mesh_status);
        if ((size_t)h[0] > cap) TT_BFAIL(TT_ERR_UNSUPPORTED, "BVH8 stage: more CWBVH8 nodes than BVH2 nodes");
        r8.push_back(h[0]);
    }
    const int total = r8.back();
    for (size_t L = r8.size() - 1; L-- > 0;) {
        const int lo = r8[L], hi = r8[L + 1];
        if (hi > lo) hipLaunchKernelGGL(k_up8, dim3(grid_of(hi - lo)), dim3(kBlock), 0, st, lo, hi, rec.p);
    }
    for (size_t L = 0; L + 1 < r8.size(); L++) {
        const int lo = r8[L], hi = r8[L + 1];
        if (hi > lo) hipLaunchKernelGGL(k_down8, dim3(grid_of(hi - lo)), dim3(kBlock), 0, st, lo, hi, rec.p);
    }
    // every root knows its node total now: the meshes' node bases are their exclusive scan
    // (one allocation, read back in one copy: the bases, then the root boxes)
    static_assert(sizeof(Box) == 6 * sizeof(int), "a root box is {BBMax, BBMin}");
    DBuf<int> totals;
    TT_BH(totals.alloc(7 * (size_t)M + 1));
    int* const node_base = totals.p;
    Box* const root_box = reinterpret_cast<Box*>(node_base + M + 1);
    hipLaunchKernelGGL(k_mesh_totals, dim3(1), dim3(kBlock), 0, st, F, rec.p, B.box.p, node_base, root_box);
    TT_BH(out.nodes.alloc((size_t)total));
    TT_BH(out.cwbvh_indices.alloc(n));
    TT_BH(hipMemsetAsync(out.nodes.p, 0, (size_t)total * sizeof(tt_cwbvh_node), st));
    TT_BH(hipMemsetAsync(out.cwbvh_indices.p, 0, (size_t)n * sizeof(int), st));
    hipLaunchKernelGGL(k_fill8, dim3(grid_of(total)), dim3(kBlock), 0, st, total, rec.p, B.box.p, dec.p, nprim.p,
                       firstpos.p, B.final_idx.p, out.nodes.p, out.cwbvh_indices.p, err.p, F, node_base, B.mesh_err);
    TT_BH(hipGetLastError());
    int e = 0;
    std::vector<uint32_t> back(7 * (size_t)M + 1);  // the bases, then the root boxes
    TT_BH(hipMemcpyAsync(&e, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    TT_BH(hipMemcpyAsync(back.data(), node_base, back.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    TT_BH(hipStreamSynchronize(st));
    out.node_base.assign(back.begin(), back.begin() + M + 1);
    out.root_box.resize(6 * (size_t)M);
    std::memcpy(out.root_box.data(), back.data() + M + 1, 6 * (size_t)M * sizeof(float));
    if (e)
        return report_meshes(st, B.mesh_err, M, TT_ERR_UNSUPPORTED,
                             "BVH8 stage: a node's quantization exponent is not a power of two", mesh_status);
    if (out.node_base[M] != (uint32_t)total) TT_BFAIL(TT_ERR_UNSUPPORTED, "BVH8 stage: the meshes' node totals do not add up");
    out.bvh2_depth = B.depth;
    return TT_OK;
}

// The three presorts of BVH2Builder on the GPU, for every mesh of a forest that `sorted` marks (nullable: all).
// TT_ERR_UNSUPPORTED (the caller sorts those meshes on the host, tt_bvh2_presort) when a key is not finite or a
// depth-exhausted partition is too large for the one-thread heapsort; both per mesh.
// prims (n boxes) and presorted (3 x n, axis-major over n, global indices; the output) are device arrays.
static tt_status presort_device(hipStream_t st, const Box* prims_p, const uint32_t* start, int M,
                                const unsigned char* sorted, int32_t* presorted, tt_status* mesh_status) {
    const int n = (int)start[M];
    const int n3 = 3 * n;
    DBuf<float> cent;
    int* const it_p = presorted;  // sorted in place
    DBuf<int> part, gerank, lerank, alist, blist, pk, cnt, err, per_mesh;
    DBuf<SortPart> parts, next, small;
    DBuf<int2> res, child;
    DBuf<unsigned char> sorted_dev;
    const size_t pmax = (size_t)n3 / 17 + 4;  // live partitions per level (> 16 elements each)
    TT_BH(cent.alloc(n3));
    TT_BH(part.alloc(n3));
    TT_BH(gerank.alloc(n3));
    TT_BH(lerank.alloc(n3));
    TT_BH(alist.alloc(n3));
    TT_BH(blist.alloc(n3));
    TT_BH(pk.alloc(pmax));
    TT_BH(parts.alloc(pmax));
    TT_BH(next.alloc(pmax));
    TT_BH(res.alloc(pmax));
    TT_BH(child.alloc(pmax));
    TT_BH(cnt.alloc(1));
    TT_BH(err.alloc(1));
    TT_BH(per_mesh.alloc(5 * (size_t)M + 1));  // one allocation: starts, the root partitions' ids, the error flags
    int* const starts = per_mesh.p;
    int* const root_id = starts + M + 1;
    int* const mesh_err = root_id + 3 * (size_t)M;
    // Sort(length): IntroSort(0, length - 1, 2 * FloorLog2(length)), FloorLog2 = bit length; per mesh and axis. A
    // root of at most 16 elements is the small branch at once, one element needs nothing. (starts and the root
    // partitions' ids: one upload.)
    std::vector<int> hmesh(start, start + M + 1);
    hmesh.resize(4 * (size_t)M + 1, -1);
    int* const hroot = hmesh.data() + M + 1;
    std::vector<SortPart> roots, smalls;
    for (int d = 0; d < 3; d++)
        for (int m = 0; m < M; m++) {
            const int s = hmesh[m], c = hmesh[m + 1] - s;
            if ((sorted && !sorted[m]) || c < 2) continue;
            int fl = 0;
            for (int k = c; k >= 1; k /= 2) fl++;
            const SortPart q{d * n + s, d * n + s + c - 1, 2 * fl};
            if (c <= 16) {
                smalls.push_back(q);
            } else {
                hroot[(size_t)d * M + m] = (int)roots.size();
                roots.push_back(q);
            }
        }
    TT_BH(hipMemcpyAsync(starts, hmesh.data(), hmesh.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (sorted) {
        TT_BH(sorted_dev.alloc(M));
        TT_BH(hipMemcpyAsync(sorted_dev.p, sorted, (size_t)M, hipMemcpyHostToDevice, st));
    }
    const Forest F{starts, M};
    TT_BH(hipMemsetAsync(err.p, 0, sizeof(int), st));
    TT_BH(hipMemsetAsync(mesh_err, 0, (size_t)M * sizeof(int), st));
    hipLaunchKernelGGL(k_centroids, dim3(grid_of(n)), dim3(kBlock), 0, st, n, prims_p, cent.p, it_p, err.p, F,
                       sorted ? sorted_dev.p : nullptr, mesh_err);
    int bad = 0;
    TT_BH(hipMemcpyAsync(&bad, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    TT_BH(hipStreamSynchronize(st));
    if (bad)
        return report_meshes(st, mesh_err, M, TT_ERR_UNSUPPORTED, "presort: non-finite centroid keys (host sort)", mesh_status);
    int P = (int)roots.size();
    if (P) TT_BH(hipMemcpyAsync(parts.p, roots.data(), (size_t)P * sizeof(SortPart), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_part_of_root, dim3(grid_of(n3)), dim3(kBlock), 0, st, n3, n, F, root_id, part.p);
    if (!smalls.empty()) {
        TT_BH(small.alloc(smalls.size()));
        TT_BH(hipMemcpyAsync(small.p, smalls.data(), smalls.size() * sizeof(SortPart), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_small_roots, dim3(grid_of(smalls.size())), dim3(kBlock), 0, st, (int)smalls.size(), small.p, it_p,
                           cent.p, n);
    }
    auto cnt_it = rocprim::make_counting_iterator<int>(0);
    size_t tb = 0, t1 = 0;
    {
        auto ge = rocprim::make_transform_iterator(cnt_it, GeFlag{it_p, part.p, parts.p, pk.p, cent.p, n});
        TT_BH(rocprim::exclusive_scan_by_key(nullptr, t1, part.p, ge, gerank.p, 0, (size_t)n3, rocprim::plus<int>(),
                                             rocprim::equal_to<int>(), st));
        tb = std::max(tb, t1);
        auto le = rocprim::make_transform_iterator(cnt_it, LeFlagRev{it_p, part.p, parts.p, pk.p, cent.p, n, n3});
        auto rk = rocprim::make_transform_iterator(cnt_it, PartKeyRev{part.p, n3});
        TT_BH(rocprim::exclusive_scan_by_key(nullptr, t1, rk, le, lerank.p, 0, (size_t)n3, rocprim::plus<int>(),
                                             rocprim::equal_to<int>(), st));
        tb = std::max(tb, t1);
    }
    DBuf<unsigned char> tstore;
    TT_BH(tstore.alloc(tb));
    int too_large = 0;
    while (P > 0) {
        hipLaunchKernelGGL(k_pivot, dim3(grid_of(P)), dim3(kBlock), 0, st, P, parts.p, it_p, cent.p, n, pk.p);
        size_t t = tb;
        auto ge = rocprim::make_transform_iterator(cnt_it, GeFlag{it_p, part.p, parts.p, pk.p, cent.p, n});
        TT_BH(rocprim::exclusive_scan_by_key(tstore.p, t, part.p, ge, gerank.p, 0, (size_t)n3, rocprim::plus<int>(),
                                             rocprim::equal_to<int>(), st));
        t = tb;
        auto le = rocprim::make_transform_iterator(cnt_it, LeFlagRev{it_p, part.p, parts.p, pk.p, cent.p, n, n3});
        auto rk = rocprim::make_transform_iterator(cnt_it, PartKeyRev{part.p, n3});
        TT_BH(rocprim::exclusive_scan_by_key(tstore.p, t, rk, le, lerank.p, 0, (size_t)n3, rocprim::plus<int>(),
                                             rocprim::equal_to<int>(), st));
        hipLaunchKernelGGL(k_stops, dim3(grid_of(n3)), dim3(kBlock), 0, st, n3, part.p, parts.p, it_p, pk.p, cent.p, n,
                           gerank.p, lerank.p, alist.p, blist.p);
        hipLaunchKernelGGL(k_crossing, dim3(grid_of(P)), dim3(kBlock), 0, st, P, parts.p, gerank.p, lerank.p, alist.p,
                           blist.p, n3, res.p);
        hipLaunchKernelGGL(k_pswap, dim3(grid_of(n3)), dim3(kBlock), 0, st, n3, part.p, parts.p, res.p, alist.p, blist.p,
                           it_p);
        TT_BH(hipMemsetAsync(cnt.p, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_children_sort, dim3(grid_of(P)), dim3(kBlock), 0, st, P, parts.p, res.p, it_p, cent.p, n,
                           next.p, cnt.p, child.p, err.p, F, mesh_err);
        hipLaunchKernelGGL(k_repart, dim3(grid_of(n3)), dim3(kBlock), 0, st, n3, part.p, res.p, child.p);
        TT_BH(hipGetLastError());
        int h[2] = {0, 0};
        TT_BH(hipMemcpyAsync(&h[0], cnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
        TT_BH(hipMemcpyAsync(&h[1], err.p, sizeof(int), hipMemcpyDeviceToHost, st));
        TT_BH(hipStreamSynchronize(st));
        too_large |= h[1];
        if (too_large && M == 1) break;  // (a forest goes on: the partition stays unsorted, the other meshes finish)
        if ((size_t)h[0] > pmax) TT_BFAIL(TT_ERR_UNSUPPORTED, "presort: too many partitions");
        std::swap(parts.p, next.p);
        P = h[0];
    }
    if (too_large)
        return report_meshes(st, mesh_err, M, TT_ERR_UNSUPPORTED,
                             "presort: a depth-exhausted partition is too large (host sort)", mesh_status);
    return TT_OK;
}

tt_status tt_build_presort_forest(hipStream_t st, const float* aabbs_dev, const uint32_t* start, uint32_t n_meshes,
                                  const unsigned char* sorted, int32_t* presorted_dev, tt_status* mesh_status) {
    g_err[0] = 0;
    if (!n_meshes || start[n_meshes] >= (1u << 29)) TT_BFAIL(TT_ERR_INVALID_ARG, "presort: too many primitives");
    return presort_device(st, reinterpret_cast<const Box*>(aabbs_dev), start, (int)n_meshes, sorted, presorted_dev, mesh_status);
}

// one mesh: the forest of one, which leaves n <= 16 to the host as it always has
tt_status tt_build_presort_dev(hipStream_t st, const float* aabbs_dev, uint32_t n, int32_t* presorted_dev) {
    g_err[0] = 0;
    if (n >= (1u << 29)) TT_BFAIL(TT_ERR_INVALID_ARG, "presort: too many primitives");
    if (n <= 16) TT_BFAIL(TT_ERR_UNSUPPORTED, "presort: tiny inputs are sorted on the host");
    const uint32_t start[2] = {0u, n};
    return presort_device(st, reinterpret_cast<const Box*>(aabbs_dev), start, 1, nullptr, presorted_dev, nullptr);
}

extern "C" tt_status tt_bvh2_presort_device(tt_ctx* ctx, const float* aabbs, uint32_t n, int32_t* presorted) {
    if (!ctx || !aabbs || !n || !presorted || n >= (1u << 29)) return TT_ERR_INVALID_ARG;
    g_err[0] = 0;
    if (hipSetDevice(ctx->device) != hipSuccess) {  // allocations and launches on the context's GPU
        ctx->err = "tt_bvh2_presort_device: hipSetDevice failed";
        return TT_ERR_HIP;
    }
    auto run = [&]() -> tt_status {
        hipStream_t st = ctx->stream;
        DevInputs D;
        tt_status s = upload_inputs(st, aabbs, n, nullptr, D);
        if (s != TT_OK) return s;
        TT_BH(D.pre.alloc(3 * (size_t)n));
        if ((s = tt_build_presort_dev(st, reinterpret_cast<const float*>(D.prims.p), n, D.pre.p)) != TT_OK) return s;
        TT_BH(hipMemcpyAsync(presorted, D.pre.p, 3 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
        TT_BH(hipStreamSynchronize(st));
        return TT_OK;
    };
    const tt_status s = run();
    if (s != TT_OK) ctx->err = g_err[0] ? g_err : "tt_bvh2_presort_device failed";
    return s;
}
