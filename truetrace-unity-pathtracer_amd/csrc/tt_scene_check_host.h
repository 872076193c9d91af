// tt_scene_check_host.h — the host-only structural checks that stand in front of every kernel: the one walk over
// CWBVH nodes (the only place that decodes a node's meta bytes), and the whole-scene check built on it
// (tt_scene_upload, tt_scene_validate and the per-frame tt_scene_update_* calls). The TLAS installation
// (tt_tlas_host.h) and the GPU-resident objects (tt_assemble_host.h) walk through the same loop with bounds and
// messages of their own. Plain C++ with no HIP in it, so a stand-alone program can run it under the host
// sanitizers (tests/native/scene_check_kat_main.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/truetrace_hip.h"

namespace tt_check {

enum class Enter { refused, seen, fresh };
// on a policy's hot members: an upload of a 10 M-triangle scene walks every node through them
#define TT_CHECK_INLINE inline __attribute__((always_inline))

// IntersectBVH's index arithmetic (IntersectionKernels.compute:157-213) from `root` down: a LIFO stack, children
// pushed in slot order 0..7, a node handled when first popped. The policy P supplies the bounds, the messages and
// what is recorded (all calls are resolved at compile time: an upload walks every node of the scene):
//   Enter enter(ni)                       a popped index: out of range (refused), met before, or recorded now
//   const tt_cwbvh_node& node(ni)
//   bool child(ni, n, rank, out)          out = the child of `n` with `rank` inner slots before it; false: refused
//   bool leaf(ni, t)                      t = base_tri + low5 + bit, in 64 bits, before any offset; false: refused
//   bool bad_meta(ni, what)               records the refusal of a malformed meta byte, returns false
template <class P>
bool walk(uint32_t root, P& p) {
    std::vector<uint32_t> work{root};
    while (!work.empty()) {
        const uint32_t ni = work.back();
        work.pop_back();
        const Enter e = p.enter(ni);
        if (e == Enter::refused) return false;
        if (e == Enter::seen) continue;
        const tt_cwbvh_node& n = p.node(ni);
        const uint32_t imask = n.e_imask >> 24;
        for (int k = 0; k < 8; k++) {
            const uint32_t meta = (n.meta[k >> 2] >> ((k & 3) * 8)) & 0xffu;
            const uint32_t low5 = meta & 0x1fu, bits = (meta >> 5) & 7u;
            if ((meta & 0x18u) == 0x18u) {
                if (bits != 1u) return p.bad_meta(ni, "inner meta with child bits != 1");
                const uint32_t slot = low5 - 24u;
                uint32_t child;
                if (!p.child(ni, n, (uint32_t)__builtin_popcount(imask & ((1u << slot) - 1u)), child)) return false;
                work.push_back(child);
            } else if (bits) {
                const uint32_t top = low5 + (31u - (uint32_t)__builtin_clz(bits));
                if (top >= 24u) return p.bad_meta(ni, "leaf meta spills into the internal-child bits");
                for (uint32_t b = 0; b < 3; b++)
                    if (((bits >> b) & 1u) && !p.leaf(ni, (uint64_t)n.base_tri + low5 + b)) return false;
            }
        }
    }
    return true;
}

// ---------------------------------------------------------------- the whole-scene check
// What the check reads, exactly as the kernels address it. TLAS-level walks read tl[0, n_tl), BLAS-level walks
// bl[0, n_bl). A scene of its own: both are its node array. An overlay borrower (tt_ctx_share_blas): its TLAS copy
// and the lender's nodes (TLAS at tlas_base, BLASes shared).
struct SceneView {
    const tt_cwbvh_node* tl;
    uint32_t n_tl;
    const tt_cwbvh_node* bl;
    uint32_t n_bl;
    const int32_t* tlas;  // TLASBVH8Indices
    size_t n_tlas;
    const tt_mesh_data* mesh;  // _MeshData
    size_t n_mesh;
    uint32_t n_tris;
};

// A BLAS as a mesh record names it
struct BlasKey {
    uint32_t root, node_offset, tri_offset;
    bool operator<(const BlasKey& o) const {
        return root != o.root ? root < o.root : node_offset != o.node_offset ? node_offset < o.node_offset
                                                                              : tri_offset < o.tri_offset;
    }
    bool operator==(const BlasKey& o) const {
        return root == o.root && node_offset == o.node_offset && tri_offset == o.tri_offset;
    }
};
inline BlasKey key_of(const tt_mesh_data& md) {
    return BlasKey{(uint32_t)(md.mesh_data_bvh_offsets & 0x7fffffff), (uint32_t)md.NodeOffset, (uint32_t)md.TriOffset};
}

// Structural validation of everything the trace kernel can reach: every reachable node, triangle, TLAS slot
// and mesh record must be in range, so the GPU kernel needs no per-access bounds checks.
struct Validator {
    const SceneView s;
    std::string why;
    std::vector<uint32_t> tlas_visit;  // nodes reached by the last TLAS-level walk
    std::vector<uint32_t> blas_visit;  // nodes reached by the BLAS-level walks of this validator
    std::vector<BlasKey> keys;         // sorted: the BLASes walked by run()
    explicit Validator(const SceneView& v) : s(v), epoch_of(std::max(v.n_tl, v.n_bl), 0u) {}

    bool walk_tlas() {
        tlas_visit.clear();
        Level<true> p{*this, 0u, 0u};
        return walk(0u, p);
    }
    bool walk_blas(const BlasKey& k) {
        Level<false> p{*this, k.node_offset, k.tri_offset};
        return walk(k.root, p);
    }
    // one mesh record's BLAS (IntersectionKernels.compute:197-213 reach it through the TLAS)
    bool walk_mesh(const tt_mesh_data& md) {
        if (md.NodeOffset < 0 || md.TriOffset < 0) {
            why = "negative mesh offsets";
            return false;
        }
        return walk_blas(key_of(md));
    }
    bool run() {
        if (s.n_tl == 0 || s.n_bl == 0 || s.n_mesh == 0) {
            why = "empty scene";
            return false;
        }
        if (!walk_tlas()) return false;
        // every mesh record, reachable through the TLAS or not (cheap, and update paths may re-point TLAS
        // leaves); one walk per distinct BLAS
        for (size_t m = 0; m < s.n_mesh; m++) {
            const BlasKey k = key_of(s.mesh[m]);
            // (a record with a walked BLAS's key has that record's offsets: not negative)
            if (std::find(keys.begin(), keys.end(), k) != keys.end()) continue;
            if (!walk_mesh(s.mesh[m])) return false;
            keys.push_back(k);
        }
        std::sort(keys.begin(), keys.end());
        return true;
    }

  private:
    std::vector<uint32_t> epoch_of;  // per node: the walk that met it last
    uint32_t epoch = 0;

    // The scene walk's policy. A child index is base_child + NodeOffset + rank in 32 bits and may wrap, as the
    // kernels' arithmetic does; it is range-checked when popped.
    template <bool tlas_level>
    struct Level {
        Validator& v;
        const uint32_t node_offset, tri_offset;
        const uint32_t walk_id = ++v.epoch;
        TT_CHECK_INLINE Enter enter(uint32_t ni) {
            if (ni >= (tlas_level ? v.s.n_tl : v.s.n_bl)) {
                v.why = "node index " + std::to_string(ni) + " out of range" +
                        (tlas_level && v.s.tl != v.s.bl ? " of the context's own TLAS nodes" : "");
                return Enter::refused;
            }
            if (v.epoch_of[ni] == walk_id) return Enter::seen;
            v.epoch_of[ni] = walk_id;
            (tlas_level ? v.tlas_visit : v.blas_visit).push_back(ni);
            return Enter::fresh;
        }
        TT_CHECK_INLINE const tt_cwbvh_node& node(uint32_t ni) const { return tlas_level ? v.s.tl[ni] : v.s.bl[ni]; }
        TT_CHECK_INLINE bool child(uint32_t, const tt_cwbvh_node& n, uint32_t rank, uint32_t& out) const {
            out = n.base_child + node_offset + rank;
            return true;
        }
        TT_CHECK_INLINE bool leaf(uint32_t, uint64_t t) {
            t += tri_offset;
            if (!tlas_level) return t < v.s.n_tris || refuse("triangle index out of range");
            if (t >= v.s.n_tlas) return refuse("TLAS leaf slot out of range");
            const int32_t m = v.s.tlas[t];
            return (m >= 0 && (size_t)m < v.s.n_mesh) || refuse("TLASBVH8Indices entry out of range");
        }
        bool bad_meta(uint32_t, const char* what) { return refuse(what); }
        bool refuse(const char* what) {
            v.why = what;
            return false;
        }
    };
};

// ---------------------------------------------------------------- what a validation leaves behind
// For the incremental per-frame updates (tt_scene_update_*): what the last full validation established.
struct Bookkeeping {
    std::vector<BlasKey> blas_ok;       // sorted: the BLASes walked and valid
    std::vector<uint8_t> is_tlas_node;  // node reached by the TLAS-level walk
    std::vector<uint32_t> tlas_nodes;   // the same, as a list
    std::vector<uint8_t> is_blas_node;  // node reached by a validated BLAS walk (never TLAS-only updated)
};

// The TLAS reach after a new TLAS-level walk. n_nodes != 0: over a new node array of that length (every flag
// starts clear); 0: over the same array, where only the old reach's flags need clearing.
inline void replace_tlas_reach(std::vector<uint8_t>& is_tlas_node, std::vector<uint32_t>& tlas_nodes,
                               const std::vector<uint32_t>& visit, size_t n_nodes) {
    if (n_nodes) {
        is_tlas_node.assign(n_nodes, 0u);
    } else {
        for (uint32_t n : tlas_nodes)
            if (n < is_tlas_node.size()) is_tlas_node[n] = 0u;
    }
    tlas_nodes = visit;
    for (uint32_t n : tlas_nodes) is_tlas_node[n] = 1u;
}

// Records what a full validation (Validator::run) of a scene of n_nodes nodes established.
inline void remember_validation(Bookkeeping& b, const Validator& v, size_t n_nodes) {
    b.blas_ok = v.keys;
    replace_tlas_reach(b.is_tlas_node, b.tlas_nodes, v.tlas_visit, n_nodes);
    b.is_blas_node.assign(n_nodes, 0u);
    for (uint32_t n : v.blas_visit) b.is_blas_node[n] = 1u;
}

}  // namespace tt_check
