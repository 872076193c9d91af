// tt_object_batch_host.h — the host-only half of tt_objects_build_device (tt_object_build.hip): the argument checks
// of a mesh set, the concatenated triangle ranges, the layout of the one device blob that holds every host mesh's
// arrays and the few copies that fill it, and the per-mesh status of a failed stage. Plain C++ with no HIP in
// it, so a stand-alone program can run it under the host sanitizers (tests/native/object_batch_kat_main.cpp).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/truetrace_hip.h"

namespace tt_batch {

constexpr uint64_t kAbsent = ~0ull;  // a nullable mesh array the mesh does not have
constexpr uint64_t kAlign = 4;       // blob offsets in 4-byte words, every array 16-byte aligned

// Word offsets of one mesh's arrays in the staging blob (all of them 4-byte elements).
struct MeshOffsets {
    uint64_t pos = kAbsent, nrm = kAbsent, tan = kAbsent, uv = kAbsent, idx = kAbsent, mat = kAbsent;
};

struct Plan {
    std::vector<uint32_t> start;   // n_meshes + 1: mesh m owns triangles [start[m], start[m + 1]) of the batch
    std::vector<MeshOffsets> off;  // per mesh (host meshes only; empty for device-pointer meshes)
    uint64_t words = 0;            // the blob's size
};

inline void set_status(tt_status* mesh_status, uint32_t m, tt_status s) {
    if (mesh_status) mesh_status[m] = s;
}

// The checks made before any launch. Every refused mesh is marked in mesh_status (nullable); why names the first.
inline tt_status check_meshes(const tt_mesh_input* meshes, uint32_t n_meshes, const int32_t* const* presorted,
                              tt_status* mesh_status, std::string& why) {
    if (!meshes || n_meshes == 0) {
        why = "argument checks: no meshes";
        return TT_ERR_INVALID_ARG;
    }
    int first = -1;
    auto refuse = [&](uint32_t m, const std::string& reason) {
        set_status(mesh_status, m, TT_ERR_INVALID_ARG);
        if (first < 0) {
            first = (int)m;
            why = "argument checks: mesh " + std::to_string(m) + ": " + reason;
        }
    };
    uint64_t total = 0;
    for (uint32_t m = 0; m < n_meshes; m++) {
        const tt_mesh_input& in = meshes[m];
        if (!in.positions || !in.indices || !in.n_vertices) {
            refuse(m, "null positions or indices");
            continue;
        }
        if (in.n_indices < 3 || in.n_indices % 3) {
            refuse(m, "n_indices (" + std::to_string(in.n_indices) + ") is not a positive multiple of 3");
            continue;
        }
        const uint32_t n = in.n_indices / 3;
        if (n >= (1u << 29) || (uint64_t)n * 48u >= (1ull << 32)) {
            refuse(m, "triangle array of 4 GiB or more (the trace kernel addresses it with 32-bit offsets)");
            continue;
        }
        total += n;
        const int32_t* pre = presorted ? presorted[m] : nullptr;
        if (pre)
            for (size_t i = 0; i < 3 * (size_t)n; i++)
                if (pre[i] < 0 || (uint32_t)pre[i] >= n) {
                    refuse(m, "presorted[" + std::to_string(i) + "] out of range");
                    break;
                }
    }
    if (first >= 0) return TT_ERR_INVALID_ARG;
    if (total >= (1ull << 29)) {
        why = "argument checks: " + std::to_string(total) + " triangles in one call (the limit is 2^29 - 1)";
        return TT_ERR_INVALID_ARG;
    }
    return TT_OK;
}

// The triangle ranges, and (stage: the meshes are host arrays) where each array goes in the blob.
inline void make_plan(const tt_mesh_input* meshes, uint32_t n_meshes, bool stage, Plan& p) {
    p.start.assign((size_t)n_meshes + 1, 0u);
    p.off.clear();
    p.words = 0;
    for (uint32_t m = 0; m < n_meshes; m++) p.start[m + 1] = p.start[m] + meshes[m].n_indices / 3;
    if (!stage) return;
    p.off.resize(n_meshes);
    auto place = [&](const void* src, uint64_t count) -> uint64_t {
        if (!src) return kAbsent;
        const uint64_t at = p.words;
        p.words += (count + kAlign - 1) / kAlign * kAlign;
        return at;
    };
    for (uint32_t m = 0; m < n_meshes; m++) {
        const tt_mesh_input& in = meshes[m];
        const uint64_t nv = in.n_vertices, n = in.n_indices / 3;
        MeshOffsets& o = p.off[m];
        o.pos = place(in.positions, 3 * nv);
        o.nrm = place(in.normals, 3 * nv);
        o.tan = place(in.tangents, 4 * nv);
        o.uv = place(in.uvs, 2 * nv);
        o.idx = place(in.indices, 3 * n);
        o.mat = place(in.matdat, n);
    }
}

// Copies one host mesh's arrays to their places in blob (p.words words). The alignment gaps are zeroed.
inline void fill_mesh(const tt_mesh_input& in, const MeshOffsets& o, uint32_t* blob) {
    auto put = [&](uint64_t at, const void* src, uint64_t count) {
        if (at == kAbsent) return;
        std::memcpy(blob + at, src, count * 4);
        const uint64_t end = (count + kAlign - 1) / kAlign * kAlign;
        for (uint64_t k = count; k < end; k++) blob[at + k] = 0u;
    };
    const uint64_t nv = in.n_vertices, n = in.n_indices / 3;
    put(o.pos, in.positions, 3 * nv);
    put(o.nrm, in.normals, 3 * nv);
    put(o.tan, in.tangents, 4 * nv);
    put(o.uv, in.uvs, 2 * nv);
    put(o.idx, in.indices, 3 * n);
    put(o.mat, in.matdat, n);
}
inline void fill_blob(const tt_mesh_input* meshes, uint32_t n_meshes, const Plan& p, uint32_t* blob) {
    for (uint32_t m = 0; m < n_meshes; m++) fill_mesh(meshes[m], p.off[m], blob);
}

// One host-to-device copy of the staging: `words` words from src to word `at` of the device blob.
struct Copy {
    uint64_t at, words;
    const void* src;
};
// The copies that fill the device blob, as few as is practical. A mesh of direct_words words or more goes array by
// array straight from the caller's memory: composing it would cost one more pass over memory and save at most five
// copies. The smaller meshes are composed in `staging` (p.words words; only their parts are touched) and every run
// of consecutive small meshes travels as one copy.
inline void stage_copies(const tt_mesh_input* meshes, uint32_t n_meshes, const Plan& p, uint64_t direct_words,
                         uint32_t* staging, std::vector<Copy>& out) {
    auto begin = [&](uint32_t m) { return m < n_meshes ? p.off[m].pos : p.words; };  // positions come first, always
    uint64_t run = kAbsent;
    for (uint32_t m = 0; m < n_meshes; m++) {
        const uint64_t b = begin(m), e = begin(m + 1);
        if (e - b < direct_words) {
            fill_mesh(meshes[m], p.off[m], staging);
            if (run == kAbsent) run = b;
            continue;
        }
        if (run != kAbsent) out.push_back(Copy{run, b - run, staging + run});
        run = kAbsent;
        const tt_mesh_input& in = meshes[m];
        const MeshOffsets& o = p.off[m];
        const uint64_t nv = in.n_vertices, n = in.n_indices / 3;
        const Copy direct[6] = {{o.pos, 3 * nv, in.positions}, {o.nrm, 3 * nv, in.normals}, {o.tan, 4 * nv, in.tangents},
                                {o.uv, 2 * nv, in.uvs},        {o.idx, 3 * n, in.indices},  {o.mat, n, in.matdat}};
        for (const Copy& c : direct)
            if (c.at != kAbsent) out.push_back(c);
    }
    if (run != kAbsent) out.push_back(Copy{run, p.words - run, staging + run});
}

// A caller's presort list of mesh m, as the forest takes it: the mesh's start added to every index. out: 3 x n.
inline void globalize_presort(const int32_t* list, uint32_t n, uint32_t start, int32_t* out) {
    for (size_t i = 0; i < 3 * (size_t)n; i++) out[i] = list[i] + (int32_t)start;
}

// A stage's per-mesh flags (non-zero: the mesh failed) into mesh_status; returns the lowest failing mesh, -1: none.
inline int mark_failed(const int* flags, uint32_t n_meshes, tt_status code, tt_status* mesh_status) {
    int first = -1;
    for (uint32_t m = 0; m < n_meshes; m++) {
        if (!flags[m]) continue;
        if (first < 0) first = (int)m;
        set_status(mesh_status, m, code);
    }
    return first;
}

}  // namespace tt_batch
