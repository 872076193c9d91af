// tt_assemble.h — device side of the GPU-resident objects (tt_object_*, tt_scene_assemble_objects): the
// segment table of the batched gather and the launchers of csrc/tt_assemble.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tt_device.h"

// One contiguous byte range an assembly copies: an object's nodes, its 88-byte triangles or its TriPos
// records. Work is counted in 16-byte units (the last unit of a segment may hold 8 bytes); unit_end is the
// inclusive prefix sum over the table, so the units of segment s are [unit_end[s - 1], unit_end[s]).
struct AsmSegment {
    const uint8_t* src;  // 16-byte aligned (the start of an object's own allocation)
    uint8_t* dst;        // 16-byte aligned, or only 8-byte aligned when `wide` is 0
    uint8_t* dst_k;      // node segments of a TT_NODE_STRIDE != 80 build: the strided copy's first slot (else null)
    uint64_t bytes;      // a multiple of 8 (88-byte triangles may exceed 4 GiB where their 48-byte TriPos do not)
    uint64_t unit_end;
    uint32_t wide;       // 1: source and destination are both 16-byte aligned
    uint32_t pad;
};
static_assert(sizeof(AsmSegment) == 48, "AsmSegment layout");

#define TT_ASM_BLOCK 256u
#define TT_ASM_UNITS_PER_THREAD 4u
#define TT_ASM_TILE (TT_ASM_BLOCK * TT_ASM_UNITS_PER_THREAD)  // 16-byte units per tile (16 KiB)

// TriPos records [0, n) from the 88-byte triangles (derive_tri's field mapping, pads zero).
hipError_t tt_launch_derive_tripos(const tt_cuda_triangle* tris, TriPos* out, uint32_t n, hipStream_t st);
// The batched gather over `n_seg` segments (device table `seg`, total_units = its last unit_end).
hipError_t tt_launch_assemble(const AsmSegment* seg, uint32_t n_seg, uint64_t total_units, hipStream_t st);
