#pragma once
#include "tt_device.h"

hipError_t tt_launch_trace(const TraceArgs& a, bool stats, bool matcheck, int info, bool leaf, uint32_t grid,
                           hipStream_t st);
uint32_t tt_trace_chunk_rays();
hipError_t tt_trace_occupancy_table(int* out24);
hipError_t tt_launch_shadow(const ShadowArgs* a, uint32_t grid, hipStream_t st, int stats, int matcheck);
hipError_t tt_launch_shadow_accumulate(const ShadowArgs* a, const float4* vis, hipStream_t st);
void tt_shadow_occupancy_table(int* out4);
uint32_t tt_trace_block_size();
uint32_t tt_trace_spill_entries();
uint32_t tt_trace_lds_bytes(bool leaf);
hipError_t tt_launch_generate(const float* c2w, const float* ip, uint32_t w, uint32_t h, float near_plane, float far_plane,
                              int32_t jitter, int32_t frames, int32_t max_bounce, tt_ray_data* rays, hipStream_t st);
hipError_t tt_launch_bounce(tt_ray_data* rays, uint32_t src_off, uint32_t dst_off, uint32_t n, float far_plane,
                            int32_t cur_bounce, int32_t frames, int32_t max_bounce, const tt_cuda_triangle* tris,
                            const tt_mesh_data* md, uint32_t* counter, hipStream_t st, const uint32_t* n_dev,
                            uint32_t* n_next_dev, uint32_t* ctl_next, uint32_t ctl_next_words,
                            uint32_t frame_pixels, uint32_t terrains, const tt_terrain* ter = nullptr,
                            uint32_t n_ter = 0, const uint16_t* hmap = nullptr, uint32_t hmap_w = 0, uint32_t hmap_h = 0);
uint32_t tt_bounce_tiles(uint32_t n);
hipError_t tt_launch_resolve(const tt_ray_data* rays, uint32_t ray_offset, uint32_t n, float far_plane,
                             const tt_cuda_triangle* tris, uint32_t n_tris, const tt_mesh_data* md, uint32_t n_mesh,
                             float* out, hipStream_t st, const tt_terrain* terrains, uint32_t n_terrains,
                             const uint16_t* hmap, uint32_t hmap_w, uint32_t hmap_h);
hipError_t tt_launch_terrain(const TerrainArgs* a, int shadow, int stats, int grid_form, uint32_t grid, hipStream_t st);
hipError_t tt_launch_terrain_shadow_outputs(const ShadowArgs* a, hipStream_t st);
void tt_terrain_occupancy_table(int* out3);
hipError_t tt_launch_rcp_selftest(unsigned long long* d_bad, hipStream_t st);
