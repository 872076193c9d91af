// Stand-alone run of the enqueue's terrain reference (tt_terrain_bounce_host, host/tt_terrain.cpp), built with
// -fsanitize=address,undefined by tests/test_terrain_bounce_host.py: rays onto a flat terrain (normal (0, -1, 0),
// flipped for the rays from above), in both bounce halves and through the batched PixelIndex decode, with
// triangle records, misses and a malformed terrain record among them. Exits 0 when every property holds and the
// sanitizers stay silent.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/truetrace_scene.h"

namespace {

const float kFar = 1000.0f;

tt_ray_data make_ray(float ox, float oy, float oz, float dx, float dy, float dz, uint32_t pix, uint32_t mesh, uint32_t tri,
                     float t) {
    tt_ray_data r;
    std::memset(&r, 0, sizeof(r));
    const float k = 1.0f / std::sqrt(dx * dx + dy * dy + dz * dz);
    r.origin[0] = ox, r.origin[1] = oy, r.origin[2] = oz;
    r.direction[0] = dx * k, r.direction[1] = dy * k, r.direction[2] = dz * k;
    r.PixelIndex = pix;
    r.hits[0] = mesh;
    r.hits[1] = tri;
    std::memcpy(&r.hits[2], &t, 4);
    r.hits[3] = 0x12345678u;
    return r;
}

}  // namespace

int main() {
    std::vector<uint16_t> map(8 * 8, (uint16_t)0x3400u);  // 0.25
    tt_terrain terrain;
    std::memset(&terrain, 0, sizeof(terrain));
    terrain.HeightScale = 4.0f;
    terrain.TerrainDim[0] = terrain.TerrainDim[1] = 32.0f;
    terrain.HeightMap[0] = terrain.HeightMap[1] = 1.0f;
    const uint32_t w = 16, h = 16, wh = w * h, n = 200;
    uint32_t seed = 777u;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)(seed >> 8) / 16777216.0f;
    };
    int bad = 0;
    for (int bounce = 0; bounce < 2; bounce++)
        for (uint32_t frame_pixels = 0; frame_pixels <= wh; frame_pixels += wh) {
            std::vector<tt_ray_data> rays(2 * wh);
            const uint32_t off = bounce ? wh : 0u;
            for (uint32_t i = 0; i < n; i++) {
                const bool up = i % 4u == 1u;  // from below: the normal is not flipped
                const float oy = up ? -6.0f : 8.0f + 10.0f * rnd();
                const float ox = 2.0f + 28.0f * rnd(), oz = 2.0f + 28.0f * rnd();
                const float tx = 2.0f + 28.0f * rnd(), tz = 2.0f + 28.0f * rnd();
                const float len = std::sqrt((tx - ox) * (tx - ox) + (2.01f - oy) * (2.01f - oy) + (tz - oz) * (tz - oz));
                uint32_t mesh = TT_TERRAIN_MESH_ID, tri = 0;
                float t = len;
                if (i % 10u == 3u) mesh = 0u, tri = 5u;      // a triangle record
                if (i % 10u == 7u) mesh = 0u, t = kFar;      // a miss
                if (i == 50u) tri = 1u;                      // triangle_id >= n_terrains
                rays[off + i] = make_ray(ox, oy, oz, tx - ox, 2.01f - oy, tz - oz, i + (frame_pixels ? (i & 1u) * wh : 0u), mesh,
                                         tri, t);
            }
            tt_trace_params p;
            std::memset(&p, 0, sizeof(p));
            p.n_rays = n;
            p.bounce = bounce;
            p.far_plane = kFar;
            p.screen_width = w;
            p.screen_height = frame_pixels ? 2 * h : h;
            std::vector<tt_ray_data> out(n);
            std::vector<int32_t> sv(n, 99);
            std::memset(out.data(), 0xEE, n * sizeof(tt_ray_data));
            const uint32_t hw = frame_pixels ? 2 * wh : wh;
            if (hw > wh) rays.resize(2 * hw);  // (the window of an odd bounce starts at W * H of the taller screen)
            if (bounce && frame_pixels) {
                for (uint32_t i = 0; i < n; i++) rays[hw + i] = rays[wh + i];
            }
            if (tt_terrain_bounce_host(&terrain, 1, map.data(), 8, 8, &p, rays.data(), 3, 4, frame_pixels, out.data(),
                                       sv.data()) != TT_OK)
                return 2;
            const uint32_t base = bounce ? hw : 0u;
            uint32_t live = 0;
            for (uint32_t i = 0; i < n; i++) {
                const tt_ray_data& R = rays[base + i];
                const bool terrain_rec = R.hits[0] == TT_TERRAIN_MESH_ID;
                if (!terrain_rec) {
                    const unsigned char* b = reinterpret_cast<const unsigned char*>(&out[i]);
                    if (sv[i] != -1 || b[0] != 0xEE || b[47] != 0xEE) bad++, std::printf("ray %u: not a terrain record\n", i);
                    continue;
                }
                if (i == 50u) {
                    if (sv[i] != 0) bad++, std::printf("ray 50: malformed record survived\n");
                    continue;
                }
                if (sv[i] != 0 && sv[i] != 1) bad++, std::printf("ray %u: survives %d\n", i, sv[i]);
                if (sv[i] != 1) continue;
                live++;
                const tt_ray_data& O = out[i];
                float t;
                std::memcpy(&t, &R.hits[2], 4);
                const float len = std::sqrt(O.direction[0] * O.direction[0] + O.direction[1] * O.direction[1] +
                                            O.direction[2] * O.direction[2]);
                const float py = R.direction[1] * t + R.origin[1];
                const float ny = R.direction[1] > 0.0f ? -1.0f : 1.0f;  // (0, -1, 0), flipped for rays from above
                if (std::fabs(len - 1.0f) > 1e-6f || O.origin[1] != ny * 0.0001f + py || O.PixelIndex != R.PixelIndex ||
                    std::memcmp(O.hits, R.hits, 16) != 0 || !(O.last_pdf > 0.0f) ||
                    std::fabs(O.direction[1] * ny - O.last_pdf * 3.14159265f) > 1e-4f) {
                    std::printf("ray %u: len %.8f origin.y %.8f (pos.y %.8f) pdf %.8f dir.y %.8f\n", i, len, O.origin[1], py,
                                O.last_pdf, O.direction[1]);
                    bad++;
                }
            }
            if (live < n / 2) bad++, std::printf("bounce %d: only %u survivors\n", bounce, live);
        }
    std::printf("terrain bounce KAT: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
