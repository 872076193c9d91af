// Stand-alone known-answer run of the host terrain reference (host/tt_terrain.cpp), built with
// -fsanitize=address,undefined by tests/test_terrain_host.py: the analytic plane rays, the special-ray
// table (the same scene and table as the Python test) and a shadow / normal pass. Exits 0 when every
// answer matches and the sanitizers stay silent.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/truetrace_scene.h"

namespace {

const float kFar = 1000.0f;

uint16_t half_bits(float v) {  // exact for the few constants used here (0.25)
    uint32_t u;
    std::memcpy(&u, &v, 4);
    const uint32_t e = ((u >> 23) & 0xffu) - 112u;
    return (uint16_t)((u >> 16 & 0x8000u) | (e << 10) | ((u >> 13) & 0x3ffu));
}

tt_terrain make_terrain(float px, float hs, float dim) {
    tt_terrain t;
    std::memset(&t, 0, sizeof(t));
    t.PositionOffset[0] = px;
    t.HeightScale = hs;
    t.TerrainDim[0] = t.TerrainDim[1] = dim;
    t.HeightMap[0] = t.HeightMap[1] = 1.0f;
    return t;
}

tt_ray_data make_ray(float ox, float oy, float oz, float dx, float dy, float dz, uint32_t pix, float t = kFar,
                     uint32_t mesh = 0, uint32_t tri = 0) {
    tt_ray_data r;
    std::memset(&r, 0, sizeof(r));
    const float k = 1.0f / std::sqrt(dx * dx + dy * dy + dz * dz);
    r.origin[0] = ox, r.origin[1] = oy, r.origin[2] = oz;
    r.direction[0] = dx * k, r.direction[1] = dy * k, r.direction[2] = dz * k;
    r.PixelIndex = pix;
    r.hits[0] = mesh;
    r.hits[1] = tri;
    std::memcpy(&r.hits[2], &t, 4);
    return r;
}

}  // namespace

int main() {
    // terrain 0: [0, 32]^2, surface y = 0.01 + 2 * 0.25 * 4 = 2.01; terrain 1: x in [40, 56], surface y = 2.21
    std::vector<uint16_t> map(8 * 8, half_bits(0.25f));
    const tt_terrain terrains[2] = {make_terrain(0.0f, 4.0f, 32.0f), make_terrain(40.0f, 4.4f, 16.0f)};
    struct Case {
        tt_ray_data ray;
        int hit, terrain;
    };
    const Case cases[] = {
        {make_ray(10, 25, 10, 0, -1, 0, 0), 1, 0},                // straight down: two zero components
        {make_ray(10, 25, 10, 1, 0, 0, 1), 0, 0},                 // horizontal, high above both
        {make_ray(16, 10, 16, 0.6f, -0.8f, 0, 2), 1, 0},          // starts inside the box, above the surface
        {make_ray(16, 1, 16, 0, 1, 0, 3), 1, 0},                  // starts below the surface, upwards: bisection
        {make_ray(16, 1, 16, 1, 0, 0, 4), 1, 0},                  // starts below the surface, sideways: bisection
        {make_ray(-5, 3, 8, 1, 0, 0, 5), 0, 0},                   // crosses both boxes above the surfaces, leaves
        {make_ray(-5, 3.27f, 8, 1, -0.02f, 0, 6), 1, 1},          // leaves terrain 0 by its far side, hits terrain 1
        {make_ray(10, 25, 10, 0, -1, 0, 7, 5.0f, 0, 7), 0, 0},    // a triangle hit at t = 5 is nearer
        {make_ray(10, 25, 10, 0, -1, 0, 8, 0.01f, 0, 7), 0, 0},   // a triangle hit nearer than the box floor 0.025
        {make_ray(-10, 25, 10, 0, -1, 0, 9), 0, 0},               // beside the footprint
        {make_ray(48, 10, 8, 0, -1, 0, 10), 1, 1},                // straight down onto terrain 1
    };
    const uint32_t n_cases = sizeof(cases) / sizeof(cases[0]);
    std::vector<tt_ray_data> rays;
    for (const Case& c : cases) rays.push_back(c.ray);
    // analytic rays: from above onto terrain 0's footprint
    uint32_t seed = 12345u;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)(seed >> 8) / 16777216.0f;
    };
    const uint32_t n_plane = 200;
    for (uint32_t i = 0; i < n_plane; i++) {
        const float tx = 2.0f + 28.0f * rnd(), tz = 2.0f + 28.0f * rnd();
        const float ox = 2.0f + 28.0f * rnd(), oy = 8.0f + 20.0f * rnd(), oz = 2.0f + 28.0f * rnd();
        rays.push_back(make_ray(ox, oy, oz, tx - ox, 2.01f - oy, tz - oz, n_cases + i));
    }
    const uint32_t n = (uint32_t)rays.size(), w = 16, h = 16;
    std::vector<tt_ray_data> buf(2 * w * h);
    std::vector<uint32_t> info(4 * w * h, 0u), detail(n, 0u);
    for (uint32_t i = 0; i < n; i++) buf[i] = rays[i];
    tt_trace_params p;
    std::memset(&p, 0, sizeof(p));
    p.n_rays = n;
    p.far_plane = kFar;
    p.screen_width = w;
    p.screen_height = h;
    tt_stats st;
    if (tt_terrain_trace_detail_host(terrains, 2, map.data(), 8, 8, &p, buf.data(), info.data(), &st, detail.data()) != TT_OK)
        return 2;
    int bad = 0;
    for (uint32_t i = 0; i < n_cases; i++) {
        const bool hit = buf[i].hits[0] == TT_TERRAIN_MESH_ID;
        if (hit != (cases[i].hit != 0) || (hit && buf[i].hits[1] != (uint32_t)cases[i].terrain)) {
            std::printf("special ray %u: hit %d terrain %u, expected %d / %d\n", i, (int)hit, buf[i].hits[1], cases[i].hit,
                        cases[i].terrain);
            bad++;
        }
        if (!hit && std::memcmp(buf[i].hits, cases[i].ray.hits, 16) != 0) {
            std::printf("special ray %u: a miss changed the record\n", i);
            bad++;
        }
    }
    if (!(detail[3] & 2u) || !(detail[4] & 2u)) {
        std::printf("the rays from below the surface did not take the bisection\n");
        bad++;
    }
    for (uint32_t i = n_cases; i < n; i++) {
        float t;
        std::memcpy(&t, &buf[i].hits[2], 4);
        // u, v belong to the last sample, which the origin shift of :649 puts 0.0001 beyond t along the ray
        const float ts = t + 0.0001f, y = buf[i].origin[1] + buf[i].direction[1] * t;
        const float x = buf[i].origin[0] + buf[i].direction[0] * ts, z = buf[i].origin[2] + buf[i].direction[2] * ts;
        const float u = (float)(buf[i].hits[3] & 0xffffu) / 65535.0f, v = (float)(buf[i].hits[3] >> 16) / 65535.0f;
        if (buf[i].hits[0] != TT_TERRAIN_MESH_ID || buf[i].hits[1] != 0u || std::fabs(y - 2.01f) > 5e-4f ||
            std::fabs(u - x / 32.0f) > 1.0f / 65535.0f + 4e-7f || std::fabs(v - z / 32.0f) > 1.0f / 65535.0f + 4e-7f) {
            std::printf("plane ray %u: mesh %u y %.7f u %.7f (x/32 %.7f) v %.7f (z/32 %.7f)\n", i, buf[i].hits[0], y, u,
                        x / 32.0f, v, z / 32.0f);
            bad++;
        }
    }
    // the shadow march and the normal over the same scene
    std::vector<tt_shadow_ray> srays(n);
    std::vector<uint8_t> occ(n);
    for (uint32_t i = 0; i < n; i++) {
        std::memset(&srays[i], 0, sizeof(tt_shadow_ray));
        std::memcpy(srays[i].origin, rays[i].origin, 12);
        std::memcpy(srays[i].direction, rays[i].direction, 12);
        srays[i].t = (i % 5u == 0u) ? 0.0f : ((i & 1u) ? -60.0f : 60.0f);
    }
    if (tt_terrain_occluded_host(terrains, 2, map.data(), 8, 8, srays.data(), n, occ.data(), &st) != TT_OK) return 2;
    for (uint32_t i = n_cases; i < n; i++)
        if ((occ[i] != 0) != (srays[i].t != 0.0f)) {  // every plane ray ends on the surface within 60 units
            std::printf("shadow ray %u: occluded %d with t %g\n", i, (int)occ[i], (double)srays[i].t);
            bad++;
        }
    const float pos[3] = {10.0f, 2.01f, 10.0f};
    float nrm[3];
    if (tt_terrain_normal_host(terrains, 2, map.data(), 8, 8, pos, 0, nrm) != TT_OK) return 2;
    // cross(+x, +z) on a flat heightmap, as the reference writes it: (0, -1, 0)
    if (nrm[0] != 0.0f || nrm[1] != -1.0f || nrm[2] != 0.0f) {
        std::printf("flat normal (%g, %g, %g)\n", (double)nrm[0], (double)nrm[1], (double)nrm[2]);
        bad++;
    }
    std::printf("terrain KAT: %u special rays, %u plane rays, %d mismatches\n", n_cases, n_plane, bad);
    return bad ? 1 : 0;
}
