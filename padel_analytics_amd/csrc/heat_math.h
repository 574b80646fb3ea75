// The arithmetic of pa_heat_accumulate (include/padel_hip.h), for host and device.  All integer, nothing rounded but by floor division.
//   splat    a point (x, y) of radius r adds  k(d2) = (255 (r r - d2)) / (r r)  to pixel (u, v), d2 = (u - x)^2 + (v - y)^2 < r r: an
//            Epanechnikov bump, 255 at the centre, 0 on the rim and beyond.  r <= 255, so 255 r r < 2^24.
//   add      saturating at 2^32 - 1.
//   level    D >= full ? 255 : (D 255) / full, full in 1 .. 2^24 - 1: below full, D 255 < 2^32.
//   blend    a = (alpha level) >> 8, alpha in 0 .. 256;  p = (p (256 - a) + c a + 128) >> 8 per channel, c = lut[level]: PA_MARK_BLEND's rule.
//            a == 0 leaves p as it is by that same formula.
// No HIP runtime call, no table.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PA_HEAT_HD __host__ __device__ __forceinline__
#else
#define PA_HEAT_HD inline
#endif

namespace padel {

constexpr int kHeatMaxDim = 4096;                   // PA_WARP_MAX_DIM: the canvases are the warp's
constexpr int kHeatMaxPoints = 64;                  // PA_HEAT_MAX_POINTS, per frame
constexpr int kHeatMaxPlanes = 4;                   // PA_HEAT_MAX_PLANES
constexpr int kHeatMaxRadius = 255;                 // PA_HEAT_MAX_RADIUS
constexpr int kHeatMaxCoord = 32767;                // PA_HEAT_MAX_COORD: |x|, |y| of a point
constexpr uint32_t kHeatMaxFull = (1u << 24) - 1;   // PA_HEAT_MAX_FULL

// what a point at distance (dx, dy) from a pixel adds to it.  |dx|, |dy| are tested first: their squares alone can leave int32
PA_HEAT_HD uint32_t heat_splat(int dx, int dy, int r) {
    if (dx <= -r || dx >= r || dy <= -r || dy >= r) return 0;
    const int r2 = r * r, d2 = dx * dx + dy * dy;
    return d2 < r2 ? (uint32_t)(255 * (r2 - d2)) / (uint32_t)r2 : 0u;
}

PA_HEAT_HD uint32_t heat_add(uint32_t d, uint32_t k) {
    const uint32_t s = d + k;
    return s < d ? 0xffffffffu : s;
}

PA_HEAT_HD uint32_t heat_level(uint32_t d, uint32_t full) { return d >= full ? 255u : (d * 255u) / full; }

PA_HEAT_HD uint32_t heat_weight(uint32_t level, int alpha) { return ((uint32_t)alpha * level) >> 8; }

// one channel: p under colour c at weight a (0 .. 255)
PA_HEAT_HD uint32_t heat_mix(uint32_t p, uint32_t c, uint32_t a) { return (p * (256u - a) + c * a + 128u) >> 8; }

// the pixel B | G << 8 | R << 16 under colour c (packed alike) at weight a
PA_HEAT_HD uint32_t heat_blend(uint32_t bgr, uint32_t c, uint32_t a) {
    return heat_mix(bgr & 0xff, c & 0xff, a) | heat_mix((bgr >> 8) & 0xff, (c >> 8) & 0xff, a) << 8 |
           heat_mix((bgr >> 16) & 0xff, (c >> 16) & 0xff, a) << 16;
}

// the pixel under the map: d the shown density; lut 256 x 3 bytes of BGR
PA_HEAT_HD uint32_t heat_pixel(uint32_t bgr, uint32_t d, uint32_t full, int alpha, const uint8_t* lut) {
    const uint32_t level = heat_level(d, full), a = heat_weight(level, alpha);
    if (a == 0) return bgr & 0xffffffu;
    const uint8_t* const c = lut + 3 * level;
    return heat_blend(bgr, (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16, a);
}

}  // namespace padel
