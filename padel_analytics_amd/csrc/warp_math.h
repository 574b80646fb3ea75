// The arithmetic of pa_warp_perspective (include/padel_hip.h), for host and device: one output pixel of the perspective resample.
//   X = (m0 u + m1 v) + m2,  Y = (m3 u + m4 v) + m5,  Z = (m6 u + m7 v) + m8        IEEE double, every operation rounded on its own
//   fill unless Z > 0;  sx = X / Z, sy = Y / Z;  fill unless -1 < sx < w and -1 < sy < h  (NaN and infinities fail the comparisons)
//   qx = (int32) floor(sx * 32), x0 = qx >> 5, wx = qx & 31, the same in y;  bilinear in int32 over P(x, y) = the source pixel inside
//   the frame, fill outside:  out = (top (32 - wy) + bot wy + 512) >> 10,  top = P(x0, y0) (32 - wx) + P(x0 + 1, y0) wx.
// The weights come from floor(32 s), never from s - floor(s): that difference rounds to 1 for a tiny negative s.
// EVERY translation unit that includes this file is compiled with -ffp-contract=off (csrc/build.sh, tests/warp_main.cpp's command
// line): a fused multiply-add in the three sums is another number, and the _rn intrinsics do not keep hipcc -O3 from fusing
// them.  No HIP runtime call, no table.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PA_WARP_HD __host__ __device__ __forceinline__
#else
#define PA_WARP_HD inline
#endif

namespace padel {

constexpr int kWarpMaxDim = 4096;      // PA_WARP_MAX_DIM
constexpr int kWarpFracBits = 5;       // weights in 1 / 32 pixel

// channel c of P(x, y): `frame` is h x w packed BGR, fill is B | G << 8 | R << 16
PA_WARP_HD int warp_tap(const uint8_t* frame, int h, int w, int x, int y, int c, uint32_t fill) {
    if (x < 0 || x >= w || y < 0 || y >= h) return (int)((fill >> (8 * c)) & 0xff);
    return frame[((size_t)y * w + x) * 3 + c];
}

// output pixel (u, v) of one frame as B | G << 8 | R << 16.  m: the frame's nine doubles, canvas -> source
PA_WARP_HD uint32_t warp_pixel(const uint8_t* frame, int h, int w, const double* m, int valid, int u, int v, uint32_t fill) {
    fill &= 0xffffffu;
    if (!valid) return fill;
    const double du = (double)u, dv = (double)v;
    const double X = (m[0] * du + m[1] * dv) + m[2];
    const double Y = (m[3] * du + m[4] * dv) + m[5];
    const double Z = (m[6] * du + m[7] * dv) + m[8];
    if (!(Z > 0.0)) return fill;
    const double sx = X / Z, sy = Y / Z;
    if (!(sx > -1.0 && sx < (double)w && sy > -1.0 && sy < (double)h)) return fill;
    const int32_t qx = (int32_t)floor(sx * 32.0), qy = (int32_t)floor(sy * 32.0);      // in [-32, 32 w) and [-32, 32 h)
    const int x0 = qx >> kWarpFracBits, y0 = qy >> kWarpFracBits, wx = qx & 31, wy = qy & 31;
    uint32_t out = 0;
    for (int c = 0; c < 3; ++c) {
        const int top = warp_tap(frame, h, w, x0, y0, c, fill) * (32 - wx) + warp_tap(frame, h, w, x0 + 1, y0, c, fill) * wx;
        const int bot = warp_tap(frame, h, w, x0, y0 + 1, c, fill) * (32 - wx) + warp_tap(frame, h, w, x0 + 1, y0 + 1, c, fill) * wx;
        out |= (uint32_t)((top * (32 - wy) + bot * wy + 512) >> 10) << (8 * c);
    }
    return out;
}

}  // namespace padel
