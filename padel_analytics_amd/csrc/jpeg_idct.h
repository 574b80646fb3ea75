// The arithmetic of the Motion-JPEG reader behind the entropy decoder (include/padel_hip.h, pa_jpeg_decode): dequantisation and the
// inverse DCT of one block (libjpeg's "islow"), the "h2v2 fancy" chroma interpolation of one pixel pair and JFIF YCbCr -> BGR.  One
// definition for host and device (jpeg_decode.hip, tests/jpeg_decode_main.cpp).  int32 with wrap-around: the sums are formed in
// uint32, so that coefficients no encoder produces (a corrupt stream) overflow without undefined behaviour.
#pragma once
#include "jpeg_tables.h"

namespace padel {
namespace jpeg {

PA_JHD int32_t wmul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
PA_JHD int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
PA_JHD int32_t wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
PA_JHD int32_t wdescale(int32_t x, int s) { return wadd(x, 1 << (s - 1)) >> s; }

// one pass over 8 values, in place
template <int S> PA_JHD void idct8(int32_t* d0, int32_t* d1, int32_t* d2, int32_t* d3, int32_t* d4, int32_t* d5, int32_t* d6, int32_t* d7) {
    int32_t z1 = wmul(wadd(*d2, *d6), 4433);
    const int32_t t2 = wsub(z1, wmul(*d6, 15137)), t3 = wadd(z1, wmul(*d2, 6270));
    const int32_t t0 = (int32_t)((uint32_t)wadd(*d0, *d4) << 13), t1 = (int32_t)((uint32_t)wsub(*d0, *d4) << 13);
    const int32_t t10 = wadd(t0, t3), t13 = wsub(t0, t3), t11 = wadd(t1, t2), t12 = wsub(t1, t2);
    int32_t a0 = *d7, a1 = *d5, a2 = *d3, a3 = *d1;
    z1 = wadd(a0, a3);
    int32_t z2 = wadd(a1, a2), z3 = wadd(a0, a2), z4 = wadd(a1, a3);
    const int32_t z5 = wmul(wadd(z3, z4), 9633);
    a0 = wmul(a0, 2446); a1 = wmul(a1, 16819); a2 = wmul(a2, 25172); a3 = wmul(a3, 12299);
    z1 = wmul(z1, -7373); z2 = wmul(z2, -20995);
    z3 = wadd(wmul(z3, -16069), z5); z4 = wadd(wmul(z4, -3196), z5);
    a0 = wadd(a0, wadd(z1, z3)); a1 = wadd(a1, wadd(z2, z4)); a2 = wadd(a2, wadd(z2, z3)); a3 = wadd(a3, wadd(z1, z4));
    *d0 = wdescale(wadd(t10, a3), S); *d7 = wdescale(wsub(t10, a3), S);
    *d1 = wdescale(wadd(t11, a2), S); *d6 = wdescale(wsub(t11, a2), S);
    *d2 = wdescale(wadd(t12, a1), S); *d5 = wdescale(wsub(t12, a1), S);
    *d3 = wdescale(wadd(t13, a0), S); *d4 = wdescale(wsub(t13, a0), S);
}
// 64 dequantised coefficients, row-major -> the IDCT output (before + 128 and the clamp), in place: columns first, then rows
PA_JHD void idct_block(int32_t* b) {
    PA_JUNROLL
    for (int c = 0; c < 8; ++c) idct8<11>(b + c, b + 8 + c, b + 16 + c, b + 24 + c, b + 32 + c, b + 40 + c, b + 48 + c, b + 56 + c);
    PA_JUNROLL
    for (int r = 0; r < 8; ++r) idct8<18>(b + 8 * r, b + 8 * r + 1, b + 8 * r + 2, b + 8 * r + 3, b + 8 * r + 4, b + 8 * r + 5, b + 8 * r + 6, b + 8 * r + 7);
}
PA_JHD int clamp255(int32_t x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }
PA_JHD int sample(int32_t x) { return clamp255(wadd(x, 128)); }

// the two chroma values of output pixels 2 c and 2 c + 1 out of the column sums s[c - 1], s[c], s[c + 1] (s = 3 near + far)
PA_JHD int chroma_even(int sl, int sc) { return (3 * sc + sl + 8) >> 4; }
PA_JHD int chroma_odd(int sc, int sr) { return (3 * sc + sr + 7) >> 4; }

// one pixel: out[0 .. 3) = B, G, R
PA_JHD void ycc_to_bgr(int y, int cb, int cr, uint8_t* out) {
    cb -= 128; cr -= 128;
    out[0] = (uint8_t)clamp255(y + ((116130 * cb + 32768) >> 16));
    out[1] = (uint8_t)clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    out[2] = (uint8_t)clamp255(y + ((91881 * cr + 32768) >> 16));
}

}  // namespace jpeg
}  // namespace padel
