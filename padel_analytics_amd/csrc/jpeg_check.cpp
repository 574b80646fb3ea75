// What is decided about a pa_jpeg_encode call before anything runs: host-only code (no HIP runtime call), built with g++ like
// render_check.cpp, so that the same refusals, tables and sizes are available without a GPU (pa_jpeg_check, pa_jpeg_interval_bytes).
#include "jpeg_check.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace padel {

static_assert(jpeg::kMaxWidth == PA_JPEG_MAX_WIDTH, "the width limit is stated twice");

#define FAIL(...)                                                \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        err = _b;                                                \
        return 1;                                                \
    } while (0)

void jpeg_quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {
    for (int i = 0; i < 64; ++i) {
        luma[i] = (uint8_t)jpeg::quant_entry(jpeg::kQuantLuma[i], quality);
        chroma[i] = (uint8_t)jpeg::quant_entry(jpeg::kQuantChroma[i], quality);
    }
}

static uint8_t* put16(uint8_t* p, int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; return p; }
static uint8_t* put_dht(uint8_t* p, int id, const jpeg::HuffSpec& s) {
    *p++ = (uint8_t)id;
    memcpy(p, s.bits, 16); p += 16;
    memcpy(p, s.vals, (size_t)s.nvals); p += s.nvals;
    return p;
}

void jpeg_build_header(int h, int w, int quality, uint8_t* out) {
    uint8_t qy[64], qc[64];
    jpeg_quant_tables(quality, qy, qc);
    uint8_t* p = out;
    p = put16(p, 0xffd8);                                        // SOI
    p = put16(p, 0xffe0); p = put16(p, 16);                      // APP0: JFIF 1.01, no units, aspect 1:1, no thumbnail
    memcpy(p, "JFIF", 5); p += 5;
    *p++ = 1; *p++ = 1; *p++ = 0; p = put16(p, 1); p = put16(p, 1); *p++ = 0; *p++ = 0;
    p = put16(p, 0xffdb); p = put16(p, 2 + 2 * 65);              // DQT: two 8-bit tables, zig-zag order
    *p++ = 0; for (int k = 0; k < 64; ++k) *p++ = qy[jpeg::kZigzag[k]];
    *p++ = 1; for (int k = 0; k < 64; ++k) *p++ = qc[jpeg::kZigzag[k]];
    p = put16(p, 0xffc0); p = put16(p, 17); *p++ = 8;            // SOF0: 8 bits, the true size, Y 2x2 table 0, Cb / Cr 1x1 table 1
    p = put16(p, h); p = put16(p, w); *p++ = 3;
    *p++ = 1; *p++ = 0x22; *p++ = 0;
    *p++ = 2; *p++ = 0x11; *p++ = 1;
    *p++ = 3; *p++ = 0x11; *p++ = 1;
    p = put16(p, 0xffc4); p = put16(p, 2 + 2 * (17 + 12) + 2 * (17 + 162));   // DHT: DC 0, AC 0, DC 1, AC 1
    p = put_dht(p, 0x00, jpeg::kDcLumaSpec);
    p = put_dht(p, 0x10, jpeg::kAcLumaSpec);
    p = put_dht(p, 0x01, jpeg::kDcChromaSpec);
    p = put_dht(p, 0x11, jpeg::kAcChromaSpec);
    p = put16(p, 0xffdd); p = put16(p, 4); p = put16(p, jpeg::mcus_per_row(w));   // DRI: one MCU row
    p = put16(p, 0xffda); p = put16(p, 12); *p++ = 3;            // SOS
    *p++ = 1; *p++ = 0x00; *p++ = 2; *p++ = 0x11; *p++ = 3; *p++ = 0x11;
    *p++ = 0; *p++ = 63; *p++ = 0;
    static_assert(kJpegHeaderBytes == 2 + 18 + 134 + 19 + 420 + 6 + 14, "header size");
}

void jpeg_fill_tables(int h, int w, int quality, JpegDevTables* t) {
    memset(t, 0, sizeof(*t));
    uint8_t q[2][64];
    jpeg_quant_tables(quality, q[0], q[1]);
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) {
            const uint32_t d = 8u * q[c][jpeg::kZigzag[k]];
            // (|c| + 4 q) < 2^17 and e = recip * d - 2^32 <= d <= 2040, so n * e < 2^32: the high word of n * recip is n / d exactly
            t->recip[c][k] = (uint32_t)((1ull << 32) / d) + 1;
            t->q4[c][k] = (uint16_t)(d / 2);
        }
    const jpeg::HuffTable* dc[2] = {&jpeg::kDcLuma, &jpeg::kDcChroma};
    const jpeg::HuffTable* ac[2] = {&jpeg::kAcLuma, &jpeg::kAcChroma};
    for (int c = 0; c < 2; ++c) {
        for (int s = 0; s < 12; ++s) t->dc[c][s] = (uint32_t)dc[c]->len[s] << 16 | dc[c]->code[s];
        for (int s = 0; s < 256; ++s) t->ac[c][s] = (uint32_t)ac[c]->len[s] << 16 | ac[c]->code[s];
    }
    jpeg_build_header(h, w, quality, t->header);
}

int jpeg_validate(int n, int h, int w, const pa_yuv_desc* g, int quality, size_t* src_span, std::string& err) {
    if (n < 1 || n > 65535) FAIL("pa_jpeg_encode: n = %d frames outside [1, 65535]", n);
    if (w < 2 || h < 2 || (w & 1) || (h & 1)) FAIL("pa_jpeg_encode: %d x %d frames: 4:2:0 needs an even width and height of at least 2", w, h);
    if (w > PA_JPEG_MAX_WIDTH) FAIL("pa_jpeg_encode: width %d is beyond the %d pixels one workgroup stages in LDS", w, PA_JPEG_MAX_WIDTH);
    if (h > 65534) FAIL("pa_jpeg_encode: height %d is beyond what SOF0 can carry", h);
    if (quality < 1 || quality > 100) FAIL("pa_jpeg_encode: quality %d outside [1, 100]", quality);
    if (!g) FAIL("pa_jpeg_encode: the geometry descriptor is NULL");
    if (g->layout != PA_YUV_NV12 && g->layout != PA_YUV_I420) FAIL("pa_jpeg_encode: unknown layout %d", g->layout);
    const bool nv12 = g->layout == PA_YUV_NV12;
    const int crow = nv12 ? w : w / 2;
    if (g->pitch_y < w) FAIL("pa_jpeg_encode: pitch_y %d is smaller than a luma row of %d bytes", g->pitch_y, w);
    if (g->pitch_c < crow) FAIL("pa_jpeg_encode: pitch_c %d is smaller than a chroma row of %d bytes", g->pitch_c, crow);
    if (g->off_u < 0 || g->off_v < 0) FAIL("pa_jpeg_encode: negative plane offset (off_u %d, off_v %d)", g->off_u, g->off_v);
    if (nv12 && g->off_v != g->off_u + 1) FAIL("pa_jpeg_encode: NV12 needs off_v == off_u + 1 (off_u %d, off_v %d)", g->off_u, g->off_v);
    const long long y_end = (long long)(h - 1) * g->pitch_y + w;
    const long long c_len = (long long)(h / 2 - 1) * g->pitch_c + crow;
    const long long extent = std::max(y_end, std::max(g->off_u + c_len, nv12 ? 0ll : g->off_v + c_len));
    if (extent > 0x7fffffffll) FAIL("pa_jpeg_encode: a frame of %lld bytes is beyond 2 GiB", extent);
    if (g->frame_stride < extent)
        FAIL("pa_jpeg_encode: frame_stride %lld is smaller than the %lld bytes the planes of one frame span (they would reach into the next frame)",
             (long long)g->frame_stride, extent);
    *src_span = (size_t)(n - 1) * (size_t)g->frame_stride + (size_t)extent;
    return 0;
}

}  // namespace padel

extern "C" int pa_jpeg_check(int n, int h, int w, const pa_yuv_desc* geom, int quality, char* why, size_t cap) {
    std::string err;
    size_t span = 0;
    const int rc = padel::jpeg_validate(n, h, w, geom, quality, &span, err);
    if (why && cap) snprintf(why, cap, "%s", rc ? err.c_str() : "");
    return rc;
}

extern "C" size_t pa_jpeg_interval_bytes(int w) { return w < 1 ? 0 : padel::jpeg::interval_max_bytes(w); }
