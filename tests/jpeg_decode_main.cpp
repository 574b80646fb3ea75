// Stand-alone program over the host-side pieces of the Motion-JPEG reader: csrc/jpeg_parse.cpp, csrc/jpeg_entropy.h and
// csrc/jpeg_idct.h, compiled with g++ (tests/test_mjpeg_decode_host.py; once more under the address and undefined-behaviour
// sanitizers over broken streams).
//   jpeg_decode_main <in> <out>
// <in>: records of (uint32 length, the bytes of one JPEG).  <out>, per record: int32 refused, status, w, h, intervals, int64
// coefficient count, the coefficients (int16, [MCU][6][64], zig-zag), then h * w * 3 bytes BGR.  A refused stream has zeros in the
// five numbers behind `refused` and nothing after them.
// Every stream is copied into an allocation of exactly its length and every result buffer is sized exactly, so that a read or write
// past either is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "jpeg_entropy.h"
#include "jpeg_idct.h"
#include "jpeg_parse.h"

using namespace padel;

static void put(FILE* f, const void* p, size_t n) {
    if (n && fwrite(p, 1, n, f) != n) { fprintf(stderr, "short write\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    uint32_t len;
    while (fread(&len, 4, 1, in) == 1) {
        uint8_t* jpg = (uint8_t*)malloc(len ? len : 1);
        if (len && fread(jpg, 1, len, in) != len) { fprintf(stderr, "short record\n"); return 2; }
        pa_jpeg_frame_info info;
        std::vector<pa_jpeg_interval> ivls;
        std::string why;
        int32_t head[4] = {0, 0, 0, 0};
        int64_t ncoef = 0;
        if (jpeg_parse_frame(jpg, len, &info, ivls, why)) {
            const int32_t refused = 1;
            put(out, &refused, 4); put(out, head, 16); put(out, &ncoef, 8);
            free(jpg);
            continue;
        }
        jpeg::HuffDec dc[2], ac[2];
        for (int t = 0; t < 2; ++t) {
            jpeg::huff_dec_build(info.dc[t].bits, info.dc[t].vals, info.dc[t].nvals, &dc[t]);
            jpeg::huff_dec_build(info.ac[t].bits, info.ac[t].vals, info.ac[t].nvals, &ac[t]);
        }
        const jpeg::HuffDec* cdc[3] = {&dc[info.comp_dc[0]], &dc[info.comp_dc[1]], &dc[info.comp_dc[2]]};
        const jpeg::HuffDec* cac[3] = {&ac[info.comp_ac[0]], &ac[info.comp_ac[1]], &ac[info.comp_ac[2]]};
        const size_t mcus = (size_t)info.mcus_x * info.mcus_y;
        ncoef = (int64_t)(mcus * 6 * 64);
        int16_t* coef = (int16_t*)malloc((size_t)ncoef * sizeof(int16_t));
        int status = info.status;
        for (const pa_jpeg_interval& v : ivls)
            status |= jpeg::decode_interval_host(jpg, v.begin, v.end, v.mcus, cdc, cac, coef + (size_t)v.first_mcu * 6 * 64);
        // planes, as the kernels lay them out
        const size_t PW = (size_t)info.mcus_x * 16, PH = (size_t)info.mcus_y * 16;
        uint8_t* planes = (uint8_t*)malloc(PW * PH * 3 / 2);
        for (size_t m = 0; m < mcus; ++m)
            for (int k = 0; k < 6; ++k) {
                const int comp = k < 4 ? 0 : k - 3;
                int32_t b[64];
                for (int i = 0; i < 64; ++i) b[jpeg::kZigzag[i]] = (int32_t)coef[(m * 6 + k) * 64 + i] * info.quant[comp][i];
                jpeg::idct_block(b);
                const size_t my = m / info.mcus_x, mx = m % info.mcus_x;
                uint8_t* p;
                size_t pitch;
                if (k < 4) { pitch = PW; p = planes + (my * 16 + (k >> 1) * 8) * PW + mx * 16 + (k & 1) * 8; }
                else { pitch = PW / 2; p = planes + PW * PH + (k == 5 ? PW * PH / 4 : 0) + my * 8 * pitch + mx * 8; }
                for (int r = 0; r < 8; ++r)
                    for (int c = 0; c < 8; ++c) p[r * pitch + c] = (uint8_t)jpeg::sample(b[8 * r + c]);
            }
        const int h = info.h, w = info.w, ch = (h + 1) / 2, cw = (w + 1) / 2;
        uint8_t* bgr = (uint8_t*)malloc((size_t)h * w * 3);
        const uint8_t* Cp[2] = {planes + PW * PH, planes + PW * PH + PW * PH / 4};
        for (int y = 0; y < h; ++y) {
            const int r = y >> 1, rr = (y & 1) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
            for (int x = 0; x < w; ++x) {
                const int c = x >> 1;
                int cc[2];
                for (int pl = 0; pl < 2; ++pl) {
                    auto s = [&](int col) {
                        col = col < 0 ? 0 : (col > cw - 1 ? cw - 1 : col);
                        return 3 * Cp[pl][(size_t)r * (PW / 2) + col] + Cp[pl][(size_t)rr * (PW / 2) + col];
                    };
                    cc[pl] = (x & 1) ? jpeg::chroma_odd(s(c), s(c + 1)) : jpeg::chroma_even(s(c - 1), s(c));
                }
                jpeg::ycc_to_bgr(planes[(size_t)y * PW + x], cc[0], cc[1], bgr + ((size_t)y * w + x) * 3);
            }
        }
        const int32_t refused = 0;
        head[1] = w; head[2] = h; head[0] = status;
        put(out, &refused, 4); put(out, &head[0], 4); put(out, &head[1], 4); put(out, &head[2], 4);
        const int32_t n_ivls = (int32_t)ivls.size();
        put(out, &n_ivls, 4); put(out, &ncoef, 8);
        put(out, coef, (size_t)ncoef * sizeof(int16_t));
        put(out, bgr, (size_t)h * w * 3);
        free(bgr); free(planes); free(coef); free(jpg);
    }
    fclose(in);
    if (fclose(out)) { fprintf(stderr, "cannot close the output\n"); return 2; }
    return 0;
}
