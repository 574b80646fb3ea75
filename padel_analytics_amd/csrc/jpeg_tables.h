// The constants of the Motion-JPEG writer (include/padel_hip.h, pa_jpeg_encode): zig-zag order, the Annex K quantisation and Huffman
// tables of ITU-T T.81, libjpeg's quality rule, the integer forward DCT and the worst-case size of a restart interval.  No HIP, no
// runtime call: jpeg_encode.hip, jpeg_check.cpp (host only) and tests/jpeg_tables_main.cpp (g++) all include it.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PA_JHD __host__ __device__ __forceinline__
#define PA_JUNROLL _Pragma("unroll")
#else
#define PA_JHD inline
#define PA_JUNROLL
#endif

namespace padel {
namespace jpeg {

constexpr int kMaxWidth = 2560;              // PA_JPEG_MAX_WIDTH: what the encode kernel's LDS staging of one MCU row supports
constexpr int kBlocksPerMcu = 6;             // Y00 Y01 Y10 Y11 Cb Cr
// one 8 x 8 block codes to at most 22 bits of DC (chroma: the 11-bit code of category 11 + 11 bits; luma: 9 + 11 = 20) plus
// 63 x (16-bit code + 10 bits) of AC: 22 + 1638 = 1660 bits = 207.5 bytes.  (8-bit samples: |DC| <= 1024 before prediction, so a
// difference has at most 11 bits, and |AC| <= 128 * 8 * 0.906 < 1024, at most 10.)
constexpr int kBlockMaxBytes = 208;

// zig-zag position k -> index 8 * row + column inside the block
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.1 / K.2, row-major
constexpr uint8_t kQuantLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                    14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                    18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kQuantChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                      24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// libjpeg's quality rule: Q in 1..100 -> the table entry for one Annex K base value
PA_JHD int quality_scale(int q) { return q < 50 ? 5000 / q : 200 - 2 * q; }
PA_JHD int quant_entry(int base, int q) {
    const int v = (base * quality_scale(q) + 50) / 100;
    return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// ---- Annex K.3 - K.6: the Huffman tables as DHT carries them (codes per length 1..16, then the symbols in code order)
struct HuffSpec { uint8_t bits[16]; int nvals; uint8_t vals[162]; };
constexpr HuffSpec kDcLumaSpec = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kDcChromaSpec = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kAcLumaSpec = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162,
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec kAcChromaSpec = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162,
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// the same tables as (code, length) per symbol; length 0: the table has no such symbol
struct HuffTable { uint16_t code[256]; uint8_t len[256]; };
constexpr HuffTable make_huff_table(const HuffSpec& s) {
    HuffTable t{};
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < s.bits[l - 1]; ++i, ++k, ++code) {
            t.code[s.vals[k]] = (uint16_t)code;
            t.len[s.vals[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
    return t;
}
constexpr HuffTable kDcLuma = make_huff_table(kDcLumaSpec), kDcChroma = make_huff_table(kDcChromaSpec);
constexpr HuffTable kAcLuma = make_huff_table(kAcLumaSpec), kAcChroma = make_huff_table(kAcChromaSpec);

// ---- the forward DCT: Loeffler-Ligtenberg-Moshovitz with 13-bit constants (libjpeg's "islow"), one pass over 8 values.
// ROWS = true: the first pass (rows), results scaled by 4; ROWS = false: the second pass (columns) over the first pass's results,
// results scaled by 8 in all.  descale(x, n) = (x + (1 << (n - 1))) >> n, >> arithmetic; every intermediate fits int32.
PA_JHD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
template <bool ROWS> PA_JHD void fdct8(int* d0, int* d1, int* d2, int* d3, int* d4, int* d5, int* d6, int* d7) {
    constexpr int kConst = 13, kPass1 = 2, kOdd = ROWS ? kConst - kPass1 : kConst + kPass1;
    const int t0 = *d0 + *d7, t7 = *d0 - *d7, t1 = *d1 + *d6, t6 = *d1 - *d6;
    const int t2 = *d2 + *d5, t5 = *d2 - *d5, t3 = *d3 + *d4, t4 = *d3 - *d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (ROWS) {
        *d0 = (t10 + t11) * (1 << kPass1);
        *d4 = (t10 - t11) * (1 << kPass1);
    } else {
        *d0 = descale(t10 + t11, kPass1);
        *d4 = descale(t10 - t11, kPass1);
    }
    const int z = (t12 + t13) * 4433;
    *d2 = descale(z + t13 * 6270, kOdd);
    *d6 = descale(z - t12 * 15137, kOdd);
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995;
    const int z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
    *d7 = descale(t4 * 2446 + z1 + z3, kOdd);
    *d5 = descale(t5 * 16819 + z2 + z4, kOdd);
    *d3 = descale(t6 * 25172 + z2 + z3, kOdd);
    *d1 = descale(t7 * 12299 + z1 + z4, kOdd);
}
// 64 level-shifted samples (row-major) -> 64 coefficients scaled by 8, in place: rows first, then columns
PA_JHD void fdct_block(int* b) {
    PA_JUNROLL
    for (int r = 0; r < 8; ++r) fdct8<true>(b + 8 * r, b + 8 * r + 1, b + 8 * r + 2, b + 8 * r + 3, b + 8 * r + 4, b + 8 * r + 5, b + 8 * r + 6, b + 8 * r + 7);
    PA_JUNROLL
    for (int c = 0; c < 8; ++c) fdct8<false>(b + c, b + 8 + c, b + 16 + c, b + 24 + c, b + 32 + c, b + 40 + c, b + 48 + c, b + 56 + c);
}
// quantisation of one coefficient scaled by 8 with table entry q
PA_JHD int quantise(int c, int q) {
    const int a = ((c < 0 ? -c : c) + 4 * q) / (8 * q);
    return c < 0 ? -a : a;
}

// ---- sizes
PA_JHD int mcus_per_row(int w) { return (w + 15) / 16; }
PA_JHD int mcu_rows(int h) { return (h + 15) / 16; }
// the most bytes one restart interval (one MCU row) of a frame of width w can take, its closing RSTm / EOI marker included: every
// block at its worst, every byte stuffed, one byte of padding
PA_JHD size_t interval_max_bytes(int w) { return 2 * ((size_t)mcus_per_row(w) * kBlocksPerMcu * kBlockMaxBytes + 1) + 2; }

}  // namespace jpeg
}  // namespace padel
