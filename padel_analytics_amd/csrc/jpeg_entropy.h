// The entropy decoder of the Motion-JPEG reader (include/padel_hip.h, pa_jpeg_decode): the bits of one restart interval -> blocks of
// 64 coefficients in zig-zag order.  One definition for host and device: jpeg_decode.hip runs it (lane 0 of the wave that owns the
// interval), tests/jpeg_decode_main.cpp compiles it with g++ and runs it, under the sanitizers, over broken streams.
// Bounded by construction: the reader never touches a byte outside [begin, end) and hands out zeros past it; the coefficient index
// never passes 63; a table lookup is masked to the table; how many blocks an interval has is the caller's number, never the data's.
#pragma once
#include "jpeg_tables.h"

namespace padel {
namespace jpeg {

enum { kStCode = 1, kStIndex = 2, kStSize = 4, kStData = 8, kStMarkers = 16 };      // PA_JPEG_ST_*

// One Huffman table in decoding form.  A code of length l matches the 16 bits ahead, v, iff v < limit[l - 1] and no shorter length
// matched (limit is non-decreasing); its symbol is vals[(off[l - 1] + (v >> (16 - l))) & 255].  look[v >> 8] answers in one read
// for the codes of up to 8 bits, which are nearly all that occur: length << 8 | symbol, 0 where the code is longer (or none matches).
struct HuffDec {
    uint32_t limit[16];
    int32_t off[16];
    uint8_t vals[256];
    uint16_t look[256];
};

inline void huff_dec_build(const uint8_t bits[16], const uint8_t* vals, int nvals, HuffDec* d) {
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        d->off[l - 1] = k - (int32_t)code;
        code += bits[l - 1];
        k += bits[l - 1];
        d->limit[l - 1] = code << (16 - l);
        code <<= 1;
    }
    for (int i = 0; i < 256; ++i) d->vals[i] = i < nvals ? vals[i] : 0;
    for (int v = 0; v < 256; ++v) {
        d->look[v] = 0;
        for (int l = 1; l <= 8; ++l)
            if (((uint32_t)v << 8) < d->limit[l - 1]) {          // every 16-bit value with these 8 bits ahead matches at length l
                d->look[v] = (uint16_t)(l << 8 | d->vals[(d->off[l - 1] + (v >> (8 - l))) & 255]);
                break;
            }
    }
}

// MSB-first reader over p[pos .. end): FF 00 is the byte FF, any other FF ends the data; past the end every bit is 0.
// 32-bit positions and counts: an interval has at most kMaxFrameBytes bytes, and an interval of the most blocks a frame can have
// takes at most 6 * 2^16 * (27 + 63 * 26) < 2^30 bits.
constexpr long long kMaxFrameBytes = 1ll << 27;     // PA_JPEG_DEC_MAX_BYTES: 8 bits of each still count in an int32
struct BitReader {
    const uint8_t* p;        // the interval's first byte
    uint32_t pos, end;
    uint64_t acc;            // the low n bits are the bits ahead
    int n;
    int32_t fed, taken;      // bits handed in from the data / bits consumed
};

PA_JHD void br_init(BitReader* r, const uint8_t* p, long long begin, long long end) {
    const long long len = end - begin;
    r->p = p + begin; r->pos = 0; r->end = len < 0 ? 0u : (len > kMaxFrameBytes ? (uint32_t)kMaxFrameBytes : (uint32_t)len);
    r->acc = 0; r->n = 0; r->fed = 0; r->taken = 0;
}
// at least 33 bits ahead afterwards.  Four bytes at a time where none of them is FF and all lie inside the data, else one
PA_JHD void br_fill(BitReader* r) {
    while (r->n <= 32) {
        if (r->pos + 4 <= r->end) {
            const uint8_t* q = r->p + r->pos;
            const uint32_t w = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3];
            if (((~w - 0x01010101u) & w & 0x80808080u) == 0) {   // no byte of ~w is 0: no byte of w is FF
                r->acc = r->acc << 32 | w;
                r->n += 32;
                r->pos += 4;
                r->fed += 32;
                continue;
            }
        }
        uint32_t b = 0;
        if (r->pos < r->end) {
            b = r->p[r->pos];
            if (b != 0xff) { ++r->pos; r->fed += 8; }
            else if (r->pos + 1 < r->end && r->p[r->pos + 1] == 0) { r->pos += 2; r->fed += 8; }
            else { r->pos = r->end; b = 0; }
        }
        r->acc = r->acc << 8 | b;
        r->n += 8;
    }
}
// the next s bits (0 <= s <= 16) as a number
PA_JHD uint32_t br_get(BitReader* r, int s) {
    br_fill(r);
    r->n -= s;
    r->taken += s;
    return (uint32_t)(r->acc >> r->n) & ((1u << s) - 1u);
}
// one symbol; -1: no code of the table matches the bits ahead
PA_JHD int huff_decode(BitReader* r, const HuffDec* t) {
    br_fill(r);
    const uint32_t v = (uint32_t)(r->acc >> (r->n - 16)) & 0xffffu;
    const uint32_t hit = t->look[v >> 8];
    if (hit) {
        r->n -= (int)(hit >> 8);
        r->taken += (int32_t)(hit >> 8);
        return (int)(hit & 255u);
    }
    int l = 9;
    while (l <= 16 && v >= t->limit[l - 1]) ++l;
    if (l > 16) return -1;
    r->n -= l;
    r->taken += l;
    return t->vals[(t->off[l - 1] + (int32_t)(v >> (16 - l))) & 255];
}
PA_JHD int extend(uint32_t bits, int s) { return bits < (1u << (s - 1)) ? (int)bits - (1 << s) + 1 : (int)bits; }

// One block into out[0 .. 64), which the caller has zeroed.  *pred: the component's DC so far in this interval.  0 or the kSt* bit
// of what stopped it; after a non-zero answer out[] is to be discarded.
PA_JHD int decode_block(BitReader* r, const HuffDec* dc, const HuffDec* ac, int* pred, int16_t* out) {
    int s = huff_decode(r, dc);
    if (s < 0) return kStCode;
    if (s > 11) return kStSize;
    if (s) *pred += extend(br_get(r, s), s);
    out[0] = (int16_t)*pred;
    int k = 1;
    while (k < 64) {
        const int rs = huff_decode(r, ac);
        if (rs < 0) return kStCode;
        s = rs & 15;
        if (s == 0) {
            if (rs != 0xf0) break;           // end of block
            k += 16;
            continue;
        }
        if (s > 10) return kStSize;
        k += rs >> 4;
        if (k > 63) return kStIndex;
        out[k++] = (int16_t)extend(br_get(r, s), s);
    }
    if (k > 64) return kStIndex;
    if (r->taken > r->fed) return kStData;
    return 0;
}

// The whole interval on the host: `mcus` MCUs of 6 blocks (Y00 Y01 Y10 Y11 Cb Cr) into coef[mcus * 6 * 64]; from the block that
// cannot be decoded on, zeros.  Returns the status bits.
inline int decode_interval_host(const uint8_t* p, long long begin, long long end, int mcus, const HuffDec* dc[3], const HuffDec* ac[3],
                                int16_t* coef) {
    BitReader r;
    br_init(&r, p, begin, end);
    int pred[3] = {0, 0, 0}, st = 0;
    for (long long b = 0; b < (long long)mcus * 6; ++b) {
        int16_t* out = coef + b * 64;
        for (int i = 0; i < 64; ++i) out[i] = 0;
        if (st) continue;
        const int c = b % 6 < 4 ? 0 : (int)(b % 6) - 3;
        st = decode_block(&r, dc[c], ac[c], &pred[c], out);
        if (st)
            for (int i = 0; i < 64; ++i) out[i] = 0;
    }
    return st;
}

}  // namespace jpeg
}  // namespace padel
