// Stand-alone program over the split entropy path of the Motion-JPEG reader: csrc/jpeg_parse.cpp, csrc/jpeg_entropy.h and
// csrc/jpeg_entropy_split.h, compiled with g++ (tests/test_mjpeg_split_host.py; once more under the address and undefined-behaviour
// sanitizers over broken streams).
//   jpeg_split_main <in> <sub_bytes> [<sub_bytes> ...]
// <in>: records of (uint32 length, the bytes of one JPEG).  One line on stdout per record and sub_bytes:
//   <record> <sub_bytes> refused
//   <record> <sub_bytes> <equal> <serial status> <split status> <serial digest> <split digest> <intervals> <subsequences> <rounds>
//            <symbols> <restarts> <passed> <stuffed starts> <longest block> <effective sub_bytes>
// every interval of the frame decoded by decode_interval_host and by decode_interval_split_host; equal: 1 iff all coefficients are the
// same; the digests are FNV-1a over the coefficients' bytes; subsequences, symbols, restarts, passed, stuffed starts are sums over the
// frame's intervals, rounds, longest block and sub_bytes the largest of any.
// Every stream is copied into an allocation of exactly its length and both coefficient buffers are sized exactly, so that a read or
// write past either is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "jpeg_entropy_split.h"
#include "jpeg_parse.h"

using namespace padel;

static unsigned long long fnv(const void* p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <in> <sub_bytes> [<sub_bytes> ...]\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t len;
    for (int rec = 0; fread(&len, 4, 1, in) == 1; ++rec) {
        uint8_t* jpg = (uint8_t*)malloc(len ? len : 1);
        if (len && fread(jpg, 1, len, in) != len) { fprintf(stderr, "short record\n"); return 2; }
        pa_jpeg_frame_info info;
        std::vector<pa_jpeg_interval> ivls;
        std::string why;
        if (jpeg_parse_frame(jpg, len, &info, ivls, why)) {
            for (int a = 2; a < argc; ++a) printf("%d %d refused\n", rec, atoi(argv[a]));
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
        const size_t ncoef = (size_t)info.mcus_x * info.mcus_y * 6 * 64;
        int16_t* serial = (int16_t*)malloc(ncoef * sizeof(int16_t));
        int16_t* split = (int16_t*)malloc(ncoef * sizeof(int16_t));
        int st_serial = info.status;
        for (const pa_jpeg_interval& v : ivls)
            st_serial |= jpeg::decode_interval_host(jpg, v.begin, v.end, v.mcus, cdc, cac, serial + (size_t)v.first_mcu * 6 * 64);
        for (int a = 2; a < argc; ++a) {
            const int S = atoi(argv[a]);
            memset(split, 0x5a, ncoef * sizeof(int16_t));
            int st_split = info.status;
            jpeg::SplitStats sum = {0, 0, 0, 0, 0, 0, 0, 0};
            for (const pa_jpeg_interval& v : ivls) {
                jpeg::SplitStats s;
                st_split |= jpeg::decode_interval_split_host(jpg, v.begin, v.end, v.mcus, cdc, cac, S, split + (size_t)v.first_mcu * 6 * 64, &s);
                sum.subsequences += s.subsequences;
                sum.symbols += s.symbols;
                sum.restarts += s.restarts;
                sum.passed += s.passed;
                sum.stuffed_starts += s.stuffed_starts;
                if (s.rounds > sum.rounds) sum.rounds = s.rounds;
                if (s.longest_block > sum.longest_block) sum.longest_block = s.longest_block;
                if (s.sub_bytes > sum.sub_bytes) sum.sub_bytes = s.sub_bytes;
            }
            // (MCUs no interval covers are in neither answer: compare what the intervals cover)
            int equal = 1;
            unsigned long long ha = 1469598103934665603ull, hb = ha;
            for (const pa_jpeg_interval& v : ivls) {
                const size_t at = (size_t)v.first_mcu * 6 * 64, n = (size_t)v.mcus * 6 * 64 * sizeof(int16_t);
                if (memcmp(serial + at, split + at, n)) equal = 0;
                ha ^= fnv(serial + at, n);
                hb ^= fnv(split + at, n);
            }
            printf("%d %d %d %d %d %016llx %016llx %d %d %d %lld %d %d %d %d %d\n", rec, S, equal, st_serial, st_split, ha, hb, (int)ivls.size(),
                   sum.subsequences, sum.rounds, sum.symbols, sum.restarts, sum.passed, sum.stuffed_starts, sum.longest_block, sum.sub_bytes);
        }
        free(split); free(serial); free(jpg);
    }
    fclose(in);
    return 0;
}
