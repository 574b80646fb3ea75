// Stand-alone program over csrc/jpeg_tables.h and csrc/jpeg_check.cpp (g++, no HIP): what the Motion-JPEG kernels are built from, on
// the CPU, for tests/test_mjpeg_host.py.
//   tables                      the four Huffman tables: "<name> <symbol> <code> <length>" per symbol, then "zigzag ..." (64 numbers)
//   quant Q                     the two quantisation tables of quality Q, row-major: "luma ..." and "chroma ..."
//   blocks Q COMP IN OUT        IN: N x 64 samples (uint8, row-major blocks); OUT: N x 64 quantised coefficients (int16, row-major)
//                               with the luma (COMP 0) or chroma (COMP 1) table of quality Q
//   header H W Q OUT            the 613 bytes SOI .. SOS of an H x W frame
//   bound W                     jpeg::interval_max_bytes(W)
#include "jpeg_check.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace padel;

static void print_table(const char* name, const jpeg::HuffTable& t) {
    for (int s = 0; s < 256; ++s)
        if (t.len[s]) printf("%s %d %u %u\n", name, s, (unsigned)t.code[s], (unsigned)t.len[s]);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "tables") {
        print_table("dc_luma", jpeg::kDcLuma);
        print_table("dc_chroma", jpeg::kDcChroma);
        print_table("ac_luma", jpeg::kAcLuma);
        print_table("ac_chroma", jpeg::kAcChroma);
        printf("zigzag");
        for (int k = 0; k < 64; ++k) printf(" %d", jpeg::kZigzag[k]);
        printf("\n");
        return 0;
    }
    if (mode == "quant" && argc == 3) {
        uint8_t q[2][64];
        jpeg_quant_tables(atoi(argv[2]), q[0], q[1]);
        for (int c = 0; c < 2; ++c) {
            printf(c ? "chroma" : "luma");
            for (int i = 0; i < 64; ++i) printf(" %d", q[c][i]);
            printf("\n");
        }
        return 0;
    }
    if (mode == "blocks" && argc == 6) {
        uint8_t q[2][64];
        jpeg_quant_tables(atoi(argv[2]), q[0], q[1]);
        const int comp = atoi(argv[3]) ? 1 : 0;
        FILE* in = fopen(argv[4], "rb");
        if (!in) return 3;
        std::vector<uint8_t> px;
        uint8_t buf[64];
        while (fread(buf, 1, 64, in) == 64) px.insert(px.end(), buf, buf + 64);
        fclose(in);
        std::vector<int16_t> out(px.size());
        for (size_t b = 0; b < px.size() / 64; ++b) {
            int v[64];
            for (int i = 0; i < 64; ++i) v[i] = (int)px[b * 64 + i] - 128;
            jpeg::fdct_block(v);
            for (int i = 0; i < 64; ++i) out[b * 64 + i] = (int16_t)jpeg::quantise(v[i], q[comp][i]);
        }
        FILE* fo = fopen(argv[5], "wb");
        if (!fo) return 3;
        fwrite(out.data(), sizeof(int16_t), out.size(), fo);
        fclose(fo);
        return 0;
    }
    if (mode == "header" && argc == 6) {
        uint8_t h[kJpegHeaderBytes];
        jpeg_build_header(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), h);
        FILE* fo = fopen(argv[5], "wb");
        if (!fo) return 3;
        fwrite(h, 1, sizeof(h), fo);
        fclose(fo);
        return 0;
    }
    if (mode == "bound" && argc == 3) {
        printf("%zu\n", jpeg::interval_max_bytes(atoi(argv[2])));
        return 0;
    }
    return 2;
}
