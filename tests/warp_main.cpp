// Stand-alone program over csrc/warp_math.h and csrc/warp_check.cpp (g++ -ffp-contract=off, no HIP): the host side of
// pa_warp_perspective.  Reads a case file (argv[1]) and writes to stdout what tests/test_warp_host.py compares with
// topdown.warp_host bit for bit.  A case in the file, little endian:
//     int32 n, h, w, oh, ow; uint32 fill; n x 9 doubles; n x int32 valid; n x h x w x 3 bytes
// and on stdout:  int32 0 and the n x oh x ow x 3 canvas bytes, or int32 1, int32 length and the words of the refusal.
// Every buffer is allocated at its exact size, so that under -fsanitize=address a tap outside the frame is an error.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "warp_check.h"
#include "warp_math.h"

static bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: warp_main CASES\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[5];
    while (fread(head, sizeof(int32_t), 5, f) == 5) {
        const int n = head[0], h = head[1], w = head[2], oh = head[3], ow = head[4];
        uint32_t fill = 0;
        if (!get(f, &fill, 4) || n < 0 || h < 0 || w < 0) { fprintf(stderr, "bad case header\n"); return 2; }
        std::vector<double> m((size_t)n * 9);
        std::vector<int32_t> valid((size_t)n);
        std::vector<uint8_t> src((size_t)n * h * w * 3);
        if (!get(f, m.data(), m.size() * 8) || !get(f, valid.data(), valid.size() * 4) || !get(f, src.data(), src.size())) {
            fprintf(stderr, "short case\n");
            return 2;
        }
        const bool sized = oh >= 1 && ow >= 1 && oh <= padel::kWarpMaxDim && ow <= padel::kWarpMaxDim;
        std::vector<uint8_t> dst(sized ? (size_t)n * oh * ow * 3 : 0);
        std::string why;
        // (an empty vector has no address: the check looks at n and the sizes before it looks at the pointers)
        const int32_t refused = padel::warp_validate(n, h, w, oh, ow, m.data(), valid.data(), src.empty() ? (const void*)&head : src.data(),
                                                     dst.empty() ? (const void*)&fill : dst.data(), why);
        fwrite(&refused, 4, 1, stdout);
        if (refused) {
            const int32_t len = (int32_t)why.size();
            fwrite(&len, 4, 1, stdout);
            fwrite(why.data(), 1, why.size(), stdout);
            continue;
        }
        for (int i = 0; i < n; ++i)
            for (int v = 0; v < oh; ++v)
                for (int u = 0; u < ow; ++u) {
                    const uint32_t p = padel::warp_pixel(src.data() + (size_t)i * h * w * 3, h, w, m.data() + 9 * (size_t)i, valid[i], u, v, fill);
                    uint8_t* o = dst.data() + (((size_t)i * oh + v) * ow + u) * 3;
                    o[0] = (uint8_t)p; o[1] = (uint8_t)(p >> 8); o[2] = (uint8_t)(p >> 16);
                }
        fwrite(dst.data(), 1, dst.size(), stdout);
    }
    fclose(f);
    return 0;
}
