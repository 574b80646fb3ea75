// Stand-alone program over csrc/heat_math.h and csrc/heat_check.cpp (g++, no HIP): the host side of pa_heat_accumulate.  Reads a
// case file (argv[1]) and writes to stdout what tests/test_heatmap_host.py compares with heatmap.accumulate_host bit for bit.  A case
// in the file, little endian:
//     int32 n, oh, ow, planes, r, alpha, show_mask, npts; uint32 full; 768 lut bytes; (n + 1) x int32 first; n x int32 valid;
//     npts x 3 int32 points; planes x oh x ow uint32 state; n x oh x ow x 3 canvas bytes
// and on stdout:  int32 0, the canvas bytes and the state, or int32 1, int32 length and the words of the refusal.
// Every buffer is allocated at its exact size, so that under -fsanitize=address an access outside a map or a canvas is an error.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "heat_check.h"
#include "heat_math.h"

static bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: heat_main CASES\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[8];
    while (fread(head, sizeof(int32_t), 8, f) == 8) {
        const int n = head[0], oh = head[1], ow = head[2], planes = head[3], r = head[4], alpha = head[5], show_mask = head[6], npts = head[7];
        uint32_t full = 0;
        if (!get(f, &full, 4) || n < 0 || oh < 0 || ow < 0 || planes < 0 || npts < 0) { fprintf(stderr, "bad case header\n"); return 2; }
        std::vector<uint8_t> lut(768);
        std::vector<int32_t> first((size_t)n + 1), valid((size_t)n), pts((size_t)npts * 3);
        std::vector<uint32_t> state((size_t)planes * oh * ow);
        std::vector<uint8_t> canvas((size_t)n * oh * ow * 3);
        if (!get(f, lut.data(), 768) || !get(f, first.data(), first.size() * 4) || !get(f, valid.data(), valid.size() * 4) ||
            !get(f, pts.data(), pts.size() * 4) || !get(f, state.data(), state.size() * 4) || !get(f, canvas.data(), canvas.size())) {
            fprintf(stderr, "short case\n");
            return 2;
        }
        std::string why;
        // (an empty vector has no address: the check looks at n and the sizes before it looks at the pointers)
        const int32_t refused = padel::heat_validate(n, oh, ow, planes, pts.empty() ? nullptr : pts.data(), first.data(), valid.data(), r, full,
                                                     alpha, show_mask, lut.data(), canvas.empty() ? (const void*)&head : canvas.data(),
                                                     state.empty() ? (const void*)&full : state.data(), why);
        fwrite(&refused, 4, 1, stdout);
        if (refused) {
            const int32_t len = (int32_t)why.size();
            fwrite(&len, 4, 1, stdout);
            fwrite(why.data(), 1, why.size(), stdout);
            continue;
        }
        const size_t plane_px = (size_t)oh * ow;
        for (int i = 0; i < n; ++i) {
            if (!valid[i]) continue;
            for (int v = 0; v < oh; ++v)
                for (int u = 0; u < ow; ++u) {
                    const size_t px = (size_t)v * ow + u;
                    for (int k = first[i]; k < first[i + 1]; ++k) {
                        uint32_t& d = state[pts[3 * (size_t)k + 2] * plane_px + px];
                        d = padel::heat_add(d, padel::heat_splat(u - pts[3 * (size_t)k], v - pts[3 * (size_t)k + 1], r));
                    }
                    uint32_t shown = 0;
                    for (int p = 0; p < planes; ++p)
                        if ((show_mask >> p) & 1) shown = padel::heat_add(shown, state[p * plane_px + px]);
                    uint8_t* const o = canvas.data() + ((size_t)i * plane_px + px) * 3;
                    const uint32_t q = padel::heat_pixel((uint32_t)o[0] | (uint32_t)o[1] << 8 | (uint32_t)o[2] << 16, shown, full, alpha, lut.data());
                    o[0] = (uint8_t)q; o[1] = (uint8_t)(q >> 8); o[2] = (uint8_t)(q >> 16);
                }
        }
        fwrite(canvas.data(), 1, canvas.size(), stdout);
        fwrite(state.data(), 4, state.size(), stdout);
    }
    fclose(f);
    return 0;
}
