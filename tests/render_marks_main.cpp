// Stand-alone harness (host only: g++, no HIP, no engine library) over csrc/render_marks.h and csrc/render_check.cpp — the code the
// render kernel applies to its pixel registers and the checks pa_render makes before it launches.
//   render_marks_main cover W H marks.bin out.bin
//       marks.bin: pa_mark records.  Every mark is checked (render_validate), resolved (render_resolve_marks) and evaluated with
//       mark_covers at every pixel of a W x H frame: out.bin receives W * H bytes (0 / 1, row-major) per mark.  A pixel covered outside
//       mark_bbox — the box the kernel culls by — ends the run with status 2; a mark the checks refuse with status 3.
//   render_marks_main glyph CODE        -> the 7 rows of the glyph as text ('#' / '.'), or "none"
#include "render_check.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace padel;

static int cover(int w, int h, const char* in_path, const char* out_path) {
    FILE* fi = fopen(in_path, "rb");
    if (!fi) { fprintf(stderr, "cannot open %s\n", in_path); return 1; }
    std::vector<pa_mark> marks;
    pa_mark m;
    while (fread(&m, sizeof(m), 1, fi) == 1) marks.push_back(m);
    fclose(fi);
    FILE* fo = fopen(out_path, "wb");
    if (!fo) { fprintf(stderr, "cannot open %s\n", out_path); return 1; }
    std::vector<unsigned char> plane((size_t)w * h);
    for (size_t k = 0; k < marks.size(); ++k) {
        const int32_t first[2] = {0, 1};
        std::string why;
        size_t span = 0;
        if (render_validate(1, h, w, &marks[k], first, PA_RENDER_BGR, nullptr, nullptr, &span, why)) {
            fprintf(stderr, "mark %zu refused: %s\n", k, why.c_str());
            fclose(fo);
            return 3;
        }
        pa_mark r;
        render_resolve_marks(&marks[k], &r, 1);
        const MarkBox b = mark_bbox(r);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const bool c = mark_covers(r, x, y);
                if (c && !mark_box_meets(b, x, y, x, y)) {
                    fprintf(stderr, "mark %zu covers (%d, %d) outside its bounding box [%d, %d] x [%d, %d]\n", k, x, y, b.x0, b.x1, b.y0, b.y1);
                    fclose(fo);
                    return 2;
                }
                plane[(size_t)y * w + x] = c ? 1 : 0;
            }
        fwrite(plane.data(), 1, plane.size(), fo);
    }
    fclose(fo);
    printf("%zu marks\n", marks.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "cover")) return cover(atoi(argv[2]), atoi(argv[3]), argv[4], argv[5]);
    if (argc == 3 && !strcmp(argv[1], "glyph")) {
        uint8_t rows[kGlyphH];
        if (glyph_rows(atoi(argv[2]), rows)) { printf("none\n"); return 0; }
        for (int j = 0; j < kGlyphH; ++j) {
            for (int i = 0; i < kGlyphW; ++i) putchar((rows[j] >> i) & 1 ? '#' : '.');
            putchar('\n');
        }
        return 0;
    }
    fprintf(stderr, "usage: render_marks_main cover W H marks.bin out.bin | glyph CODE\n");
    return 1;
}
