// Stand-alone harness (host only: g++, no HIP, no engine library) over csrc/render_marks.h and csrc/render_check.cpp for PA_MARK_ARC, the
// elliptical ring cut to octants: mark_covers and mark_bbox are the functions the render kernel culls and covers by.
//   render_arc_main cover X0 Y0 W H marks.bin out.bin boxes.bin
//       marks.bin: pa_mark records.  Every mark is checked (render_validate), resolved (render_resolve_marks) and evaluated with
//       mark_covers at the pixels X0 <= x < X0 + W, Y0 <= y < Y0 + H (0 <= x, y < 8192): out.bin receives W * H bytes (0 / 1, row-major)
//       per mark, boxes.bin its mark_bbox as 4 x int32 (x0, y0, x1, y1).  A pixel covered outside mark_bbox — the box the kernel culls
//       by — ends the run with status 2; a mark the checks refuse with status 3 and the reason on stderr.
//   render_arc_main check marks.bin      -> "ok", or the reason the checks refuse the list (one frame of 64 x 64), status 0 either way
#include "render_check.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace padel;

static std::vector<pa_mark> read_marks(const char* path) {
    std::vector<pa_mark> marks;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(1); }
    pa_mark m;
    while (fread(&m, sizeof(m), 1, f) == 1) marks.push_back(m);
    fclose(f);
    return marks;
}

static int cover(int x0, int y0, int w, int h, const char* in_path, const char* out_path, const char* box_path) {
    if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || x0 + w > kRenderMaxSide || y0 + h > kRenderMaxSide) {
        fprintf(stderr, "the window leaves [0, %d)\n", kRenderMaxSide);
        return 1;
    }
    const std::vector<pa_mark> marks = read_marks(in_path);
    FILE* fo = fopen(out_path, "wb");
    FILE* fb = fopen(box_path, "wb");
    if (!fo || !fb) { fprintf(stderr, "cannot open %s or %s\n", out_path, box_path); return 1; }
    int status = 0;
    std::vector<unsigned char> plane((size_t)w * h);
    for (size_t k = 0; k < marks.size() && !status; ++k) {
        const int32_t first[2] = {0, 1};
        std::string why;
        size_t span = 0;
        if (render_validate(1, y0 + h, x0 + w, &marks[k], first, PA_RENDER_BGR, nullptr, nullptr, &span, why)) {
            fprintf(stderr, "mark %zu refused: %s\n", k, why.c_str());
            status = 3;
            break;
        }
        pa_mark r;
        render_resolve_marks(&marks[k], &r, 1);
        const MarkBox b = mark_bbox(r);
        const int32_t box[4] = {b.x0, b.y0, b.x1, b.y1};
        fwrite(box, sizeof(box), 1, fb);
        for (int y = 0; y < h && !status; ++y)
            for (int x = 0; x < w; ++x) {
                const bool c = mark_covers(r, x0 + x, y0 + y);
                if (c && !mark_box_meets(b, x0 + x, y0 + y, x0 + x, y0 + y)) {
                    fprintf(stderr, "mark %zu covers (%d, %d) outside its bounding box [%d, %d] x [%d, %d]\n", k, x0 + x, y0 + y, b.x0, b.x1, b.y0, b.y1);
                    status = 2;
                    break;
                }
                plane[(size_t)y * w + x] = c ? 1 : 0;
            }
        if (!status) fwrite(plane.data(), 1, plane.size(), fo);
    }
    fclose(fo);
    fclose(fb);
    if (!status) printf("%zu marks\n", marks.size());
    return status;
}

int main(int argc, char** argv) {
    if (argc == 9 && !strcmp(argv[1], "cover"))
        return cover(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), argv[6], argv[7], argv[8]);
    if (argc == 3 && !strcmp(argv[1], "check")) {
        const std::vector<pa_mark> marks = read_marks(argv[2]);
        const int32_t first[2] = {0, (int32_t)marks.size()};
        std::string why;
        size_t span = 0;
        printf("%s\n", render_validate(1, 64, 64, marks.data(), first, PA_RENDER_BGR, nullptr, nullptr, &span, why) ? why.c_str() : "ok");
        return 0;
    }
    fprintf(stderr, "usage: render_arc_main cover X0 Y0 W H marks.bin out.bin boxes.bin | check marks.bin\n");
    return 1;
}
