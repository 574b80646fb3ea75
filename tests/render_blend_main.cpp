// Stand-alone harness (host only: g++, no HIP, no engine library) over csrc/render_marks.h and csrc/render_check.cpp for the one mark
// that is not opaque, PA_MARK_BLEND: mark_apply is the function the render kernel calls on a covered pixel register.
//   render_blend_main apply A out.bin
//       weight A: for every pair (p, c) in 0..255 x 0..255 (p outer) the pixel  p | (255 - p) << 8 | (p ^ 0x55) << 16  under a blend
//       mark of colour  c | (255 - c) << 8 | (c ^ 0xaa) << 16  -> 3 bytes B G R per pair (the three channels carry different values, so
//       a carry from one channel into the next would show).  Status 3 when the checks refuse the mark (a weight outside 1..255).
//   render_blend_main draw W H marks.bin in.bin out.bin
//       the marks applied in list order to one W x H packed BGR frame the way the kernel applies them — render_validate,
//       render_resolve_marks, reject by mark_bbox, mark_covers, mark_apply.  Status 3 with the reason on stderr when a mark is refused.
//   render_blend_main check marks.bin      -> "ok", or the reason the checks refuse the list (one frame of 64 x 64), status 0 either way
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

static int validate(const std::vector<pa_mark>& marks, int w, int h, std::string& why) {
    const int32_t first[2] = {0, (int32_t)marks.size()};
    size_t span = 0;
    return render_validate(1, h, w, marks.data(), first, PA_RENDER_BGR, nullptr, nullptr, &span, why);
}

static int apply(int a, const char* out_path) {
    pa_mark m = {};
    m.kind = PA_MARK_BLEND;
    m.x1 = m.y1 = 3;
    m.arg = a;
    std::vector<unsigned char> out;
    out.reserve(256 * 256 * 3);
    for (unsigned p = 0; p < 256; ++p)
        for (unsigned c = 0; c < 256; ++c) {
            m.bgr = c | ((255u - c) << 8) | ((c ^ 0xaau) << 16);
            if (p == 0 && c == 0) {
                std::string why;
                if (validate({m}, 8, 8, why)) { fprintf(stderr, "%s\n", why.c_str()); return 3; }
            }
            const unsigned q = mark_apply(m, p | ((255u - p) << 8) | ((p ^ 0x55u) << 16));
            out.push_back((unsigned char)q);
            out.push_back((unsigned char)(q >> 8));
            out.push_back((unsigned char)(q >> 16));
            if (q >> 24) { fprintf(stderr, "bits above the pixel's 24 at p %u c %u\n", p, c); return 2; }
        }
    FILE* fo = fopen(out_path, "wb");
    if (!fo) { fprintf(stderr, "cannot open %s\n", out_path); return 1; }
    fwrite(out.data(), 1, out.size(), fo);
    fclose(fo);
    return 0;
}

static int draw(int w, int h, const char* marks_path, const char* in_path, const char* out_path) {
    const std::vector<pa_mark> marks = read_marks(marks_path);
    std::string why;
    if (validate(marks, w, h, why)) { fprintf(stderr, "%s\n", why.c_str()); return 3; }
    std::vector<unsigned char> frame((size_t)w * h * 3);
    FILE* fi = fopen(in_path, "rb");
    if (!fi || fread(frame.data(), 1, frame.size(), fi) != frame.size()) { fprintf(stderr, "cannot read %s\n", in_path); return 1; }
    fclose(fi);
    std::vector<pa_mark> resolved(marks.size());
    render_resolve_marks(marks.data(), resolved.data(), marks.size());
    for (const pa_mark& m : resolved) {
        const MarkBox b = mark_bbox(m);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                if (!mark_box_meets(b, x, y, x, y) || !mark_covers(m, x, y)) continue;
                unsigned char* q = &frame[((size_t)y * w + x) * 3];
                const unsigned p = mark_apply(m, (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16));
                q[0] = (unsigned char)p; q[1] = (unsigned char)(p >> 8); q[2] = (unsigned char)(p >> 16);
            }
    }
    FILE* fo = fopen(out_path, "wb");
    if (!fo) { fprintf(stderr, "cannot open %s\n", out_path); return 1; }
    fwrite(frame.data(), 1, frame.size(), fo);
    fclose(fo);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "apply")) return apply(atoi(argv[2]), argv[3]);
    if (argc == 7 && !strcmp(argv[1], "draw")) return draw(atoi(argv[2]), atoi(argv[3]), argv[4], argv[5], argv[6]);
    if (argc == 3 && !strcmp(argv[1], "check")) {
        std::string why;
        printf("%s\n", validate(read_marks(argv[2]), 64, 64, why) ? why.c_str() : "ok");
        return 0;
    }
    fprintf(stderr, "usage: render_blend_main apply A out.bin | draw W H marks.bin in.bin out.bin | check marks.bin\n");
    return 1;
}
