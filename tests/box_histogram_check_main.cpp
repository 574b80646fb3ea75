// CPU check of csrc/box_histogram_check.cpp: the refusals of pa_box_histograms.  Stand-alone (own main, plain g++); exit status 0 =
// all checks hold, otherwise one line per failed check.  Driven by tests/test_identity_host.py, also under
// -fsanitize=address,undefined.  "check n h w k frame x0 y0 x1 y1 ..." (5 k numbers; k < 0 is passed on with no list, "null" in
// place of the numbers passes a NULL list) prints the reason or "ok".
#include "activity_check.h"
#include "box_histogram_check.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace padel;

extern "C" const char* pa_box_histograms_check(int n, int h, int w, const int32_t* rects, int k);

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) { ++failures; printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static bool refused(int n, int h, int w, const int32_t* rects, int k, const char* word) {
    std::string why;
    if (!box_hist_validate(n, h, w, rects, k, why)) return false;
    const char* c = pa_box_histograms_check(n, h, w, rects, k);
    return c && why == c && why.find(word) != std::string::npos;
}

int main(int argc, char** argv) {
    if (argc >= 6 && !strcmp(argv[1], "check")) {
        const int n = atoi(argv[2]), h = atoi(argv[3]), w = atoi(argv[4]), k = atoi(argv[5]);
        std::vector<int32_t> rects;
        const bool null = argc == 7 && !strcmp(argv[6], "null");
        if (!null) {
            if (argc != 6 + 5 * (k > 0 ? k : 0)) { printf("usage: check n h w k, then 5 numbers per rectangle\n"); return 2; }
            for (int i = 6; i < argc; ++i) rects.push_back(atoi(argv[i]));
        }
        const char* why = pa_box_histograms_check(n, h, w, rects.empty() ? nullptr : rects.data(), k);
        printf("%s\n", why ? why : "ok");
        return 0;
    }
    std::string why;
    const int32_t good[][5] = {{0, 0, 0, 7, 5}, {1, 6, 4, 7, 5}, {1, 0, 0, 1, 1}, {0, 0, 0, 7, 5}};
    CHECK(!box_hist_validate(2, 5, 7, &good[0][0], 4, why) && !pa_box_histograms_check(2, 5, 7, &good[0][0], 4), "plain call refused");
    CHECK(!box_hist_validate(2, 5, 7, nullptr, 0, why) && !box_hist_validate(2, 5, 7, &good[0][0], 0, why), "k = 0 refused");
    const int32_t corner[5] = {kActivityMaxFrames - 1, kActivityMaxSide - 1, kActivityMaxSide - 1, kActivityMaxSide, kActivityMaxSide};
    CHECK(!box_hist_validate(kActivityMaxFrames, kActivityMaxSide, kActivityMaxSide, corner, 1, why), "the limits themselves refused");
    std::vector<int32_t> many((size_t)5 * kBoxHistMaxRects);
    for (int j = 0; j < kBoxHistMaxRects; ++j) { int32_t* r = &many[5 * (size_t)j]; r[0] = j & 1; r[1] = 0; r[2] = 0; r[3] = 7; r[4] = 5; }
    CHECK(!box_hist_validate(2, 5, 7, many.data(), kBoxHistMaxRects, why), "the most rectangles refused");
    CHECK(refused(0, 5, 7, &good[0][0], 1, "n = 0") && refused(kActivityMaxFrames + 1, 5, 7, &good[0][0], 1, "n = "), "n out of range accepted");
    CHECK(refused(2, 0, 7, &good[0][0], 1, "width and height") && refused(2, 5, -1, &good[0][0], 1, "width and height") &&
          refused(2, kActivityMaxSide + 1, 7, &good[0][0], 1, "width and height"), "geometry out of range accepted");
    CHECK(refused(2, 5, 7, &good[0][0], -1, "k = -1") && refused(2, 5, 7, &good[0][0], kBoxHistMaxRects + 1, "k = "), "k out of range accepted");
    CHECK(refused(2, 5, 7, nullptr, 1, "NULL"), "a NULL list of one rectangle accepted");
    const int32_t frames[][5] = {{-1, 0, 0, 7, 5}, {2, 0, 0, 7, 5}};
    for (const auto& r : frames) CHECK(refused(2, 5, 7, r, 1, "names frame"), "frame %d accepted", r[0]);
    const int32_t bad[][5] = {{0, 0, 0, 8, 5}, {0, 0, 0, 7, 6}, {0, -1, 0, 7, 5}, {0, 0, -1, 7, 5}, {0, 3, 0, 3, 5}, {0, 0, 4, 7, 4}, {0, 5, 0, 4, 5}};
    for (const auto& r : bad) CHECK(refused(2, 5, 7, r, 1, "is empty or leaves"), "rectangle (%d, %d, %d, %d) accepted", r[1], r[2], r[3], r[4]);
    // the first offending rectangle is named, the ones before it are fine
    int32_t list[3][5] = {{0, 0, 0, 7, 5}, {1, 6, 4, 7, 5}, {1, 6, 4, 8, 5}};
    CHECK(refused(2, 5, 7, &list[0][0], 3, "rectangle 2 ") && !box_hist_validate(2, 5, 7, &list[0][0], 2, why), "the third rectangle's fault not found");
    if (!failures) printf("ok\n");
    return failures ? 1 : 0;
}
