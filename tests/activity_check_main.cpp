// CPU check of csrc/activity_check.cpp: the refusals of pa_frame_activity and how a launch is cut into bands.  Stand-alone (own main,
// plain g++); exit status 0 = all checks hold, otherwise one line per failed check.  Driven by tests/test_frame_activity_host.py,
// also under -fsanitize=address,undefined.  "check n h w x0 y0 x1 y1 tau" (x0 < 0: no roi) prints the reason or "ok".
#include "activity_check.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace padel;

extern "C" const char* pa_frame_activity_check(int n, int h, int w, const int32_t* roi, int tau);

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) { ++failures; printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static bool refused(int n, int h, int w, const int32_t* roi, int tau, const char* word) {
    std::string why;
    if (!activity_validate(n, h, w, roi, tau, why)) return false;
    const char* c = pa_frame_activity_check(n, h, w, roi, tau);
    return c && why == c && why.find(word) != std::string::npos;
}

int main(int argc, char** argv) {
    if (argc == 10 && !strcmp(argv[1], "check")) {
        int v[8];
        for (int i = 0; i < 8; ++i) v[i] = atoi(argv[2 + i]);
        const int32_t roi[4] = {v[3], v[4], v[5], v[6]};
        const char* why = pa_frame_activity_check(v[0], v[1], v[2], v[3] < 0 ? nullptr : roi, v[7]);
        printf("%s\n", why ? why : "ok");
        return 0;
    }
    std::string why;
    const int32_t whole[4] = {0, 0, 7, 5}, one[4] = {6, 4, 7, 5};
    CHECK(!activity_validate(1, 5, 7, nullptr, 0, why) && !pa_frame_activity_check(1, 5, 7, nullptr, 0), "plain call refused");
    CHECK(!activity_validate(kActivityMaxFrames, kActivityMaxSide, kActivityMaxSide, nullptr, 255, why), "the limits themselves refused");
    CHECK(!activity_validate(2, 5, 7, whole, 24, why) && !activity_validate(2, 5, 7, one, 24, why), "roi inside the frame refused");
    CHECK(refused(0, 5, 7, nullptr, 24, "n = 0") && refused(kActivityMaxFrames + 1, 5, 7, nullptr, 24, "n = "), "n out of range accepted");
    CHECK(refused(1, 0, 7, nullptr, 24, "width and height") && refused(1, 5, -1, nullptr, 24, "width and height") &&
          refused(1, kActivityMaxSide + 1, 7, nullptr, 24, "width and height"), "geometry out of range accepted");
    const int32_t bad[][4] = {{0, 0, 8, 5}, {0, 0, 7, 6}, {-1, 0, 7, 5}, {0, -1, 7, 5}, {3, 0, 3, 5}, {0, 4, 7, 4}, {5, 0, 4, 5}};
    for (const auto& r : bad) CHECK(refused(1, 5, 7, r, 24, "roi"), "roi (%d, %d, %d, %d) accepted", r[0], r[1], r[2], r[3]);
    CHECK(refused(1, 5, 7, nullptr, -1, "tau") && refused(1, 5, 7, nullptr, 256, "tau"), "tau out of range accepted");
    // bands: whole rows, at most kActivityBandPixels pixels unless one row alone is longer; every row in exactly one band
    const int ws[] = {1, 2, 3, 15, 16, 17, 640, 1280, 1920, 8191, 16383, 16384}, hs[] = {1, 2, 7, 12, 13, 360, 720, 16384};
    for (int w : ws)
        for (int h : hs) {
            const int r = activity_band_rows(w, h), b = activity_bands(h, r);
            CHECK(r >= 1 && r <= h, "%d x %d: %d rows per band", w, h, r);
            CHECK((long long)r * w <= kActivityBandPixels || r == 1, "%d x %d: a band of %d rows has more than %d pixels", w, h, r, kActivityBandPixels);
            CHECK((long long)b * r >= h && (long long)(b - 1) * r < h, "%d x %d: %d bands of %d rows do not tile the rows", w, h, b, r);
            CHECK(255ll * r * w < (1ll << 32), "%d x %d: a band's sum can wrap 32 bits", w, h);
        }
    if (!failures) printf("ok\n");
    return failures ? 1 : 0;
}
