// What is decided about a pa_box_histograms call before anything runs: host-only code (no HIP runtime call), built with g++ like
// activity_check.cpp, so that the same refusals are available without a GPU (pa_box_histograms_check,
// tests/box_histogram_check_main.cpp).  The limits on n, h and w are those of pa_frame_activity.
#include "box_histogram_check.h"
#include "activity_check.h"

#include <cstdio>

namespace padel {

#define FAIL(...)                                                \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        err = _b;                                                \
        return 1;                                                \
    } while (0)

int box_hist_validate(int n, int h, int w, const int32_t* rects, int k, std::string& err) {
    if (n < 1 || n > kActivityMaxFrames) FAIL("pa_box_histograms: n = %d frames outside [1, %d]", n, kActivityMaxFrames);
    if (w < 1 || h < 1 || w > kActivityMaxSide || h > kActivityMaxSide)
        FAIL("pa_box_histograms: %d x %d frames: width and height must lie in [1, %d]", w, h, kActivityMaxSide);
    if (k < 0 || k > kBoxHistMaxRects) FAIL("pa_box_histograms: k = %d rectangles outside [0, %d]", k, kBoxHistMaxRects);
    if (k > 0 && !rects) FAIL("%s", kBoxHistNull);
    for (int j = 0; j < k; ++j) {
        const int32_t* r = rects + 5 * j;
        if (r[0] < 0 || r[0] >= n) FAIL("pa_box_histograms: rectangle %d names frame %d, outside [0, %d)", j, r[0], n);
        if (!(0 <= r[1] && r[1] < r[3] && r[3] <= w && 0 <= r[2] && r[2] < r[4] && r[4] <= h))
            FAIL("pa_box_histograms: rectangle %d (%d, %d, %d, %d) is empty or leaves the %d x %d frame (x0, y0, x1, y1, half-open)", j,
                 r[1], r[2], r[3], r[4], w, h);
    }
    return 0;
}

}  // namespace padel

extern "C" const char* pa_box_histograms_check(int n, int h, int w, const int32_t* rects, int k) {
    static thread_local std::string why;
    return padel::box_hist_validate(n, h, w, rects, k, why) ? why.c_str() : nullptr;
}
