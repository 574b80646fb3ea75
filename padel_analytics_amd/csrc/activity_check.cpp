// What is decided about a pa_frame_activity call before anything runs: host-only code (no HIP runtime call), built with g++ like
// render_check.cpp, so that the same refusals are available without a GPU (pa_frame_activity_check, tests/activity_check_main.cpp).
#include "activity_check.h"

#include <algorithm>
#include <cstdio>

namespace padel {

#define FAIL(...)                                                \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        err = _b;                                                \
        return 1;                                                \
    } while (0)

int activity_validate(int n, int h, int w, const int32_t* roi, int tau, std::string& err) {
    if (n < 1 || n > kActivityMaxFrames) FAIL("pa_frame_activity: n = %d frames outside [1, %d]", n, kActivityMaxFrames);
    if (w < 1 || h < 1 || w > kActivityMaxSide || h > kActivityMaxSide)
        FAIL("pa_frame_activity: %d x %d frames: width and height must lie in [1, %d]", w, h, kActivityMaxSide);
    if (roi && !(0 <= roi[0] && roi[0] < roi[2] && roi[2] <= w && 0 <= roi[1] && roi[1] < roi[3] && roi[3] <= h))
        FAIL("pa_frame_activity: roi (%d, %d, %d, %d) is empty or leaves the %d x %d frame (x0, y0, x1, y1, half-open)", roi[0], roi[1],
             roi[2], roi[3], w, h);
    if (tau < 0 || tau > 255) FAIL("pa_frame_activity: tau = %d outside [0, 255]", tau);
    return 0;
}

int activity_band_rows(int roi_w, int roi_h) {
    return std::max(1, std::min(roi_h, kActivityBandPixels / std::max(roi_w, 1)));
}

}  // namespace padel

extern "C" const char* pa_frame_activity_check(int n, int h, int w, const int32_t* roi, int tau) {
    static thread_local std::string why;
    return padel::activity_validate(n, h, w, roi, tau, why) ? why.c_str() : nullptr;
}
