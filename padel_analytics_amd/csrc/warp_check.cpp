// What is decided about a pa_warp_perspective call before anything runs: host-only code (no HIP at all), built with g++ like
// render_check.cpp, so that the same refusals are available without a GPU (pa_warp_check, tests/warp_main.cpp).
#include "warp_check.h"
#include "warp_math.h"

#include <cmath>
#include <cstdio>

namespace padel {

#define FAIL(...)                                                \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        err = _b;                                                \
        return 1;                                                \
    } while (0)

int warp_validate(int n, int h, int w, int oh, int ow, const double* m, const int32_t* valid, const void* src, const void* dst,
                  std::string& err) {
    if (n < 1) FAIL("pa_warp_perspective: n = %d, at least one frame is needed", n);
    const int dims[4] = {h, w, oh, ow};
    const char* const names[4] = {"h", "w", "oh", "ow"};
    for (int k = 0; k < 4; ++k)
        if (dims[k] < 1 || dims[k] > kWarpMaxDim) FAIL("pa_warp_perspective: %s = %d outside [1, %d]", names[k], dims[k], kWarpMaxDim);
    if (!src || !dst || !m || !valid) FAIL("pa_warp_perspective: src, dst, the matrices or valid is NULL");
    for (int i = 0; i < n; ++i) {
        if (!valid[i]) continue;
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(m[9 * (size_t)i + k])) FAIL("pa_warp_perspective: entry %d of frame %d's matrix is not finite", k, i);
    }
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    const size_t src_bytes = (size_t)n * h * w * 3, dst_bytes = (size_t)n * oh * ow * 3;
    if (s < d + dst_bytes && d < s + src_bytes) FAIL("pa_warp_perspective: dst overlaps src (the warp is not in place)");
    return 0;
}

}  // namespace padel

extern "C" int pa_warp_check(int n, int h, int w, int oh, int ow, const double* m, const int32_t* valid, const void* src, const void* dst,
                             char* why, size_t cap) {
    std::string err;
    const int rc = padel::warp_validate(n, h, w, oh, ow, m, valid, src, dst, err);
    if (why && cap) snprintf(why, cap, "%s", rc ? err.c_str() : "");
    return rc;
}
