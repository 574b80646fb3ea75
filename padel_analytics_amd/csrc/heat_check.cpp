// What is decided about a pa_heat_accumulate call before anything runs: host-only code (no HIP at all), built with g++ like
// warp_check.cpp, so that the same refusals are available without a GPU (pa_heat_check, tests/heat_main.cpp).
#include "heat_check.h"
#include "heat_math.h"

#include <cstdio>

namespace padel {

#define FAIL(...)                                                \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        err = _b;                                                \
        return 1;                                                \
    } while (0)

int heat_validate(int n, int oh, int ow, int planes, const int32_t* pts, const int32_t* first, const int32_t* valid, int r, uint32_t full,
                  int alpha, int show_mask, const uint8_t* lut, const void* canvas, const void* state, std::string& err) {
    if (n < 1) FAIL("pa_heat_accumulate: n = %d, at least one frame is needed", n);
    if (oh < 1 || oh > kHeatMaxDim) FAIL("pa_heat_accumulate: oh = %d outside [1, %d]", oh, kHeatMaxDim);
    if (ow < 1 || ow > kHeatMaxDim) FAIL("pa_heat_accumulate: ow = %d outside [1, %d]", ow, kHeatMaxDim);
    if (planes < 1 || planes > kHeatMaxPlanes) FAIL("pa_heat_accumulate: planes = %d outside [1, %d]", planes, kHeatMaxPlanes);
    if (r < 1 || r > kHeatMaxRadius) FAIL("pa_heat_accumulate: r = %d outside [1, %d]", r, kHeatMaxRadius);
    if (full < 1 || full > kHeatMaxFull) FAIL("pa_heat_accumulate: full = %u outside [1, %u]", full, kHeatMaxFull);
    if (alpha < 0 || alpha > 256) FAIL("pa_heat_accumulate: alpha = %d outside [0, 256]", alpha);
    if (show_mask < 1 || show_mask >= (1 << planes))
        FAIL("pa_heat_accumulate: show_mask = %d names no plane or one at or above planes = %d", show_mask, planes);
    if (!canvas || !state || !first || !valid || !lut) FAIL("pa_heat_accumulate: the canvases, the state, first, valid or the lut is NULL");
    if (first[0] != 0) FAIL("pa_heat_accumulate: first[0] = %d, it must be 0", first[0]);
    for (int i = 0; i < n; ++i)
        if (first[i + 1] < first[i]) FAIL("pa_heat_accumulate: first[%d] = %d is below first[%d] = %d", i + 1, first[i + 1], i, first[i]);
    for (int i = 0; i < n; ++i)
        if (first[i + 1] - first[i] > kHeatMaxPoints)
            FAIL("pa_heat_accumulate: frame %d has %d points, at most %d are taken", i, first[i + 1] - first[i], kHeatMaxPoints);
    if (first[n] > 0 && !pts) FAIL("pa_heat_accumulate: first[] announces %d points and the points are NULL", first[n]);
    for (int i = 0; i < n; ++i)
        for (int k = first[i]; k < first[i + 1]; ++k) {
            const int32_t x = pts[3 * (size_t)k], y = pts[3 * (size_t)k + 1], p = pts[3 * (size_t)k + 2];
            if (x < -kHeatMaxCoord || x > kHeatMaxCoord || y < -kHeatMaxCoord || y > kHeatMaxCoord || p < 0 || p >= planes)
                FAIL("pa_heat_accumulate: point %d (frame %d) is (%d, %d) on plane %d: beyond +/-%d or no plane of %d", k, i, x, y, p,
                     kHeatMaxCoord, planes);
        }
    for (int i = 0; i < n; ++i)
        if (!valid[i] && first[i + 1] > first[i])
            FAIL("pa_heat_accumulate: frame %d is not valid and carries %d points", i, first[i + 1] - first[i]);
    const uintptr_t c = reinterpret_cast<uintptr_t>(canvas), s = reinterpret_cast<uintptr_t>(state);
    const size_t canvas_bytes = (size_t)n * oh * ow * 3, state_bytes = (size_t)planes * oh * ow * sizeof(uint32_t);
    if (c < s + state_bytes && s < c + canvas_bytes) FAIL("pa_heat_accumulate: the state overlaps the canvases");
    return 0;
}

}  // namespace padel

extern "C" int pa_heat_check(int n, int oh, int ow, int planes, const int32_t* pts, const int32_t* first, const int32_t* valid, int r,
                             uint32_t full, int alpha, int show_mask, const uint8_t* lut, const void* canvas, const void* state,
                             char* why, size_t cap) {
    std::string err;
    const int rc = padel::heat_validate(n, oh, ow, planes, pts, first, valid, r, full, alpha, show_mask, lut, canvas, state, err);
    if (why && cap) snprintf(why, cap, "%s", rc ? err.c_str() : "");
    return rc;
}
