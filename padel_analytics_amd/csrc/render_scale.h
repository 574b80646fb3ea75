// The rounding of pa_render_scaled's box average (include/padel_hip.h), for host and device: an output channel is
//     D = (sum of the s x s rendered source channels + s^2 / 2) / s^2        s in 1..4, integer division
// i.e. (sum + 2) >> 2, (sum + 4) / 9, (sum + 8) >> 4.  The divide by 9 is a multiply and a shift: 7282 = ceil(2^16 / 9) and
// 9 * 7282 - 2^16 = 2, so floor(x * 7282 / 2^16) == x / 9 for every x with 2 x < 2^16 — the largest numerator is
// 9 * 255 + 4 = 2299.  tests/render_scale_main.cpp prints the quotient of every possible sum against the plain division.
// No HIP runtime call, no table.
#pragma once

#if defined(__HIPCC__)
#define PA_SCALE_HD __host__ __device__ __forceinline__
#else
#define PA_SCALE_HD inline
#endif

namespace padel {

constexpr int kRenderMaxScale = 4;
constexpr unsigned kScaleNinthMul = 7282, kScaleNinthShift = 16;

template <int S>
PA_SCALE_HD unsigned scale_round(unsigned sum) {
    static_assert(S >= 1 && S <= kRenderMaxScale, "scale 1..4");
    constexpr unsigned bias = (unsigned)(S * S) / 2;
    if (S == 1) return sum;
    if (S == 2) return (sum + bias) >> 2;
    if (S == 3) return ((sum + bias) * kScaleNinthMul) >> kScaleNinthShift;
    return (sum + bias) >> 4;
}

}  // namespace padel
