// pa_warp_perspective (include/padel_hip.h): n packed BGR frames of h x w -> n packed BGR frames of oh x ow, each through its own
// 3 x 3 matrix canvas -> source, bilinear with weights in 1 / 32 pixel.  The arithmetic of a pixel is warp_math.h, shared with the
// host; this file is compiled with -ffp-contract=off (build.sh) so that the device rounds every product and sum as the host does.
//
// Shape.  One thread makes kPx consecutive pixels of one canvas row; the threads of a workgroup take consecutive runs, so that a
// wave reads a stretch of a few source rows and writes one contiguous stretch of the canvas.  Nothing is staged in LDS: the four
// taps of neighbouring pixels fall into the same cache lines, and under minification (the far end of the court) there is no reuse
// to stage for.
//   vector path (ow % 16 == 0, dst 16-byte aligned): kPx = 16, i.e. 48 bytes, packed in registers and stored as three 16-byte words;
//   byte path (everything else): kPx = 1, three byte stores.
// A launch covers at most kWarpMaxBlocksX x 256 threads per frame and at most 65535 frames at once; what is left is walked by the
// grid-stride loops.  Registers and occupancy: DESIGN.md §3.3.8 (no scratch, no LDS).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "warp_math.h"

namespace padel {

constexpr unsigned kWarpMaxBlocksX = 2048;
constexpr int kWarpVecPx = 16;

template <bool kVec>
__global__ void __launch_bounds__(256) warp_kernel(const WarpArgs a) {
    constexpr int kPx = kVec ? kWarpVecPx : 1;
    const unsigned per_row = (unsigned)a.ow / kPx;                    // (vector path: ow is a multiple of kPx)
    const unsigned per_frame = (unsigned)a.oh * per_row;              // at most 4096 * 4096
    for (int i = (int)blockIdx.y; i < a.n; i += (int)gridDim.y) {
        const uint8_t* const frame = a.src + (size_t)i * a.h * a.w * 3;
        const int valid = a.valid[i];
        double m[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = a.m[9 * (size_t)i + k];
        for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < per_frame; t += gridDim.x * 256u) {
            const int v = (int)(t / per_row), u0 = (int)(t % per_row) * kPx;
            uint8_t* const out = a.dst + (((size_t)i * a.oh + v) * a.ow + u0) * 3;
            if constexpr (!kVec) {
                const uint32_t p = warp_pixel(frame, a.h, a.w, m, valid, u0, v, a.fill);
                out[0] = (uint8_t)p; out[1] = (uint8_t)(p >> 8); out[2] = (uint8_t)(p >> 16);
            } else {
                uint32_t wd[3 * kPx / 4];
#pragma unroll
                for (int k = 0; k < kPx / 4; ++k) {                       // four pixels are three dwords
                    const uint32_t p0 = warp_pixel(frame, a.h, a.w, m, valid, u0 + 4 * k, v, a.fill);
                    const uint32_t p1 = warp_pixel(frame, a.h, a.w, m, valid, u0 + 4 * k + 1, v, a.fill);
                    const uint32_t p2 = warp_pixel(frame, a.h, a.w, m, valid, u0 + 4 * k + 2, v, a.fill);
                    const uint32_t p3 = warp_pixel(frame, a.h, a.w, m, valid, u0 + 4 * k + 3, v, a.fill);
                    wd[3 * k] = p0 | p1 << 24;
                    wd[3 * k + 1] = p1 >> 8 | p2 << 16;
                    wd[3 * k + 2] = p2 >> 16 | p3 << 8;
                }
                uint4* const o4 = reinterpret_cast<uint4*>(out);          // 16-byte aligned: dst is, and 3 ow and 3 u0 are multiples of 48
#pragma unroll
                for (int k = 0; k < 3; ++k) o4[k] = make_uint4(wd[4 * k], wd[4 * k + 1], wd[4 * k + 2], wd[4 * k + 3]);
            }
        }
    }
}

bool warp_vector_path_ok(const WarpArgs& a) {
    return a.ow % kWarpVecPx == 0 && reinterpret_cast<uintptr_t>(a.dst) % 16 == 0;
}

hipError_t launch_warp(const WarpArgs& a, hipStream_t s, int* vec_out) {
    const bool vec = warp_vector_path_ok(a);
    const unsigned per_frame = (unsigned)a.oh * ((unsigned)a.ow / (vec ? kWarpVecPx : 1));
    const dim3 grid(std::min((per_frame + 255u) / 256u, kWarpMaxBlocksX), (unsigned)std::min(a.n, 65535)), block(256);
    if (vec) hipLaunchKernelGGL((warp_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((warp_kernel<false>), grid, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess && vec_out) *vec_out = vec ? 1 : 0;
    return e;
}

}  // namespace padel
