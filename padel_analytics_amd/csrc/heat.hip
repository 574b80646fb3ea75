// pa_heat_accumulate (include/padel_hip.h): the players' density maps on the top-down canvas, and the maps blended into the n canvases
// of a call, in place.  The arithmetic is heat_math.h, shared with the host; all integer.
//
// Shape.  One thread owns kPx consecutive pixels of one canvas row for ALL n frames of the call: it loads their densities (every
// plane) once, walks the frames in order — add the frame's points, then blend the frame's pixels under the map as it stands — and
// stores the densities once.  The state moves once per call, a canvas pixel is read and written once per frame: 6 bytes per pixel
// per frame, 8 per pixel per plane per call.  No atomics: a pixel has one owner.
//   vector path (ow % 16 == 0, canvases and state 16-byte aligned): kPx = 16, i.e. 48 canvas bytes as three 16-byte words and 64
//   state bytes per plane as four;  byte path (everything else): kPx = 1.
// A frame's points are the same for every lane (scalar loads); a thread looks at them only if its run meets the bounding box of the
// frame's discs (the host's, staged with the points), and at a point's pixels only if its run meets that disc's.  Pixels whose shown
// density is still 0 are neither loaded nor stored.  The planes are a template parameter, so the densities are registers indexed at
// compile time (a point's plane is matched by a wave-uniform branch per plane).  The lut is staged in LDS as one word per level.
// A launch covers at most kHeatMaxBlocks x 256 threads; what is left is walked by the grid-stride loop.  Registers and occupancy:
// DESIGN.md §3.3.9 (no scratch).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "heat_math.h"
#include "kernels.h"

namespace padel {

constexpr unsigned kHeatMaxBlocks = 2048;
constexpr int kHeatVecPx = 16;

template <bool kVec, int kPlanes>
__global__ void __launch_bounds__(256) heat_kernel(const HeatArgs a) {
    constexpr int kPx = kVec ? kHeatVecPx : 1;
    __shared__ uint32_t lut[256];
    lut[threadIdx.x] = a.lut[threadIdx.x];
    __syncthreads();
    const unsigned per_row = (unsigned)a.ow / kPx;                    // (vector path: ow is a multiple of kPx)
    const unsigned total = (unsigned)a.oh * per_row;                  // at most 4096 * 4096
    const size_t plane_px = (size_t)a.oh * a.ow;
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < total; t += gridDim.x * 256u) {
        const int v = (int)(t / per_row), u0 = (int)(t % per_row) * kPx, u1 = u0 + kPx - 1;
        const size_t px = (size_t)v * a.ow + u0;
        uint32_t d[kPlanes][kPx];
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) {
            uint32_t* const s = a.state + p * plane_px + px;
            if constexpr (kVec) {
#pragma unroll
                for (int k = 0; k < kPx / 4; ++k) {
                    const uint4 q = reinterpret_cast<const uint4*>(s)[k];
                    d[p][4 * k] = q.x; d[p][4 * k + 1] = q.y; d[p][4 * k + 2] = q.z; d[p][4 * k + 3] = q.w;
                }
            } else {
                d[p][0] = s[0];
            }
        }
        for (int i = 0; i < a.n; ++i) {
            if (!a.valid[i]) continue;                                    // (the host refused points in such a frame)
            const int32_t* const bb = a.box + 4 * (size_t)i;
            if (v >= bb[1] && v <= bb[3] && u1 >= bb[0] && u0 <= bb[2]) {
                for (int k = a.first[i]; k < a.first[i + 1]; ++k) {
                    const int x = a.pts[3 * (size_t)k], y = a.pts[3 * (size_t)k + 1], pl = a.pts[3 * (size_t)k + 2];
                    const int dy = v - y;
                    if (dy <= -a.r || dy >= a.r || u1 <= x - a.r || u0 >= x + a.r) continue;
                    uint32_t add[kPx];
#pragma unroll
                    for (int j = 0; j < kPx; ++j) add[j] = heat_splat(u0 + j - x, dy, a.r);
#pragma unroll
                    for (int p = 0; p < kPlanes; ++p) {
                        if (pl != p) continue;
#pragma unroll
                        for (int j = 0; j < kPx; ++j) d[p][j] = heat_add(d[p][j], add[j]);
                    }
                }
            }
            if (a.alpha == 0) continue;
            uint32_t shown[kPx], any = 0;
#pragma unroll
            for (int j = 0; j < kPx; ++j) shown[j] = 0;
#pragma unroll
            for (int p = 0; p < kPlanes; ++p) {
                if (!((a.show_mask >> p) & 1)) continue;
#pragma unroll
                for (int j = 0; j < kPx; ++j) shown[j] = heat_add(shown[j], d[p][j]);
            }
#pragma unroll
            for (int j = 0; j < kPx; ++j) any |= shown[j];
            if (!any) continue;                                           // level 0 has weight 0: the pixels stay
            uint8_t* const out = a.canvas + ((size_t)i * plane_px + px) * 3;
            if constexpr (!kVec) {
                const uint32_t level = heat_level(shown[0], a.full), w = heat_weight(level, a.alpha);
                if (w) {
                    const uint32_t q = heat_blend((uint32_t)out[0] | (uint32_t)out[1] << 8 | (uint32_t)out[2] << 16, lut[level], w);
                    out[0] = (uint8_t)q; out[1] = (uint8_t)(q >> 8); out[2] = (uint8_t)(q >> 16);
                }
            } else {
                uint4* const o4 = reinterpret_cast<uint4*>(out);          // 16-byte aligned: the canvases are, and 3 ow and 3 u0 are multiples of 48
                uint32_t wd[3 * kPx / 4];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint4 q = o4[k];
                    wd[4 * k] = q.x; wd[4 * k + 1] = q.y; wd[4 * k + 2] = q.z; wd[4 * k + 3] = q.w;
                }
#pragma unroll
                for (int k = 0; k < kPx / 4; ++k) {                       // four pixels are three dwords
                    uint32_t p4[4] = {wd[3 * k] & 0xffffffu, wd[3 * k] >> 24 | (wd[3 * k + 1] & 0xffffu) << 8,
                                      wd[3 * k + 1] >> 16 | (wd[3 * k + 2] & 0xffu) << 16, wd[3 * k + 2] >> 8};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t level = heat_level(shown[4 * k + j], a.full), w = heat_weight(level, a.alpha);
                        if (w) p4[j] = heat_blend(p4[j], lut[level], w);
                    }
                    wd[3 * k] = p4[0] | p4[1] << 24;
                    wd[3 * k + 1] = p4[1] >> 8 | p4[2] << 16;
                    wd[3 * k + 2] = p4[2] >> 16 | p4[3] << 8;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) o4[k] = make_uint4(wd[4 * k], wd[4 * k + 1], wd[4 * k + 2], wd[4 * k + 3]);
            }
        }
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) {
            uint32_t* const s = a.state + p * plane_px + px;
            if constexpr (kVec) {
#pragma unroll
                for (int k = 0; k < kPx / 4; ++k)
                    reinterpret_cast<uint4*>(s)[k] = make_uint4(d[p][4 * k], d[p][4 * k + 1], d[p][4 * k + 2], d[p][4 * k + 3]);
            } else {
                s[0] = d[p][0];
            }
        }
    }
}

bool heat_vector_path_ok(const HeatArgs& a) {
    return a.ow % kHeatVecPx == 0 && reinterpret_cast<uintptr_t>(a.canvas) % 16 == 0 && reinterpret_cast<uintptr_t>(a.state) % 16 == 0;
}

template <bool kVec>
static void launch_planes(const HeatArgs& a, dim3 grid, hipStream_t s) {
    const dim3 block(256);
    switch (a.planes) {
        case 1: hipLaunchKernelGGL((heat_kernel<kVec, 1>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((heat_kernel<kVec, 2>), grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL((heat_kernel<kVec, 3>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((heat_kernel<kVec, 4>), grid, block, 0, s, a); break;
    }
}

hipError_t launch_heat(const HeatArgs& a, hipStream_t s, int* vec_out) {
    if (a.planes < 1 || a.planes > kHeatMaxPlanes) return hipErrorInvalidValue;
    const bool vec = heat_vector_path_ok(a);
    const unsigned total = (unsigned)a.oh * ((unsigned)a.ow / (vec ? kHeatVecPx : 1));
    const dim3 grid(std::min((total + 255u) / 256u, kHeatMaxBlocks));
    if (vec) launch_planes<true>(a, grid, s);
    else launch_planes<false>(a, grid, s);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess && vec_out) *vec_out = vec ? 1 : 0;
    return e;
}

}  // namespace padel
