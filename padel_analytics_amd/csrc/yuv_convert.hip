// YUV 4:2:0 (NV12 / I420, 8 bit) -> packed BGR, the bytes every other kernel of the engine consumes (gfx950), HBM-bound:
// 1.5 bytes read and 3 written per pixel.  Nearest-neighbour chroma, 20-bit fixed point, all int32 (include/padel_hip.h,
// pa_yuv_desc; the readable twin is video.yuv420_to_bgr_host):
//     y = max(0, Y - y_off) * CY + (1 << 19)      u = U - 128      v = V - 128
//     R = clamp((y + CVR v) >> 20)    G = clamp((y + CUG u + CVG v) >> 20)    B = clamp((y + CUB u) >> 20)     (>> arithmetic)
// One thread converts a 2-row x 4-pixel block, so every chroma pair is read once.  A workgroup is 32 x 8 threads: 128 pixels
// of 16 rows.  kVec: dword loads of Y and of NV12's UV (two 16-bit loads for I420's planes) and three dword stores per row —
// only when the launcher has checked every address of THIS launch for alignment; otherwise bytes, which also covers the
// two-pixel tail of widths that are no multiple of 4.
#include "kernels.h"

namespace padel {

struct YuvChroma { int r, g, b; };       // the chroma terms of one 2x2 block

__device__ __forceinline__ YuvChroma yuv_chroma(const YuvArgs& a, int U, int V) {
    const int u = U - 128, v = V - 128;
    return {a.cvr * v, a.cug * u + a.cvg * v, a.cub * u};
}

// clamp(x >> 20, 0, 255) with the clamp applied BEFORE the shift (the same value: negatives give 0, anything from 256 << 20 up
// gives 255).  Written shift-then-clamp, the B and G of a pixel compile to one v_ashr_pk_u8_i32 whose result the compiler ORs into
// the word as if bits 16..31 were zero; on the MI355X they came back holding the upper half of the register's previous value
// (the destination was also the first source), so R and the next pixel's B carried stray bits.  This form selects no such instruction.
__device__ __forceinline__ int yuv_clamp8(int x) { return min(max(x, 0), (255 << 20) | 0xfffff) >> 20; }

// -> B | G << 8 | R << 16
__device__ __forceinline__ unsigned yuv_pixel(const YuvArgs& a, int Y, const YuvChroma& c) {
    const int y = max(0, Y - a.y_off) * a.cy + (1 << 19);
    return (unsigned)yuv_clamp8(y + c.b) | ((unsigned)yuv_clamp8(y + c.g) << 8) | ((unsigned)yuv_clamp8(y + c.r) << 16);
}

template <bool kVec, bool kNv12>
__global__ void __launch_bounds__(256) yuv420_to_bgr_kernel(const YuvArgs a) {
    const int bx = blockIdx.x * 32 + threadIdx.x;        // 4-pixel column block
    const int by = blockIdx.y * 8 + threadIdx.y;         // row pair
    const int x0 = bx * 4;
    if (x0 >= a.w || by * 2 >= a.h) return;
    const uint8_t* f = a.src + (size_t)blockIdx.z * (size_t)a.frame_stride;
    uint8_t* o = a.dst + ((size_t)blockIdx.z * a.h + (size_t)by * 2) * ((size_t)a.w * 3) + (size_t)x0 * 3;
    const uint8_t* py = f + (size_t)by * 2 * a.pitch_y + x0;
    const size_t crow = (size_t)by * a.pitch_c;
    if (kVec) {                                          // w % 4 == 0: every block is whole
        unsigned cu, cv;                                 // U and V of the two chroma pairs in bits 0..7 and 8..15
        if (kNv12) {
            const unsigned uv = *reinterpret_cast<const unsigned*>(f + a.off_u + crow + x0);      // U0 V0 U1 V1
            cu = (uv & 0xff) | ((uv >> 8) & 0xff00);
            cv = ((uv >> 8) & 0xff) | ((uv >> 16) & 0xff00);
        } else {
            cu = *reinterpret_cast<const unsigned short*>(f + a.off_u + crow + bx * 2);
            cv = *reinterpret_cast<const unsigned short*>(f + a.off_v + crow + bx * 2);
        }
        const YuvChroma c0 = yuv_chroma(a, cu & 0xff, cv & 0xff), c1 = yuv_chroma(a, cu >> 8, cv >> 8);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const unsigned yy = *reinterpret_cast<const unsigned*>(py + (size_t)r * a.pitch_y);
            const unsigned p0 = yuv_pixel(a, yy & 0xff, c0), p1 = yuv_pixel(a, (yy >> 8) & 0xff, c0);
            const unsigned p2 = yuv_pixel(a, (yy >> 16) & 0xff, c1), p3 = yuv_pixel(a, yy >> 24, c1);
            unsigned* od = reinterpret_cast<unsigned*>(o + (size_t)r * a.w * 3);                  // 12 bytes: B G R B | G R B G | R B G R
            od[0] = p0 | (p1 << 24);
            od[1] = (p1 >> 8) | (p2 << 16);
            od[2] = (p2 >> 16) | (p3 << 8);
        }
    } else {
        const int pairs = (a.w - x0) >= 4 ? 2 : 1;       // w is even: a tail block holds one chroma pair
        for (int k = 0; k < pairs; ++k) {
            int U, V;
            if (kNv12) {
                const uint8_t* pc = f + a.off_u + crow + x0 + 2 * k;
                U = pc[0]; V = pc[1];
            } else {
                U = f[a.off_u + crow + bx * 2 + k];
                V = f[a.off_v + crow + bx * 2 + k];
            }
            const YuvChroma c = yuv_chroma(a, U, V);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint8_t* yr = py + (size_t)r * a.pitch_y + 2 * k;
                uint8_t* ob = o + (size_t)r * a.w * 3 + 6 * k;
                const unsigned p0 = yuv_pixel(a, yr[0], c), p1 = yuv_pixel(a, yr[1], c);
                ob[0] = (uint8_t)p0; ob[1] = (uint8_t)(p0 >> 8); ob[2] = (uint8_t)(p0 >> 16);
                ob[3] = (uint8_t)p1; ob[4] = (uint8_t)(p1 >> 8); ob[5] = (uint8_t)(p1 >> 16);
            }
        }
    }
}

bool yuv_vector_path_ok(const YuvArgs& a) {
    const uintptr_t s = reinterpret_cast<uintptr_t>(a.src), d = reinterpret_cast<uintptr_t>(a.dst);
    if (a.w % 4 || s % 4 || d % 4 || a.pitch_y % 4) return false;
    if (a.n > 1 && a.frame_stride % 4) return false;
    if (a.nv12) return a.off_u % 4 == 0 && a.pitch_c % 4 == 0;
    return a.off_u % 2 == 0 && a.off_v % 2 == 0 && a.pitch_c % 2 == 0;     // (src and the stride are multiples of 4 already)
}

hipError_t launch_yuv420_to_bgr(const YuvArgs& a, hipStream_t s, int* vec_out) {
    const bool vec = yuv_vector_path_ok(a);
    const dim3 grid((unsigned)((a.w + 127) / 128), (unsigned)((a.h / 2 + 7) / 8), (unsigned)a.n), block(32, 8);
    if (vec && a.nv12) hipLaunchKernelGGL((yuv420_to_bgr_kernel<true, true>), grid, block, 0, s, a);
    else if (vec) hipLaunchKernelGGL((yuv420_to_bgr_kernel<true, false>), grid, block, 0, s, a);
    else if (a.nv12) hipLaunchKernelGGL((yuv420_to_bgr_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((yuv420_to_bgr_kernel<false, false>), grid, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess && vec_out) *vec_out = vec ? 1 : 0;
    return e;
}

}  // namespace padel
