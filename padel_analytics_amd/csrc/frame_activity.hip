// frame_activity_kernel: per frame, over a rectangle, the summed luma difference to a reference image, the number of pixels whose
// difference exceeds tau, and the summed luma difference to the previous frame (the specification: include/padel_hip.h; the twin:
// activity.frame_activity_host).  One streaming pass: 3 bytes per pixel of the frames; the reference image is re-read by every frame
// and the previous frame was this launch's own traffic a moment ago, so both come from cache.
//
// Workgroup (band, frame) takes band_rows whole roi rows of one frame (at most 16384 pixels: 32-bit sums cannot wrap).  A row is
// cut at the pixels where the FRAME's byte address is a multiple of 16 — 3 is invertible mod 16, so one of any 16 consecutive pixels
// is — into a head of at most 15 pixels, units of 16 pixels = 48 bytes = three 16-byte vectors, and a tail of at most 15 pixels.
// A lane takes whole units: aligned 16-byte loads of the frame, and 16-byte loads of ref / prev at the same pixel, whose alignment
// is whatever their pointers give (the same as the frame's whenever h * w * 3 is a multiple of 16 and the buffers are allocations).
// Heads and tails go pixel by pixel through byte loads.  Lanes add into 32-bit registers, a wave reduces by cross-lane shuffles,
// the four waves through LDS, and three lanes store the workgroup's sums to its slab entry with plain stores.
// frame_activity_sum_kernel adds a frame's slab entries into its three uint64.  No atomics: the result is exact and the same for
// every launch shape.
#include "kernels.h"

#include <hip/hip_runtime.h>

#define ACT_THREADS 256

namespace padel {

__device__ __forceinline__ unsigned act_luma(unsigned b, unsigned g, unsigned r) { return (29u * b + 150u * g + 77u * r + 128u) >> 8; }
__device__ __forceinline__ unsigned act_absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

// 48 bytes = 16 pixels as 12 dwords; ALIGNED: p is a multiple of 16
template <bool ALIGNED>
__device__ __forceinline__ void act_load48(const uint8_t* p, uint32_t (&d)[12]) {
    uint4 v[3];
    if (ALIGNED) {
        const uint4* q = reinterpret_cast<const uint4*>(p);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    } else {
        __builtin_memcpy(v, p, 48);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { d[4 * k] = v[k].x; d[4 * k + 1] = v[k].y; d[4 * k + 2] = v[k].z; d[4 * k + 3] = v[k].w; }
}

// the 16 lumas of a unit (j is a compile-time constant after unrolling: each byte is one bit-field extract)
__device__ __forceinline__ void act_lumas(const uint32_t (&d)[12], unsigned (&y)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        unsigned c[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int j = 3 * k + t;
            c[t] = (d[j >> 2] >> (8 * (j & 3))) & 0xffu;
        }
        y[k] = act_luma(c[0], c[1], c[2]);
    }
}

__global__ void __launch_bounds__(ACT_THREADS) frame_activity_kernel(const ActivityArgs a) {
    const int band = blockIdx.x, fi = blockIdx.y, tid = threadIdx.x;
    const long long fb = (long long)a.h * a.w * 3;
    const uint8_t* const f = a.frames + (long long)fi * fb;
    const uint8_t* const p = fi ? f - fb : a.prev;                  // nullptr: frame 0 without a predecessor
    const int ya = a.y0 + band * a.band_rows;
    const int rows = min(a.y1, ya + a.band_rows) - ya, rw = a.x1 - a.x0;
    const unsigned tau = (unsigned)a.tau;
    unsigned sr = 0, ch = 0, sp = 0;

    // pixel offset (in bytes, < 2^30) of the roi's first pixel of row r, and that row's head: pixels up to the first one whose
    // frame address is a multiple of 16 (11 = 3^-1 mod 16)
    auto row_off = [&](int r) { return ((ya + r) * a.w + a.x0) * 3; };
    auto row_head = [&](int off) {
        const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(f + off) & 15u);
        return min((int)((((16u - mis) & 15u) * 11u) & 15u), rw);
    };

    const int umax = rw >> 4;                                       // units a row can have (one fewer where the head is long)
    for (int idx = tid; idx < rows * umax; idx += ACT_THREADS) {
        const int r = idx / umax, u = idx - r * umax;
        const int off = row_off(r), hd = row_head(off);
        if (u >= (rw - hd) >> 4) continue;
        const int o = off + (hd + 16 * u) * 3;
        uint32_t d[12];
        unsigned yf[16], yo[16];
        act_load48<true>(f + o, d);
        act_lumas(d, yf);
        act_load48<false>(a.ref + o, d);
        act_lumas(d, yo);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned df = act_absdiff(yf[k], yo[k]);
            sr += df;
            ch += df > tau ? 1u : 0u;
        }
        if (p) {
            act_load48<false>(p + o, d);
            act_lumas(d, yo);
#pragma unroll
            for (int k = 0; k < 16; ++k) sp += act_absdiff(yf[k], yo[k]);
        }
    }

    // heads and tails: 32 slots per row, slot s < 16 the head's pixel s, slot 16 + t the tail's pixel t
    for (int idx = tid; idx < rows * 32; idx += ACT_THREADS) {
        const int r = idx >> 5, s = idx & 31;
        const int off = row_off(r), hd = row_head(off);
        const int units = (rw - hd) >> 4, tail = rw - hd - 16 * units;
        int x;                                                      // pixel of the roi row
        if (s < 16) { if (s >= hd) continue; x = s; }
        else { if (s - 16 >= tail) continue; x = hd + 16 * units + (s - 16); }
        const int o = off + x * 3;
        const unsigned yf = act_luma(f[o], f[o + 1], f[o + 2]);
        const unsigned df = act_absdiff(yf, act_luma(a.ref[o], a.ref[o + 1], a.ref[o + 2]));
        sr += df;
        ch += df > tau ? 1u : 0u;
        if (p) sp += act_absdiff(yf, act_luma(p[o], p[o + 1], p[o + 2]));
    }

#pragma unroll
    for (int o = 32; o; o >>= 1) {
        sr += __shfl_xor(sr, o);
        ch += __shfl_xor(ch, o);
        sp += __shfl_xor(sp, o);
    }
    __shared__ unsigned part[3][ACT_THREADS / 64];
    if ((tid & 63) == 0) { part[0][tid >> 6] = sr; part[1][tid >> 6] = ch; part[2][tid >> 6] = sp; }
    __syncthreads();
    if (tid < 3) {
        unsigned v = 0;
#pragma unroll
        for (int wv = 0; wv < ACT_THREADS / 64; ++wv) v += part[tid][wv];
        a.slab[((size_t)fi * a.bands + band) * 3 + tid] = v;
    }
}

// one wave per frame: its bands' partial sums -> three uint64
__global__ void __launch_bounds__(64) frame_activity_sum_kernel(const uint32_t* slab, int bands, unsigned long long* out) {
    const int fi = blockIdx.x, lane = threadIdx.x;
    unsigned long long s[3] = {0, 0, 0};
    for (int b = lane; b < bands; b += 64) {
        const uint32_t* e = slab + ((size_t)fi * bands + b) * 3;
        s[0] += e[0]; s[1] += e[1]; s[2] += e[2];
    }
#pragma unroll
    for (int o = 32; o; o >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += __shfl_xor(s[k], o);
    if (lane < 3) out[(size_t)fi * 3 + lane] = lane == 0 ? s[0] : lane == 1 ? s[1] : s[2];
}

hipError_t launch_frame_activity(const ActivityArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(frame_activity_kernel, dim3((unsigned)a.bands, (unsigned)a.n), dim3(ACT_THREADS), 0, s, a);
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(frame_activity_sum_kernel, dim3((unsigned)a.n), dim3(64), 0, s, a.slab, a.bands, a.out);
    return hipGetLastError();
}

}  // namespace padel
