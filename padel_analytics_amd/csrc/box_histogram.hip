// box_histogram_kernel: per rectangle of a BGR frame, the 512-bin histogram of its pixels' colours quantised to three bits a channel
// (the specification: include/padel_hip.h; the twin: identity.box_histograms_host).  One pass over the rectangle's bytes.
//
// One workgroup per rectangle: the counts of a rectangle depend on nothing else in the call.  A row is cut as frame_activity.hip cuts
// it, at the pixels where the FRAME's byte address is a multiple of 16, into a head of at most 15 pixels, units of 16 pixels = 48
// bytes = three aligned 16-byte loads, and a tail of at most 15 pixels; heads and tails go pixel by pixel through byte loads.  (A
// torso rectangle of 20 .. 100 pixels has one to six units a row, and as many head and tail pixels as unit pixels at the narrow end.)
// A lane keeps the bin of its last pixel and how often it came in registers and adds to LDS only when the bin changes: a shirt is
// mostly one bin, and 64 lanes adding to one LDS word one by one would serialise.  Each wave adds into a histogram of its own with
// LDS atomics (integer addition: exact in any order); at the end lane t adds the four waves' bins 2t and 2t + 1 and stores them with
// one 8-byte store.  No global atomics, no partial results in memory.
#include "kernels.h"

#include <hip/hip_runtime.h>

#define BH_THREADS 256
#define BH_WAVES (BH_THREADS / 64)
#define BH_BINS 512

namespace padel {

// run-length front of a lane's pixels: (bin, count) not yet added to the wave's histogram
struct BhRun {
    unsigned* hist;
    unsigned bin = 0, cnt = 0;
    __device__ __forceinline__ void put(unsigned b) {
        if (b == bin) { ++cnt; return; }
        if (cnt) atomicAdd(&hist[bin], cnt);
        bin = b; cnt = 1;
    }
    __device__ __forceinline__ void flush() { if (cnt) atomicAdd(&hist[bin], cnt); cnt = 0; }
};

__global__ void __launch_bounds__(BH_THREADS) box_histogram_kernel(const BoxHistArgs a) {
    __shared__ unsigned hist[BH_WAVES][BH_BINS];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int32_t* const rc = a.rects + 5 * (size_t)j;
    const int x0 = rc[1], y0 = rc[2], rw = rc[3] - x0, rows = rc[4] - y0;
    const uint8_t* const f = a.frames + (long long)rc[0] * ((long long)a.h * a.w * 3);

    for (int i = tid; i < BH_WAVES * BH_BINS; i += BH_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    BhRun run{hist[tid >> 6]};

    // byte offset (< 2^30) of the rectangle's first pixel of row r, and that row's head: pixels up to the first one whose frame
    // address is a multiple of 16 (11 = 3^-1 mod 16)
    auto row_off = [&](int r) { return ((y0 + r) * a.w + x0) * 3; };
    auto row_head = [&](int off) {
        const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(f + off) & 15u);
        return min((int)((((16u - mis) & 15u) * 11u) & 15u), rw);
    };

    const int umax = rw >> 4;                                       // units a row can have (one fewer where the head is long)
    for (int idx = tid; idx < rows * umax; idx += BH_THREADS) {
        const int r = idx / umax, u = idx - r * umax;
        const int off = row_off(r), hd = row_head(off);
        if (u >= (rw - hd) >> 4) continue;
        const uint4* const q = reinterpret_cast<const uint4*>(f + off + (hd + 16 * u) * 3);
        const uint4 v0 = q[0], v1 = q[1], v2 = q[2];
        const uint32_t d[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            unsigned c[3];                                          // the top three bits of B, G, R: one bit-field extract each
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int b = 3 * k + t;
                c[t] = (d[b >> 2] >> (8 * (b & 3) + 5)) & 7u;
            }
            run.put((c[0] << 6) | (c[1] << 3) | c[2]);
        }
    }

    // heads and tails: 32 slots per row, slot s < 16 the head's pixel s, slot 16 + t the tail's pixel t
    for (int idx = tid; idx < rows * 32; idx += BH_THREADS) {
        const int r = idx >> 5, s = idx & 31;
        const int off = row_off(r), hd = row_head(off);
        const int units = (rw - hd) >> 4, tail = rw - hd - 16 * units;
        int x;                                                      // pixel of the rectangle's row
        if (s < 16) { if (s >= hd) continue; x = s; }
        else { if (s - 16 >= tail) continue; x = hd + 16 * units + (s - 16); }
        const int o = off + x * 3;
        run.put(((unsigned)(f[o] >> 5) << 6) | ((unsigned)(f[o + 1] >> 5) << 3) | (unsigned)(f[o + 2] >> 5));
    }
    run.flush();
    __syncthreads();

    uint2 v = make_uint2(0u, 0u);
#pragma unroll
    for (int wv = 0; wv < BH_WAVES; ++wv) { v.x += hist[wv][2 * tid]; v.y += hist[wv][2 * tid + 1]; }
    reinterpret_cast<uint2*>(a.out + (size_t)j * BH_BINS)[tid] = v;
}

hipError_t launch_box_histograms(const BoxHistArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(box_histogram_kernel, dim3((unsigned)a.k), dim3(BH_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace padel
