// Baseline JPEG of YUV 4:2:0 frames in HBM (include/padel_hip.h, pa_jpeg_encode): one workgroup per restart interval — one MCU row
// of one frame — and a gather that lays the intervals of every frame back to back behind its header.
//
// jpeg_encode_kernel, 256 threads, per workgroup:
//   1. the tables and the interval's 16 luma + 2 x 8 chroma rows go to LDS, the last column / row repeated up to the MCU edge;
//   2. the interval's blocks (6 per MCU, in scan order) are taken 256 at a time, one block per thread: level shift, integer DCT,
//      quantisation into LDS in zig-zag order (element k of thread t at [k][t]: no bank conflict); the quantised DCs of the whole
//      interval stay in LDS, so a DC difference needs no serial chain;
//   3. each thread counts its block's code bits, a prefix sum places the blocks, each thread packs its codes at its bit offset
//      (whole 32-bit words OR-ed into a zeroed LDS bit buffer; blocks share words at their ends);
//   4. the chunk's whole bytes are stuffed — a second prefix sum, over the 0xFF bytes of each thread's run — and stored to the
//      interval's slot; the bits of a last partial byte carry into the next chunk; the last chunk pads with 1-bits;
//   5. thread 0 appends RSTm (EOI behind the frame's last interval) and writes the slot's length.
// No coefficient reaches HBM.  Every loop runs to a bound fixed at launch; a slot is as large as the worst case of its interval
// (jpeg::interval_max_bytes), so no input can write outside it.
#include "jpeg_check.h"

#include <hip/hip_runtime.h>

namespace padel {
namespace {

constexpr int kThreads = 256;
constexpr int kBlockWords = jpeg::kBlockMaxBytes / 4;            // 52
constexpr int kBitWords = kThreads * kBlockWords + 4;            // a chunk's bits at their worst, 7 carried bits, one spare word
constexpr int kMaxRun = kBitWords * 4 / kThreads + 1;            // bytes per thread in the stuffing pass, at most

// exclusive prefix sum of v over the workgroup; *total = the sum.  s: 4 words of LDS.  Every thread calls it.
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* s, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) s[wave] = x;
    __syncthreads();
    unsigned base = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) base += i < wave ? s[i] : 0u;
    *total = s[0] + s[1] + s[2] + s[3];
    __syncthreads();
    return base + x - v;
}

struct BitCounter {
    unsigned bits = 0;
    __device__ __forceinline__ void put(unsigned, int len) { bits += (unsigned)len; }
};
// codes MSB first into 32-bit words: bit p of the stream is bit 31 - (p & 31) of word p >> 5
struct BitPacker {
    unsigned* words;
    unsigned long long acc = 0;
    int nacc, widx;
    __device__ __forceinline__ BitPacker(unsigned* w, unsigned start) : words(w), nacc((int)(start & 31)), widx((int)(start >> 5)) {}
    __device__ __forceinline__ void put(unsigned v, int len) {   // len <= 27, nacc < 32
        acc = (acc << len) | v;
        nacc += len;
        if (nacc >= 32) {
            atomicOr(&words[widx++], (unsigned)(acc >> (nacc - 32)));
            nacc -= 32;
            acc &= (1ull << nacc) - 1;
        }
    }
    __device__ __forceinline__ void flush() {
        if (nacc > 0) atomicOr(&words[widx], (unsigned)(acc << (32 - nacc)));
    }
};

__device__ __forceinline__ int bit_size(int v) { return 32 - __clz(v < 0 ? -v : v); }
__device__ __forceinline__ unsigned value_bits(int v, int s) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1); }

// the codes of one block: coef[k * kThreads] = zig-zag element k
template <class P> __device__ __forceinline__ void code_block(const int16_t* coef, int pred, const unsigned* dc, const unsigned* ac, P& p) {
    const int diff = coef[0] - pred;
    int s = bit_size(diff);
    unsigned e = dc[s];
    p.put(((e & 0xffffu) << s) | value_bits(diff, s), (int)(e >> 16) + s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int c = coef[k * kThreads];
        if (c == 0) { ++run; continue; }
        for (int z = 0; z < 3 && run >= 16; ++z, run -= 16) p.put(ac[0xf0] & 0xffffu, (int)(ac[0xf0] >> 16));     // ZRL
        s = bit_size(c);
        e = ac[run << 4 | s];
        p.put(((e & 0xffffu) << s) | value_bits(c, s), (int)(e >> 16) + s);
        run = 0;
    }
    if (run) p.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));                                                          // EOB
}

__global__ __launch_bounds__(kThreads) void jpeg_encode_kernel(JpegEncArgs a) {
    __shared__ unsigned s_recip[128];
    __shared__ unsigned short s_q4[128];
    __shared__ unsigned s_dc[24];
    __shared__ unsigned s_ac[512];
    __shared__ unsigned s_bits[kBitWords];
    __shared__ int16_t s_coef[64 * kThreads];
    __shared__ unsigned s_scan[4];
    extern __shared__ unsigned char s_dyn[];                     // 16 luma rows, 8 Cb rows, 8 Cr rows of the padded width, then the DCs

    const int tid = threadIdx.x, row = blockIdx.x, f = blockIdx.y;
    const int wp = a.mcus * 16, wc = a.mcus * 8, nb = a.mcus * jpeg::kBlocksPerMcu;
    unsigned char* s_y = s_dyn;
    unsigned char* s_c = s_dyn + 16 * wp;                        // Cb rows, then Cr rows
    int16_t* s_dcs = reinterpret_cast<int16_t*>(s_dyn + 24 * wp);

    if (tid < 128) { s_recip[tid] = a.tab->recip[tid >> 6][tid & 63]; s_q4[tid] = a.tab->q4[tid >> 6][tid & 63]; }
    if (tid < 24) s_dc[tid] = a.tab->dc[tid / 12][tid % 12];
    for (int i = tid; i < 512; i += kThreads) s_ac[i] = a.tab->ac[i >> 8][i & 255];

    const unsigned char* src = a.src + (size_t)f * (size_t)a.frame_stride;
    for (int i = tid; i < 16 * wp; i += kThreads) {
        const int y = i / wp, x = i - y * wp;
        const int sy = min(row * 16 + y, a.h - 1), sx = min(x, a.w - 1);
        s_y[i] = src[(size_t)sy * a.pitch_y + sx];
    }
    const int cstep = a.nv12 ? 2 : 1;
    for (int i = tid; i < 16 * wc; i += kThreads) {
        const int p = i / (8 * wc), r = i - p * 8 * wc, y = r / wc, x = r - y * wc;
        const int sy = min(row * 8 + y, a.h / 2 - 1), sx = min(x, a.w / 2 - 1);
        s_c[i] = src[(size_t)(p ? a.off_v : a.off_u) + (size_t)sy * a.pitch_c + (size_t)sx * cstep];
    }
    __syncthreads();

    unsigned char* slot = a.slots + ((size_t)f * a.rows + row) * a.slot_cap;
    const int chunks = (nb + kThreads - 1) / kThreads;
    unsigned carry_bits = 0, carry_byte = 0, outpos = 0;          // the same in every thread
    for (int chunk = 0; chunk < chunks; ++chunk) {
        const int b = chunk * kThreads + tid;
        const bool active = b < nb;
        const int mcu = b / jpeg::kBlocksPerMcu, k6 = b - mcu * jpeg::kBlocksPerMcu, comp = k6 >= 4;
        if (active) {
            int v[64];
            const unsigned char* px;
            int pitch;
            if (!comp) { px = s_y + (k6 >> 1) * 8 * wp + mcu * 16 + (k6 & 1) * 8; pitch = wp; }
            else { px = s_c + (k6 - 4) * 8 * wc + mcu * 8; pitch = wc; }
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int c = 0; c < 8; ++c) v[8 * r + c] = (int)px[r * pitch + c] - 128;
            jpeg::fdct_block(v);
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                const int c = v[jpeg::kZigzag[k]];
                const unsigned m = __umulhi((unsigned)(c < 0 ? -c : c) + s_q4[comp * 64 + k], s_recip[comp * 64 + k]);
                s_coef[k * kThreads + tid] = (int16_t)(c < 0 ? -(int)m : (int)m);
            }
            s_dcs[b] = s_coef[tid];
        }
        __syncthreads();
        int pred = 0;
        if (active) {
            if (!comp) pred = k6 ? s_dcs[b - 1] : (mcu ? s_dcs[b - 3] : 0);
            else pred = mcu ? s_dcs[b - jpeg::kBlocksPerMcu] : 0;
        }
        const unsigned* dc = s_dc + comp * 12;
        const unsigned* ac = s_ac + comp * 256;
        BitCounter counter;
        if (active) code_block(s_coef + tid, pred, dc, ac, counter);
        const bool last = chunk == chunks - 1;
        unsigned total;
        const unsigned off = block_scan(counter.bits, s_scan, &total);
        const unsigned end = carry_bits + total;                 // bits of the buffer in use, the carried ones included
        const unsigned pad = last ? (8 - (end & 7)) & 7 : 0;
        const int words = (int)((end + pad + 31) >> 5) + 1;
        for (int i = tid; i < kBitWords; i += kThreads)
            if (i < words) s_bits[i] = i == 0 ? carry_byte << 24 : 0u;
        __syncthreads();
        if (active) {
            BitPacker packer(s_bits, carry_bits + off);
            code_block(s_coef + tid, pred, dc, ac, packer);
            if (b == nb - 1 && pad) packer.put((1u << pad) - 1, (int)pad);
            packer.flush();
        }
        __syncthreads();
        const int nbytes = (int)((end + pad) >> 3);
        const int per = (nbytes + kThreads - 1) / kThreads;
        const int i0 = min(tid * per, nbytes), i1 = min(i0 + per, nbytes);
        unsigned ff = 0;
        for (int k = 0; k < kMaxRun; ++k) {
            const int i = i0 + k;
            if (i >= i1) break;
            ff += ((s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu) == 0xffu;
        }
        unsigned total_ff;
        unsigned p = outpos + (unsigned)i0 + block_scan(ff, s_scan, &total_ff);
        for (int k = 0; k < kMaxRun; ++k) {
            const int i = i0 + k;
            if (i >= i1) break;
            const unsigned byte = (s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu;
            slot[p++] = (unsigned char)byte;
            if (byte == 0xffu) slot[p++] = 0;
        }
        carry_bits = (end + pad) & 7;
        carry_byte = carry_bits ? ((s_bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 0xffu) : 0u;
        outpos += (unsigned)nbytes + total_ff;
        __syncthreads();                                         // s_bits and s_coef are free again
    }
    if (tid == 0) {
        slot[outpos] = 0xff;
        slot[outpos + 1] = (unsigned char)(row == a.rows - 1 ? 0xd9 : 0xd0 + (row & 7));
        a.lens[(size_t)f * a.rows + row] = (int32_t)(outpos + 2);
    }
}

// one workgroup, thread t = frame t (n <= 256)
__global__ __launch_bounds__(kThreads) void jpeg_offsets_kernel(const int32_t* lens, int n, int rows, long long* frame_off, long long* ivl_off) {
    __shared__ unsigned s_scan[4];
    const int t = threadIdx.x;
    unsigned size = 0;
    if (t < n) {
        size = kJpegHeaderBytes;
        for (int r = 0; r < rows; ++r) size += (unsigned)lens[(size_t)t * rows + r];
    }
    unsigned total;
    const unsigned off = block_scan(size, s_scan, &total);
    if (t < n) {
        frame_off[t] = off;
        long long at = (long long)off + kJpegHeaderBytes;
        for (int r = 0; r < rows; ++r) {
            ivl_off[(size_t)t * rows + r] = at;
            at += lens[(size_t)t * rows + r];
        }
    }
    if (t == 0) frame_off[n] = total;
}

// one workgroup per (interval, frame): its bytes, and in front of the first interval the header
__global__ __launch_bounds__(kThreads) void jpeg_gather_kernel(const uint8_t* slots, size_t slot_cap, const int32_t* lens, const long long* frame_off,
                                                               const long long* ivl_off, const JpegDevTables* tab, uint8_t* out, int rows) {
    const int row = blockIdx.x, f = blockIdx.y;
    const size_t idx = (size_t)f * rows + row;
    if (row == 0) {
        uint8_t* h = out + frame_off[f];
        for (int i = threadIdx.x; i < kJpegHeaderBytes; i += kThreads) h[i] = tab->header[i];
    }
    const uint8_t* src = slots + idx * slot_cap;
    uint8_t* dst = out + ivl_off[idx];
    const int len = lens[idx];
    for (int i = threadIdx.x; i < len; i += kThreads) dst[i] = src[i];
}

}  // namespace

hipError_t launch_jpeg_encode(const JpegEncArgs& a, hipStream_t s) {
    const size_t dyn = (size_t)24 * a.mcus * 16 + (size_t)a.mcus * jpeg::kBlocksPerMcu * sizeof(int16_t);
    hipLaunchKernelGGL(jpeg_encode_kernel, dim3(a.rows, a.n), dim3(kThreads), dyn, s, a);
    return hipGetLastError();
}

hipError_t launch_jpeg_offsets(const int32_t* lens, int n, int rows, long long* frame_off, long long* ivl_off, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(kThreads), 0, s, lens, n, rows, frame_off, ivl_off);
    return hipGetLastError();
}

hipError_t launch_jpeg_gather(const uint8_t* slots, size_t slot_cap, const int32_t* lens, const long long* frame_off, const long long* ivl_off,
                              const JpegDevTables* tab, uint8_t* out, int n, int rows, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_gather_kernel, dim3(rows, n), dim3(kThreads), 0, s, slots, slot_cap, lens, frame_off, ivl_off, tab, out, rows);
    return hipGetLastError();
}

}  // namespace padel
