// pa_jpeg_decode on the device (include/padel_hip.h has the specification, mjpeg.decode_host is the numpy twin): three passes.
//   (a) jpeg_entropy_kernel   one wave per restart interval: lane 0 runs the shared decoder (jpeg_entropy.h) block by block into 64
//                             coefficients in LDS, the 64 lanes store the block — int16, zig-zag order, one coalesced 128-byte row.
//                             (Decoding 24 blocks per barrier instead of one was tried and measured the same: the pass is bound by
//                             lane 0's serial work, about 0.5 us per symbol, not by the barriers or the stores.)
//                             The bit stream is serial, so lanes cannot share one interval's decoding; intervals are what is parallel.
//   (b) jpeg_idct_kernel      one thread per block, as the encoder's DCT: dequantise, inverse DCT, 8 rows of 8 samples into the
//                             padded planes (Y: MCUs x 16, Cb / Cr: MCUs x 8 a side).
//   (c) jpeg_colour_kernel    one thread per 16 pixels of an output row: fancy chroma upsampling (rows r - 1 .. r + 1 of the chroma
//                             planes, which is why this is its own pass), YCbCr -> BGR, three 16-byte stores where width and
//                             destination allow, byte stores otherwise.
#include "jpeg_decode.h"
#include "jpeg_idct.h"

namespace padel {

using namespace jpeg;

static_assert(sizeof(HuffDec) == 896 && offsetof(JpegDecFrame, quant) == 4 * sizeof(HuffDec), "table layout");
static_assert(sizeof(JpegDecFrame) % 16 == 0 && offsetof(JpegDecFrame, quant) % 16 == 0, "quantisers are read 16 bytes at a time");

__global__ void __launch_bounds__(64) jpeg_entropy_kernel(const JpegDecArgs a) {
    __shared__ HuffDec tab[4];               // dc[0], dc[1], ac[0], ac[1] of the interval's frame
    __shared__ int16_t blk[64];
    __shared__ int s_status;
    const int lane = threadIdx.x;
    const JpegDecInterval iv = a.ivls[blockIdx.x];
    const JpegDecFrame* fr = a.frames + iv.frame;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(fr);
        uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
        for (int i = lane; i < (int)(4 * sizeof(HuffDec) / 4); i += 64) dst[i] = src[i];
    }
    if (lane == 0) s_status = 0;
    const HuffDec* dc[3] = {&tab[fr->comp_dc[0] & 1], &tab[fr->comp_dc[1] & 1], &tab[fr->comp_dc[2] & 1]};
    const HuffDec* ac[3] = {&tab[2 + (fr->comp_ac[0] & 1)], &tab[2 + (fr->comp_ac[1] & 1)], &tab[2 + (fr->comp_ac[2] & 1)]};
    BitReader r;
    br_init(&r, a.data, iv.begin, iv.end);
    int pred0 = 0, pred1 = 0, pred2 = 0;
    int16_t* out = a.coef + ((size_t)iv.frame * (size_t)(a.mcus_x * a.mcus_y) + (size_t)iv.first_mcu) * (kBlocksPerMcu * 64);
    const int blocks = iv.mcus * kBlocksPerMcu;
    for (int b = 0, j = 0; b < blocks; ++b, j = j == 5 ? 0 : j + 1) {
        blk[lane] = 0;
        __syncthreads();
        if (lane == 0 && s_status == 0) {
            int st;
            if (j < 4) st = decode_block(&r, dc[0], ac[0], &pred0, blk);
            else if (j == 4) st = decode_block(&r, dc[1], ac[1], &pred1, blk);
            else st = decode_block(&r, dc[2], ac[2], &pred2, blk);
            s_status = st;
        }
        __syncthreads();
        out[(size_t)b * 64 + lane] = s_status ? (int16_t)0 : blk[lane];      // a block that could not be decoded, and all behind it: zeros
    }
    __syncthreads();
    if (lane == 0) a.ivl_status[blockIdx.x] = s_status;
}

__global__ void __launch_bounds__(256) jpeg_idct_kernel(const JpegDecArgs a) {
    const size_t per_frame = (size_t)a.mcus_x * a.mcus_y * kBlocksPerMcu;
    const size_t B = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (B >= per_frame * (size_t)a.n) return;
    const int f = (int)(B / per_frame);
    const int rem = (int)(B % per_frame);
    const int mcu = rem / kBlocksPerMcu, k = rem % kBlocksPerMcu;
    const int my = mcu / a.mcus_x, mx = mcu % a.mcus_x;
    const int comp = k < 4 ? 0 : k - 3;
    const uint4* cs = reinterpret_cast<const uint4*>(a.coef + B * 64);
    const uint4* qs = reinterpret_cast<const uint4*>(a.frames[f].quant[comp]);
    int32_t b[64];
    PA_JUNROLL
    for (int i = 0; i < 8; ++i) {
        const uint4 c = cs[i], q = qs[i];
        const uint32_t cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
        PA_JUNROLL
        for (int j = 0; j < 4; ++j) {
            b[kZigzag[8 * i + 2 * j]] = (int32_t)(int16_t)(cw[j] & 0xffffu) * (int32_t)(qw[j] & 0xffffu);
            b[kZigzag[8 * i + 2 * j + 1]] = (int32_t)(int16_t)(cw[j] >> 16) * (int32_t)(qw[j] >> 16);
        }
    }
    idct_block(b);
    const size_t PW = (size_t)a.mcus_x * 16, PH = (size_t)a.mcus_y * 16;
    uint8_t* frame = a.planes + (size_t)f * (PW * PH * 3 / 2);
    uint8_t* p;
    size_t pitch;
    if (k < 4) {
        pitch = PW;
        p = frame + ((size_t)my * 16 + (k >> 1) * 8) * PW + (size_t)mx * 16 + (k & 1) * 8;
    } else {
        pitch = PW / 2;
        p = frame + PW * PH + (k == 5 ? PW * PH / 4 : 0) + (size_t)my * 8 * pitch + (size_t)mx * 8;
    }
    PA_JUNROLL
    for (int r = 0; r < 8; ++r) {
        uint2 v;
        v.x = (uint32_t)sample(b[8 * r]) | (uint32_t)sample(b[8 * r + 1]) << 8 | (uint32_t)sample(b[8 * r + 2]) << 16 | (uint32_t)sample(b[8 * r + 3]) << 24;
        v.y = (uint32_t)sample(b[8 * r + 4]) | (uint32_t)sample(b[8 * r + 5]) << 8 | (uint32_t)sample(b[8 * r + 6]) << 16 | (uint32_t)sample(b[8 * r + 7]) << 24;
        *reinterpret_cast<uint2*>(p + (size_t)r * pitch) = v;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) jpeg_colour_kernel(const JpegDecArgs a) {
    const int groups = (a.w + 15) / 16;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (size_t)groups * a.h * a.n) return;
    const int g = (int)(gid % groups);
    const int y = (int)((gid / groups) % a.h);
    const int f = (int)(gid / ((size_t)groups * a.h));
    const size_t PW = (size_t)a.mcus_x * 16, PH = (size_t)a.mcus_y * 16;
    const uint8_t* Yp = a.planes + (size_t)f * (PW * PH * 3 / 2);
    const uint8_t* Cb = Yp + PW * PH;
    const uint8_t* Cr = Cb + PW * PH / 4;
    const int ch = (a.h + 1) / 2, cw = (a.w + 1) / 2;
    const int r = y >> 1;
    const int rr = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
    const int c0 = g * 8;
    int sb[10], sr[10];
    PA_JUNROLL
    for (int i = 0; i < 10; ++i) {
        const int c = min(max(c0 - 1 + i, 0), cw - 1);
        sb[i] = 3 * Cb[(size_t)r * (PW / 2) + c] + Cb[(size_t)rr * (PW / 2) + c];
        sr[i] = 3 * Cr[(size_t)r * (PW / 2) + c] + Cr[(size_t)rr * (PW / 2) + c];
    }
    const uint4 yv = *reinterpret_cast<const uint4*>(Yp + (size_t)y * PW + (size_t)g * 16);
    const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
    uint8_t px[48];
    PA_JUNROLL
    for (int i = 0; i < 8; ++i) {
        const int y0 = (yw[i >> 1] >> (16 * (i & 1))) & 255, y1 = (yw[i >> 1] >> (16 * (i & 1) + 8)) & 255;
        ycc_to_bgr(y0, chroma_even(sb[i], sb[i + 1]), chroma_even(sr[i], sr[i + 1]), px + 6 * i);
        ycc_to_bgr(y1, chroma_odd(sb[i + 1], sb[i + 2]), chroma_odd(sr[i + 1], sr[i + 2]), px + 6 * i + 3);
    }
    uint8_t* d = a.dst + (((size_t)f * a.h + y) * a.w + (size_t)g * 16) * 3;
    if (VEC) {
        PA_JUNROLL
        for (int j = 0; j < 3; ++j) {
            uint32_t wds[4];
            PA_JUNROLL
            for (int k = 0; k < 4; ++k)
                wds[k] = (uint32_t)px[16 * j + 4 * k] | (uint32_t)px[16 * j + 4 * k + 1] << 8 | (uint32_t)px[16 * j + 4 * k + 2] << 16 |
                         (uint32_t)px[16 * j + 4 * k + 3] << 24;
            reinterpret_cast<uint4*>(d)[j] = make_uint4(wds[0], wds[1], wds[2], wds[3]);
        }
    } else {
        PA_JUNROLL
        for (int i = 0; i < 16; ++i)
            if (g * 16 + i < a.w) {
                d[3 * i] = px[3 * i];
                d[3 * i + 1] = px[3 * i + 1];
                d[3 * i + 2] = px[3 * i + 2];
            }
    }
}

hipError_t launch_jpeg_decode(const JpegDecArgs& a, int* path, hipStream_t s, hipEvent_t* ev) {
    if (ev) hipEventRecord(ev[0], s);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)a.n_ivls), dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (ev) hipEventRecord(ev[1], s);
    const size_t blocks = (size_t)a.n * a.mcus_x * a.mcus_y * kBlocksPerMcu;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (ev) hipEventRecord(ev[2], s);
    const size_t items = (size_t)a.n * a.h * ((a.w + 15) / 16);
    const bool vec = a.w % 16 == 0 && reinterpret_cast<uintptr_t>(a.dst) % 16 == 0;
    if (vec) hipLaunchKernelGGL(jpeg_colour_kernel<true>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(jpeg_colour_kernel<false>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
    *path = vec ? 1 : 2;
    e = hipGetLastError();
    if (ev && e == hipSuccess) hipEventRecord(ev[3], s);
    return e;
}

}  // namespace padel
