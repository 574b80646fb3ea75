// What the kernels of jpeg_decode.hip read, and their launchers (engine_jpeg_decode.cpp fills the tables from jpeg_parse.cpp's answers).
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_entropy.h"
#include "jpeg_entropy_split.h"

namespace padel {

constexpr int kSplitMaxThreads = 1024;          // of a workgroup of jpeg_entropy_split_kernel

// one frame's tables, uploaded per sub-batch
struct alignas(16) JpegDecFrame {
    jpeg::HuffDec dc[2], ac[2];
    uint16_t quant[3][64];                   // per component, zig-zag order
    uint8_t comp_dc[3], comp_ac[3], pad_[10];
};
// one restart interval of the sub-batch
struct JpegDecInterval {
    long long begin, end;                    // its bytes inside the sub-batch's compressed data
    int32_t frame, first_mcu, mcus, pad_;    // frame: inside the sub-batch
};

struct JpegDecArgs {
    const uint8_t* data;                     // the compressed bytes of the sub-batch
    const JpegDecInterval* ivls;
    const JpegDecFrame* frames;
    int16_t* coef;                           // [n][mcus][6][64], zig-zag order
    int32_t* ivl_status;                     // [2][n_ivls]: the status words, then the rounds of the intervals on the split path
    uint8_t* planes;                         // per frame: Y [mcus_y * 16][mcus_x * 16], Cb, Cr [mcus_y * 8][mcus_x * 8]
    uint8_t* dst;                            // [n][h][w][3]
    int n, n_ivls, h, w, mcus_x, mcus_y;
    const int32_t* order;                    // [n_ivls] indices into ivls: the n_serial intervals of the serial kernel, then the n_split others
    int n_serial, n_split;
    int sub_bytes, split_threads;            // the split kernel: S as asked for (an interval of more than kSplitMaxSub * S bytes enlarges it), its block size
};
// (a) one wave per interval below the split threshold and one workgroup per interval at or above it (neither is launched over no
// intervals), (b) one thread per block, (c) one thread per 16 pixels of a row; *path: 1 vector stores, 2 byte stores.
// ev: NULL, or four events recorded in front of (a), (b), (c) and behind (c) (tools: the passes timed apart; both kernels of (a) lie
// between the first two)
hipError_t launch_jpeg_decode(const JpegDecArgs& a, int* path, hipStream_t s, hipEvent_t* ev);

}  // namespace padel
