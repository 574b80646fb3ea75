// Host-only half of the Motion-JPEG writer (jpeg_check.cpp): the refusals of pa_jpeg_encode, the quantisation tables of a quality,
// the frame header, and the block of tables the kernels read.  The launchers of jpeg_encode.hip are declared here too.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/padel_hip.h"
#include "jpeg_tables.h"

#include <cstddef>
#include <string>

namespace padel {

constexpr int kJpegHeaderBytes = 613;        // SOI 2, APP0 18, DQT 134, SOF0 19, DHT 420, DRI 6, SOS 14

// what the kernels read, uploaded per call (the tables depend on the quality, the header on the size as well)
struct JpegDevTables {
    uint32_t recip[2][64];                   // [luma | chroma][zig-zag position]: floor(2^32 / (8 q)) + 1
    uint16_t q4[2][64];                      // 4 q
    uint32_t dc[2][12];                      // [luma | chroma][category]: length << 16 | code
    uint32_t ac[2][256];                     // [luma | chroma][run << 4 | size]
    uint8_t header[kJpegHeaderBytes + 3];    // SOI .. SOS of every frame of the call
};

// the two tables of a quality, row-major
void jpeg_quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]);
// SOI .. SOS of an h x w frame -> out[0 .. kJpegHeaderBytes)
void jpeg_build_header(int h, int w, int quality, uint8_t* out);
void jpeg_fill_tables(int h, int w, int quality, JpegDevTables* t);
// every refusal of pa_jpeg_encode that needs no device pointer.  *src_span = bytes of src the kernel may read
int jpeg_validate(int n, int h, int w, const pa_yuv_desc* geom, int quality, size_t* src_span, std::string& err);

#if defined(__HIPCC__)
struct JpegEncArgs {
    const uint8_t* src;
    const JpegDevTables* tab;
    uint8_t* slots;                          // [n][rows] slots of slot_cap bytes
    int32_t* lens;                           // [n][rows] bytes written to each slot, its closing marker included
    int n, h, w, mcus, rows, nv12;
    int pitch_y, pitch_c, off_u, off_v;
    long long frame_stride;
    size_t slot_cap;
};
// one workgroup per (MCU row, frame)
hipError_t launch_jpeg_encode(const JpegEncArgs& a, hipStream_t s);
// n <= 256 frames: frame_off[n + 1] (from 0) and ivl_off[n][rows] (from the start of `out`) out of lens
hipError_t launch_jpeg_offsets(const int32_t* lens, int n, int rows, long long* frame_off, long long* ivl_off, hipStream_t s);
// header and intervals of every frame, back to back, into out
hipError_t launch_jpeg_gather(const uint8_t* slots, size_t slot_cap, const int32_t* lens, const long long* frame_off, const long long* ivl_off,
                              const JpegDevTables* tab, uint8_t* out, int n, int rows, hipStream_t s);
#endif

}  // namespace padel
