// Index arithmetic shared by the convolution kernels: which tile a workgroup owns, where a tile sits in the image, where a
// 16-byte operand slot sits in a swizzled LDS plane, division by a launch-time constant.  Integers only and no HIP type, so a
// plain C++ compiler can include it (tests/conv_index_main.cpp checks every function here on the CPU).
#pragma once

#if defined(__HIPCC__)
#define PADEL_IDX __host__ __device__ __forceinline__ constexpr
#else
#define PADEL_IDX inline constexpr
#endif

namespace padel {

// ---- the XCD-aware 1-D tile map.  The hardware deals workgroup `bid` to XCD bid % 8.  XCD x owns a contiguous run of pixel
// tiles (nmt / 8 of them, one more on the first nmt % 8 XCDs), and consecutive workgroups of one XCD are the CHANNEL tiles of
// one pixel tile: they run side by side on that XCD, so the input tile comes from HBM once and is re-read from its L2.
// Launchers pad the grid to 8 * ceil(nmt / 8) * nnt; the padding ids are invalid, and within an XCD they come after every valid
// id (the persistent walk of conv_patch_h2r.hip relies on that).
// A kernel computes the slot, tests it, RETURNS, and only then asks for the pixel tile: the order the compiler sees is part of
// the generated code.
struct XcdSlot { int q8, r8, xcd, mloc, nt; };      // nt: channel tile; mloc: pixel tile within the XCD's run
PADEL_IDX XcdSlot xcd_slot(int nmt, int nnt, int bid) {
    const int q8 = nmt >> 3, r8 = nmt & 7, xcd = bid & 7, idx = bid >> 3;
    const int mloc = idx / nnt, nt = idx - mloc * nnt;
    return {q8, r8, xcd, mloc, nt};
}
PADEL_IDX bool xcd_slot_padding(const XcdSlot& s) { return s.mloc >= s.q8 + (s.xcd < s.r8 ? 1 : 0); }
PADEL_IDX int xcd_slot_mtile(const XcdSlot& s) {
    return (s.xcd < s.r8 ? s.xcd * (s.q8 + 1) : s.r8 * (s.q8 + 1) + (s.xcd - s.r8) * s.q8) + s.mloc;
}

// pixel tile mt -> image n and the tile's first output pixel (y0, x0), for tiles of 2^LH x 2^LW pixels, row-major per image
struct TileOrigin { int n, y0, x0; };
template <int LH, int LW>
PADEL_IDX TileOrigin tile_origin(int Ho, int Wo, int mt) {
    const int txN = (Wo + (1 << LW) - 1) >> LW, tyN = (Ho + (1 << LH) - 1) >> LH;
    const int tpi = tyN * txN;
    const int n = mt / tpi, rt = mt - n * tpi;
    const int ty = rt / txN, tx = rt - ty * txN;
    return {n, ty << LH, tx << LW};
}

// ---- LDS planes of MFMA operands.  Full planes: 64 bytes per pixel, logical 16-byte chunk q (K slots 8q .. 8q + 7) of pixel p
// lives in slot q ^ 2 ((p >> 2) & 1): a ds_read_b128 of 16 consecutive pixels at any shift is conflict-free.  Tail planes (the
// 16-channel K tail of the fp16 / h2 kernels): 32 bytes per pixel, 16-byte slot s (channels 8s .. 8s + 7) at s ^ ((p >> 3) & 1).
PADEL_IDX unsigned swz_off(int p, int q) { return (unsigned)(p * 64 + ((q ^ (((p >> 2) & 1) << 1)) << 4)); }
PADEL_IDX unsigned swz_tail_off(int p, int s) { return (unsigned)(p * 32 + ((s ^ ((p >> 3) & 1)) << 4)); }

// the input patch under a tile of 16 pixels' width, halo included: 18 pixels wide; 10 rows under the 8 x 16 tile
constexpr int kPatchW = 18;
constexpr int kPatchPix = 10 * kPatchW;            // 180
constexpr int kPatchPlaneB = kPatchPix * 64;       // one 64-byte-per-pixel operand plane of a 32-channel chunk
constexpr int kPatchPadPlaneB = 192 * 64;          // the same, padded to 12 spans of 16 pixels (filled by LDS-DMA, a span per request)
constexpr int kPatchSqPix = 18 * kPatchW;          // 324: the patch under a 16 x 16 tile

// n / d for 0 <= n < 2^31 with the (magic, shift) pair of fill_fastdiv (kernels.h): 3 instructions instead of ~35
PADEL_IDX int fastdiv(int n, unsigned magic, unsigned shift) {
    return (int)(((unsigned)(((unsigned long long)(unsigned)n * magic) >> 32) + (unsigned)n) >> shift);
}

// 3x3 taps are walked COLUMN-major by every h2 kernel and in the packed weights (graph.py:pack_conv_weight_h2): k-step t
// of a channel chunk is tap (ky, kx) = (t % 3, t / 3).  The quad patch kernel (conv_patch_h2q.hip) keeps the input rows of
// one kx in registers across its three ky; one order for all kernels keeps their results bitwise identical.
PADEL_IDX int h2_tap_ky(int t) { return t % 3; }
PADEL_IDX int h2_tap_kx(int t) { return t / 3; }

}  // namespace padel
