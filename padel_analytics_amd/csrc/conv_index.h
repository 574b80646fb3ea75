// Index arithmetic shared by the convolution kernels: which tile a workgroup owns, where a tile sits in the image, where a
// 16-byte operand slot sits in a swizzled LDS plane, division by a launch-time constant.  Integers only and no HIP type, so a
// plain C++ compiler can include it (tests/conv_index_main.cpp and, for the stem patch, tests/stem_index_main.cpp check every
// function here on the CPU).
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

// ---- the u8 input patch of the fused stem + layer-1 kernel (stem_l1_h2.hip, register-weights instantiations).  A workgroup owns
// 4 x 16 pixels of layer 1 at (oy0, ox0): 9 x 33 stem positions p = 33 srow + scol, stem pixel (2 oy0 - 1 + srow, 2 ox0 - 1 + scol),
// whose tap (dy, dx) is input pixel (4 oy0 - 3 + 2 srow + dy, 4 ox0 - 3 + 2 scol + dx): 19 rows x 67 pixels of the NHWC4 input.
// The patch in LDS starts one pixel further left (4 ox0 - 4: 16-byte aligned in a row of W % 4 == 0 pixels) and holds 72 words
// (pixels) per row = 18 chunks of 16 bytes; chunk c = 18 row + ch lies at byte 16 c.  A chunk is wholly inside the image or
// wholly outside (zeros: the conv's padding, and never a row of the neighbouring frame).
constexpr int kStemPatchRows = 19, kStemPatchRowW = 72;
constexpr int kStemPatchChunks = kStemPatchRows * kStemPatchRowW / 4;       // 342
constexpr int kStemPatchB = kStemPatchRows * kStemPatchRowW * 4;            // 5472
PADEL_IDX int stem_patch_y0(int oy0) { return 4 * oy0 - 3; }
PADEL_IDX int stem_patch_x0(int ox0) { return 4 * ox0 - 4; }
PADEL_IDX int stem_patch_chunk_row(int c) { return c / (kStemPatchRowW / 4); }
PADEL_IDX int stem_patch_chunk_col(int c) { return 4 * (c % (kStemPatchRowW / 4)); }      // first pixel of the chunk within the patch row
PADEL_IDX bool stem_patch_chunk_inside(int H, int W, int iy, int ix0) { return (unsigned)iy < (unsigned)H && ix0 >= 0 && ix0 + 4 <= W; }
// patch word of tap (dy, dx) of stem position p < 297
PADEL_IDX int stem_patch_tap_word(int p, int dy, int dx) {
    const int srow = p / 33, scol = p - srow * 33;
    return (2 * srow + dy) * kStemPatchRowW + 1 + 2 * scol + dx;
}
// K slot kk of lane group lq is k = 8 lq + kk = 3 tap + colour (k >= 27: zero).  The 8 slots of a group span the taps
// 8 lq / 3 .. min(8 lq + 7, 26) / 3 — 3, 4, 3, 1 words; word i of the group is that tap's pixel (i past the span: the last one again,
// read and not used).
PADEL_IDX int stem_lq_tap0(int lq) { return 8 * lq / 3; }
PADEL_IDX int stem_lq_words(int lq) { return (8 * lq + 7 < 26 ? 8 * lq + 7 : 26) / 3 - stem_lq_tap0(lq) + 1; }
PADEL_IDX int stem_lq_word_tap(int lq, int i) { return stem_lq_tap0(lq) + (i < stem_lq_words(lq) ? i : stem_lq_words(lq) - 1); }
// Slots 2 j and 2 j + 1 of every group lie in the words lo, lo + 1 with lo = stem_pair_word(j).  Byte selector of v_perm_b32 with
// S1 = word lo, S0 = word lo + 1: result bytes (slot 2 j, 0, slot 2 j + 1, 0); selector value 4 w + colour, 0x0c: a zero byte.
PADEL_IDX int stem_pair_word(int j) { return j == 0 ? 0 : j - 1; }
PADEL_IDX unsigned stem_slot_selector(int lq, int kk) {
    const int k = 8 * lq + kk;
    return k >= 27 ? 0x0cu : (unsigned)(4 * (k / 3 - stem_lq_tap0(lq) - stem_pair_word(kk >> 1)) + k % 3);
}
PADEL_IDX unsigned stem_pair_selector(int lq, int j) {
    return stem_slot_selector(lq, 2 * j) | (stem_slot_selector(lq, 2 * j + 1) << 16) | 0x0c000c00u;
}

}  // namespace padel
