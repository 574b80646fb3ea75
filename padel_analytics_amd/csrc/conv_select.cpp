// Which kernel runs a conv: the one place that knows.  Host code only (no HIP runtime call; compiles with g++).
//
//   * one TILE TABLE per path (fp32 tap, bf16x3, h2, fp16): id, family that runs the id natively, workgroup tile, and the
//     relative speeds the choosers score with                                                   -> conv_tile_shape
//   * the family PREDICATES (which layers a kernel family takes; they read ConvArgs only) and the operand-copy rule
//     that mirrors them                                                                          -> conv_wants_operand_copy
//   * the RESOLVER: (path, layer, requested id) -> (tile, family) after every fall-through      -> resolve_conv
//   * the four CHOOSERS over the table with one scoring helper                                  -> choose_conv_*_variant
//
// The .hip files keep kernels and launch_conv_<family>(a, tile, s), which launches exactly that tile; the step builder (launch_plan.cpp)
// resolves, launch_conv_family (conv_tap.hip) calls the launcher the row names.  A new tile is one table row and one launcher case.
#include "launch_plan.h"

#include <string.h>

namespace padel {

// rows = 0: `cols` consecutive output pixels (a linear pixel tile, BM = cols); else a rows x cols patch of the output map.
// s3 / s1: relative speed on 3x3 / 1x1 layers as measured (the profile each factor comes from is cited at the row);
// 0: never chosen by score (forced, or taken by a rule of the chooser).  Choosers walk a table in order and keep the first
// of equal scores, so the ORDER of the scored rows is part of the choice.
struct ConvTile {
    int id;
    ConvFamily family;
    int rows, cols, bn;
    float s3, s1;
};

// ---- fp32 MFMA tap kernels (conv_tap.hip).  Measured on MI355X (profiles/conv_tap_sweep_r1.txt) every tile runs at
// 113-121 TFLOP/s when its shape fits the layer exactly (128x16: ~0.8 of that), so the choice is about padding waste
// (channel tile and pixel tile fill) and about the last, partly filled round of workgroups.
static const ConvTile kTapTiles[] = {
    {7, CONV_TAP, 0, 64, 96, 1.00f, 1.00f},   {13, CONV_TAP, 0, 128, 96, 0.99f, 0.99f}, {9, CONV_TAP, 0, 128, 64, 0.99f, 0.99f},
    {14, CONV_TAP, 0, 128, 128, 1.00f, 1.00f}, {6, CONV_TAP, 0, 64, 128, 0.98f, 0.98f},  {20, CONV_TAP, 0, 128, 48, 0.98f, 0.98f},
    {11, CONV_TAP, 0, 128, 32, 0.99f, 0.99f},  {12, CONV_TAP, 0, 128, 16, 0.80f, 0.80f},
    {10, CONV_TAP, 0, 128, 64, 0.f, 0.f},      // 2 x 2 waves
    {15, CONV_TAP, 0, 128, 64, 0.f, 0.f},      // 8 waves
};

// ---- bf16x3 (conv_tap_bx3.hip, conv_patch_bx3.hip).  Relative tile speeds measured on MI355X
// (profiles/conv_bx3_sweep_r2d.txt, ..._r2j.txt): 3x3 — 64x96 and 128x48 (4 waves, 2 workgroups per CU) lead at 173-189 TFLOP/s
// on the yolov8m bottlenecks, the 8-wave tiles follow at ~0.9; 1x1 — since the channel tiles of a pixel tile run side by side on
// one XCD (the input is fetched from HBM once) the same two tiles lead there too (147-169 on the wide C2f cv2 layers).
// ids + 200 = the 2-stage ring: 51-53 KB of LDS instead of 77-80 -> 3 workgroups per CU, measured +5..12 % on every yolov8m 3x3
// layer shape and +4..20 % on the 1x1 ones (profiles/conv_bx3_sweep_r2k.txt, ..._r2l.txt)
static const ConvTile kBx3Tiles[] = {
    {213, CONV_BX3T, 0, 128, 96, 1.07f, 1.08f},     // 128 x 96 with 4 waves of 2 x 6 fragments, 2 workgroups per CU (..._r2p.txt)
    {220, CONV_BX3T, 0, 128, 48, 1.00f, 1.00f}, {207, CONV_BX3T, 0, 64, 96, 0.98f, 0.95f}, {209, CONV_BX3T, 0, 128, 64, 1.00f, 1.00f},
    {206, CONV_BX3T, 0, 64, 128, 0.90f, 0.70f}, {211, CONV_BX3T, 0, 128, 32, 0.85f, 0.87f}, {225, CONV_BX3T, 0, 64, 80, 0.95f, 0.90f},
    {7, CONV_BX3T, 0, 64, 96, 0.93f, 0.84f},    {20, CONV_BX3T, 0, 128, 48, 0.93f, 0.87f}, {13, CONV_BX3T, 0, 128, 96, 0.85f, 0.82f},
    {14, CONV_BX3T, 0, 128, 128, 0.83f, 0.85f}, {25, CONV_BX3T, 0, 64, 80, 0.90f, 0.78f},  // 25: the 19-fragment (304-channel) fused pose heads
    {11, CONV_BX3T, 0, 128, 32, 0.80f, 0.61f},  {9, CONV_BX3T, 0, 128, 64, 0.65f, 0.70f},  {6, CONV_BX3T, 0, 64, 128, 0.50f, 0.49f},
    {12, CONV_BX3T, 0, 128, 16, 0.45f, 0.26f},
    // stride-1 3x3: the patch kernel measured 1.18x (48-channel tiles, 3 workgroups per CU) / 1.15x (64-channel tiles) the best
    // tap tile on full 8 x 16 patches (profiles/conv_bx3_sweep_r2n.txt); its fill counts the pixels of partial patches
    {303, CONV_BX3P, 8, 16, 48, 1.17f, 0.f},    {304, CONV_BX3P, 8, 16, 64, 1.14f, 0.f},   {306, CONV_BX3P, 8, 16, 96, 0.f, 0.f},
};

// ---- h2 (conv_tap_h2.hip and the files named at the rows).  Tap-tile speeds start from the bf16x3 measurements and are
// re-measured for h2 in profiles/conv_h2_sweep_r3*.txt.  (The eight-wave tiles 230 = 128 x 192 and 231 = 256 x 96 of round 4 were
// timed at the start of round 5 and removed: 8-25 % slower than 128 x 96 on the K >= 576 1x1 and the stride-2 3x3 layers, 20-70 %
// on the P2 layers — profiles/r5a_tiles_230_231.txt; eight waves in lock step behind one barrier leave one workgroup per CU.)
static const ConvTile kH2Tiles[] = {
    {213, CONV_H2T, 0, 128, 96, 1.07f, 1.08f},  // 4 waves of 2 x 6 fragments
    {220, CONV_H2T, 0, 128, 48, 1.00f, 1.00f}, {207, CONV_H2T, 0, 64, 96, 0.98f, 0.95f}, {209, CONV_H2T, 0, 128, 64, 1.00f, 1.00f},
    {211, CONV_H2T, 0, 128, 32, 0.85f, 0.87f}, {225, CONV_H2T, 0, 64, 80, 0.95f, 0.90f},  // 225: the fused pose heads
    // 1x1 with the three-stage activation ring (conv_tap_h2p.hip): the two-stage tile's id + 30
    {239, CONV_H2D, 0, 128, 64, 0.f, 0.f},     {243, CONV_H2D, 0, 128, 96, 0.f, 0.f},
    // register weights and a deep activation ring (conv_1x1_h2s.hip): 1x1 — 128 x 96 (4 waves), 128 x 192 (8 waves, one workgroup per
    // CU), 64 x 192 (four waves, two workgroups per CU); stride-2 3x3 — 128 x 192, 64 x 192
    {244, CONV_H2S, 0, 128, 96, 0.f, 0.f},     {245, CONV_H2S, 0, 128, 192, 0.f, 0.f},   {247, CONV_H2S, 0, 64, 192, 0.f, 0.f},
    {246, CONV_H2S3, 0, 128, 192, 0.f, 0.f},   {248, CONV_H2S3, 0, 64, 192, 0.f, 0.f},
    // stride-1 3x3 patch kernel (conv_patch_h2.hip).  (The 6-fragment patch tile accumulates its main product in ONE level —
    // registers — and measured no faster than the 3-fragment one, profiles/conv_h2_sweep_r3a.txt: removed in round 5, like the
    // software-pipelined 64-channel tile 314 — 10-15 % slower than 304, profiles/conv_h2_sweep_r3f_pipe.txt.)
    {303, CONV_H2P, 8, 16, 48, 1.17f, 0.f},    {304, CONV_H2P, 8, 16, 64, 1.10f, 0.f},
    {313, CONV_H2P, 8, 16, 48, 0.f, 0.f},      // 303 with the software-pipelined schedule
    // the quad patch kernel (conv_patch_h2q.hip: 8 x 16 pixels x 96 channels per workgroup, 2 workgroups per CU) measured
    // 1.02-1.05 x the 48-channel tile where the channels fill its tiles (profiles/r3k_sweep_h2q.txt); bitwise the same results
    {323, CONV_H2Q, 8, 16, 96, 1.21f, 0.f},
    // two-product layers (PA_CONV_W_SINGLE) with at least two 32-channel chunks: the register-weights form of the quad tile
    // (conv_patch_h2r.hip, round 6: weights global -> VGPR, one barrier per chunk, 2 persistent workgroups per CU) measured
    // 1.15-1.18 x the quad kernel (96 -> 96: 440 -> 505, 192 -> 192: 520 -> 615 TFLOP/s; profiles/r6_sweep_h2r.txt) — fast enough to
    // take channel counts that leave its last 96-channel tile part empty (192 -> 256: 553 vs 473 on the 64-channel tile)
    {324, CONV_H2R, 8, 16, 96, 1.40f, 0.f},
    // the same kernel on 64-channel tiles (a wave 4 rows x 2 fragments): two-product layers whose channels are not a multiple of 96
    // (192 -> 256: 600 vs 544 on tile 324 vs 472 on the 64-channel patch tile; 192 -> 64: 569 vs 451; 64 -> 64: 401 vs 325) and,
    // at kH2rThreeProducts, every THREE-product layer with whole chunks — TrackNetV3's fp32 checkpoints (64 -> 64 .. 512 -> 512:
    // 314-438 vs 294-393 TFLOP/s) — profiles/r6u_sweep_h2r_nf2.txt
    {325, CONV_H2R, 8, 16, 64, 1.33f, 0.f},
    // few input channels (16 / 32 / 48: 5-14 k-steps): the wide patch kernel keeps the whole K extent of a 16 x 16 pixel tile in
    // LDS.  h2v (conv_patch_h2v.hip, round 6) is its register-weights form and runs the id where it applies; the chooser scores the
    // id by the h2w rows (conv_patch_h2w.hip): 16 -> 16: 121 vs 42 TFLOP/s, 32 -> 32: 185 vs 148, 48 -> 48: 244 vs 211 for the best
    // 8 x 16 / tap tile (profiles/r3_sweep_h2w.txt)
    {341, CONV_H2V, 16, 16, 16, 0.f, 0.f},     {341, CONV_H2W, 16, 16, 16, 1.28f, 0.f},
    {342, CONV_H2V, 16, 16, 32, 0.f, 0.f},     {342, CONV_H2W, 16, 16, 32, 1.42f, 0.f},
    {343, CONV_H2V, 16, 16, 48, 0.f, 0.f},     {343, CONV_H2W, 16, 16, 48, 1.46f, 0.f},
};
static const float kH2rThreeProducts = 1.22f;      // tile 325 on a three-product layer (its row holds the two-product speed)

// ---- fp16 (conv_tap16.hip, conv_patch16.hip).  These kernels are issue- / HBM-bound, not MFMA-bound, so (a) the channel tile
// should cover all of cout when it can (every extra channel tile re-reads the whole input from L2 / HBM), (b) bigger per-wave
// tiles amortise the fixed per-k-step instruction cost, (c) the grid still has to fill 256 CUs.
static const ConvTile kF16Tiles[] = {
    {30, CONV_TAP16, 0, 128, 128, 1.30f, 1.30f},   // + 30: 4 waves of 64 x 64
    {31, CONV_TAP16, 0, 128, 96, 1.25f, 1.25f},  {32, CONV_TAP16, 0, 128, 64, 1.10f, 1.10f},  {6, CONV_TAP16, 0, 64, 128, 1.05f, 1.05f},
    {7, CONV_TAP16, 0, 64, 96, 1.00f, 1.00f},    {9, CONV_TAP16, 0, 128, 64, 1.00f, 1.00f},   {20, CONV_TAP16, 0, 128, 48, 0.95f, 0.95f},
    {11, CONV_TAP16, 0, 128, 32, 0.85f, 0.85f},  {12, CONV_TAP16, 0, 128, 16, 0.60f, 0.60f},
    // + 40: the same tile with 64-channel (double) k-steps.  They win where K is a whole number of 64-channel steps and long
    // enough to matter: 3x3 with cin % 64 == 0 (yolov8m 192 -> 192 / 304: 684-696 vs 626 TFLOP/s,
    // profiles/conv_tap16_sweep_r2i.txt); with a 32-channel tail or on the short-K 1x1 layers the single-step tiles stay ahead
    {49, CONV_TAP16D, 0, 128, 64, 1.40f, 0.f},   {72, CONV_TAP16D, 0, 128, 64, 1.40f, 0.f},
    {46, CONV_TAP16D, 0, 64, 128, 0.f, 0.f},     {47, CONV_TAP16D, 0, 64, 96, 0.f, 0.f},      {51, CONV_TAP16D, 0, 128, 32, 0.f, 0.f},
    {60, CONV_TAP16D, 0, 128, 48, 0.f, 0.f},     {70, CONV_TAP16D, 0, 128, 128, 0.f, 0.f},    {71, CONV_TAP16D, 0, 128, 96, 0.f, 0.f},
    // stride-1 3x3: the patch kernel (conv_patch16.hip) fetches the input once per chunk instead of once per tap:
    // 806 vs 662 TFLOP/s on 192 -> 192, 875 vs 674 on the 256-channel heads, 558 vs 461 on 48(64) -> 64, about even on
    // the short-K 96 -> 96 layers (profiles/conv_tap16_sweep_r2x_patch.txt) — hence the K-length factor of the chooser
    {304, CONV_P16, 8, 16, 64, 1.70f, 0.f},      {303, CONV_P16, 8, 16, 48, 1.55f, 0.f},      {306, CONV_P16, 8, 16, 96, 1.45f, 0.f},
    // the quad kernel (16 x 16 pixels per workgroup): 749-770 vs 656-682 TFLOP/s on 96 -> 96, 885 vs 857 on 192 -> 192; behind
    // on partial channel tiles and on maps that do not fill 16-row tiles (profiles/r3s_sweep_p16q.txt)
    {323, CONV_P16Q, 16, 16, 48, 0.f, 0.f},      {324, CONV_P16Q, 16, 16, 64, 0.f, 0.f},      {326, CONV_P16Q, 16, 16, 96, 1.78f, 0.f},
};

struct TileSpan { const ConvTile* t; int n; };
static TileSpan tiles_of(int path) {
    switch (path) {
        case CONV_PATH_TAP: return {kTapTiles, (int)(sizeof(kTapTiles) / sizeof(ConvTile))};
        case CONV_PATH_BX3: return {kBx3Tiles, (int)(sizeof(kBx3Tiles) / sizeof(ConvTile))};
        case CONV_PATH_H2: return {kH2Tiles, (int)(sizeof(kH2Tiles) / sizeof(ConvTile))};
        case CONV_PATH_F16: return {kF16Tiles, (int)(sizeof(kF16Tiles) / sizeof(ConvTile))};
    }
    return {nullptr, 0};
}
// (ids 341..343 have two rows, h2v then h2w: without `family` the first is returned, so the shape lookup relies on the rows of
//  one id agreeing in shape)
static const ConvTile* find_tile(int path, int id, int family = -1) {
    const TileSpan ts = tiles_of(path);
    for (int i = 0; i < ts.n; ++i)
        if (ts.t[i].id == id && (family < 0 || ts.t[i].family == family)) return &ts.t[i];
    return nullptr;
}

bool conv_tile_shape(int path, int id, int* bm, int* bn) {
    const ConvTile* t = find_tile(path, id);
    if (!t) return false;
    *bm = t->rows ? t->rows * t->cols : t->cols;
    *bn = t->bn;
    return true;
}

// tuning "timeline": the one kernel instantiated with s_memtime stamps — the 3x3 of the fp32 64 x 96 tap tile
int conv_timeline_words(const ConvLaunched& k, int ksize) {
    if (!strcmp(k.family, "tap") && k.tile == 7 && ksize == 3) return kConvDbgWords;
    return 0;
}

// =====================================================================================================  predicates
// k-steps of a layer in the packed h2 blob: 9 taps per whole 32-channel chunk + 5 tap pairs for a 16-channel tail
// (1x1 layers: one k-step per 32 channels, a 16-channel tail half-filled)
int h2_ksteps(int cin, int ksize) { return ksize == 3 ? (cin >> 5) * 9 + ((cin & 16) ? 5 : 0) : (cin + 31) >> 5; }
size_t conv_h2r_copy_bytes(int n16, int cin, int ksize) { return (size_t)n16 * (size_t)h2_ksteps(cin, ksize) * 2048; }

// The LAYER classes of the kernels that read an operand-order weight copy (ConvArgs::wr), shared by their predicates below and
// by conv_wants_operand_copy, which decides which convs get one
static bool few_channels(int cin) { return cin == 16 || cin == 32 || cin == 48; }
static bool whole_chunks(int cin, int at_least) { return (cin & 31) == 0 && cin >= at_least; }
static bool h2r_layer(int k, int s, int cin) { return k == 3 && s == 1 && whole_chunks(cin, 64); }
static bool h2v_layer(int k, int s, int cin) { return k == 3 && s == 1 && few_channels(cin); }
static bool h2s_layer(int k, int s, int cin) { return k == 1 && s == 1 && whole_chunks(cin, 64); }      // two products only
static bool h2s3_layer(int k, int s, int cin) { return k == 3 && s == 2 && whole_chunks(cin, 32); }     // two products only
static bool stem_l1_layer(int k, int s, int cin) { return k == 3 && s == 2 && few_channels(cin); }      // stem_l1_h2.hip: the layer behind the stem

bool conv_wants_operand_copy(int ksize, int stride, int cin, bool w_single) {
    return h2r_layer(ksize, stride, cin) || h2v_layer(ksize, stride, cin) || stem_l1_layer(ksize, stride, cin) ||
           (w_single && (h2s_layer(ksize, stride, cin) || h2s3_layer(ksize, stride, cin)));
}

// The family predicates: which layers a kernel family takes (they read ConvArgs only; the resolver and the choosers ask them)
static bool same_size(const ConvArgs& a) { return a.Ho == a.H && a.Wo == a.W; }
// an absorbed nn.Upsample(2) (a.in2): whole 32-channel chunks from a coarse map of an even-sized input
static bool up_ok(const ConvArgs& a) { return (a.up_c & 31) == 0 && a.up_c > 0 && a.up_c <= a.cin && ((a.H | a.W) & 1) == 0; }
static bool up_ok_1x1(const ConvArgs& a) { return !a.in2 || (a.ksize == 1 && a.stride == 1 && up_ok(a)); }
static bool up_ok_patch(const ConvArgs& a) { return !a.in2 || ((a.cin & 31) == 0 && up_ok(a)); }

static bool conv_bx3p_supported(const ConvArgs& a) {
    return a.ksize == 3 && a.stride == 1 && (a.cin & 15) == 0 && a.cin >= 16 && same_size(a) && a.w3 != nullptr && up_ok_patch(a);
}
static bool conv_h2p_supported(const ConvArgs& a) {
    return a.ksize == 3 && a.stride == 1 && (a.cin & 15) == 0 && a.cin >= 16 && same_size(a) && a.w != nullptr && up_ok_patch(a);
}
static bool conv_h2q_supported(const ConvArgs& a) {
    return a.ksize == 3 && a.stride == 1 && whole_chunks(a.cin, 32) && same_size(a) && a.w != nullptr && !a.in2;
}
static bool conv_h2r_supported(const ConvArgs& a) {
    return a.wr && h2r_layer(a.ksize, a.stride, a.cin) && same_size(a) && a.w != nullptr && !a.in2;
}
static bool conv_h2w_supported(const ConvArgs& a) {
    return a.ksize == 3 && a.stride == 1 && few_channels(a.cin) && same_size(a) && a.w != nullptr && !a.in2;
}
static bool conv_h2v_supported(const ConvArgs& a) {
    return a.wr && h2v_layer(a.ksize, a.stride, a.cin) && same_size(a) && a.w != nullptr && !a.in2;
}
static bool conv_h2s_supported(const ConvArgs& a) {
    return a.w_single && a.wr && h2s_layer(a.ksize, a.stride, a.cin) && same_size(a) && a.w != nullptr && !a.in2 &&
           (long long)128 * a.in_cs * 4 < 0x7FFFFFFFll;
}
static bool conv_h2s3_supported(const ConvArgs& a) {
    return a.w_single && a.wr && h2s3_layer(a.ksize, a.stride, a.cin) && a.w != nullptr && !a.in2 && a.Ho <= (a.H + 1) / 2 &&
           a.Wo <= (a.W + 1) / 2 && (long long)4 * a.W * a.in_cs * 4 < 0x3FFFFFFFll;
}
static bool conv_p16_supported(const ConvArgs& a) { return a.ksize == 3 && a.stride == 1 && whole_chunks(a.cin, 32) && same_size(a); }

// does `family` run layer `a` as tile `id`?  (the family's predicate and what the tile itself asks for)
static bool family_takes(ConvFamily family, const ConvArgs& a, int id) {
    switch (family) {
        case CONV_TAP: case CONV_TAP16: case CONV_TAP16D: return true;
        case CONV_BX3T: return up_ok_1x1(a);
        case CONV_BX3P: return conv_bx3p_supported(a);
        case CONV_H2T: return up_ok_1x1(a);
        case CONV_H2D: return a.ksize == 1 && up_ok_1x1(a);
        case CONV_H2S: return conv_h2s_supported(a);
        case CONV_H2S3: return conv_h2s3_supported(a);
        case CONV_H2P: return conv_h2p_supported(a);
        case CONV_H2Q: return conv_h2q_supported(a);
        case CONV_H2R: return conv_h2r_supported(a) && (id == 325 || a.w_single);      // 96-channel tiles: two-product layers only
        case CONV_H2V: return !(a.tune & kTunePrevGen) && conv_h2v_supported(a) && (id < 343 || a.w_single);      // kTunePrevGen: h2w, the round-3 kernel; 3 fragments: two products only
        case CONV_H2W: return conv_h2w_supported(a);
        case CONV_P16: case CONV_P16Q: return conv_p16_supported(a);
    }
    return false;
}

// =====================================================================================================  resolver
// `id` as a tile of `family`, if the table has that row and the family takes the layer
struct Resolved { int tile; ConvFamily family; };
static bool take(int path, const ConvArgs& a, int id, ConvFamily family, Resolved* out) {
    if (!find_tile(path, id, family) || !family_takes(family, a, id)) return false;
    out->tile = id; out->family = family;
    return true;
}
// ... of whichever family the table names for it
static bool take(int path, const ConvArgs& a, int id, Resolved* out) {
    const ConvTile* t = find_tile(path, id);
    return t && take(path, a, id, t->family, out);
}

static bool resolve_bx3(const ConvArgs& a, int id, Resolved* out) {
    if ((a.cin & 15) || a.cin < 16 || !a.w3) return false;
    const bool patch_id = id >= 300 && id < 400;
    if (a.in2 && a.ksize == 3) return patch_id && take(CONV_PATH_BX3, a, id, CONV_BX3P, out);      // absorbed upsample in front of a 3x3: the patch kernel only
    if (a.in2) {                                            // ... in front of a 1x1: the three tiles instantiated for it
        id = (id == 209 || id == 9 || id == 304) ? 209 : (id == 213 || id == 13 || id == 14 || id == 306 || id == 206 || id == 6) ? 213 : 220;
        return take(CONV_PATH_BX3, a, id, CONV_BX3T, out);
    }
    if (patch_id) {                                         // patch kernel, or its tap-kernel sibling where it does not apply
        if (conv_bx3p_supported(a)) return take(CONV_PATH_BX3, a, id, CONV_BX3P, out);
        id = id == 303 ? 220 : id == 304 ? 209 : 206;
    }
    return take(CONV_PATH_BX3, a, id, CONV_BX3T, out);
}

static bool resolve_f16(const ConvArgs& a, int id, Resolved* out) {
    if ((a.cin & 31) || a.cin < 32 || a.res_pre) return false;      // PA_CONV_RES_PREACT: h2 and bf16x3 epilogues only
    if (id >= 300 && id < 400) {                            // fp16 patch kernels, or a tap tile where they do not apply
        if (conv_p16_supported(a)) return take(CONV_PATH_F16, a, id, out);
        id = id == 303 ? 20 : id == 304 ? 9 : 31;
    }
    return take(CONV_PATH_F16, a, id, out);
}

// tile ids follow the bf16x3 ids (+ 200); 3xx = the patch kernels or, where they do not apply, a tap sibling
static bool resolve_h2(const ConvArgs& a, int id, Resolved* out) {
    const int P = CONV_PATH_H2;
    if ((a.cin & 15) || a.cin < 16 || !a.w || !a.oscale || !a.ovf_flag) return false;
    if (id >= 341 && id <= 343) {          // the wide patch kernel: its register-weights form, else the round-3 kernel, else the 48-channel patch tile
        if (take(P, a, id, CONV_H2V, out) || take(P, a, id, CONV_H2W, out)) return true;
        id = 303;
    }
    if (id == 324 || id == 325) {          // the register-weights quad kernels; elsewhere the quad kernel / the 64-channel patch tile
        if (take(P, a, id, CONV_H2R, out)) return true;
        id = id == 324 ? 323 : 304;
    }
    if (id == 323) {                       // the quad patch kernel; where it does not apply, the 48-channel patch tile
        if (take(P, a, id, CONV_H2Q, out)) return true;
        id = 303;
    }
    if (a.in2 && a.ksize == 3) return id >= 300 && id < 400 && take(P, a, id, CONV_H2P, out);      // an absorbed upsample in front of a 3x3: the patch kernel only
    if (id >= 300 && id < 400) {
        if (conv_h2p_supported(a)) return take(P, a, id, CONV_H2P, out);
        const int nf = id - 300;           // where the patch kernel does not apply: its tap sibling
        id = (nf == 3 || nf == 13) ? 220 : (nf == 4 || nf == 14) ? 209 : 213;
    }
    if (id == 246 || id == 248) {          // stride-2 3x3 on the register-weights ring machine; elsewhere the 128 x 96 tap tile
        if (take(P, a, id, CONV_H2S3, out)) return true;
        id = 213;
    }
    if (id == 244 || id == 245 || id == 247) {   // 1x1 with register weights; elsewhere the deep-ring tile
        if (take(P, a, id, CONV_H2S, out)) return true;
        id = 243;
    }
    if (id == 243 || id == 239) {          // 1x1 with the three-stage activation ring; other kernel sizes: the plain tile
        if (take(P, a, id, CONV_H2D, out)) return true;
        id -= 30;
    }
    return take(P, a, id, CONV_H2T, out);
}

const char* conv_family_name(ConvFamily f) {
    static const char* const names[] = {"tap", "bx3t", "bx3p", "h2t", "h2d", "h2s", "h2s3", "h2p", "h2q", "h2r", "h2w", "h2v", "tap16", "tap16d", "p16", "p16q"};
    return names[f];
}

bool resolve_conv(int path, const ConvArgs& a, int requested, ConvLaunched* out, ConvFamily* family) {
    Resolved r{-1, CONV_TAP};
    if (a.ksize != 3 && a.ksize != 1) return false;
    bool ok = false;
    switch (path) {
        case CONV_PATH_TAP: ok = !(a.cin & 15) && a.cin >= 16 && !a.res_pre && take(path, a, requested, &r); break;      // PA_CONV_RES_PREACT: h2 and bf16x3 epilogues only
        case CONV_PATH_BX3: ok = resolve_bx3(a, requested, &r); break;
        case CONV_PATH_H2: ok = resolve_h2(a, requested, &r); break;
        case CONV_PATH_F16: ok = resolve_f16(a, requested, &r); break;
    }
    if (ok && out) *out = ConvLaunched{r.tile, conv_family_name(r.family)};
    if (ok && family) *family = r.family;
    return ok;
}

// =====================================================================================================  choosers
// speed x fill of the channel tiles x fill of the pixel tiles x fill of the last round of workgroups on 256 CUs (`rounds`).
// The products keep the order the measurements were fitted with: scores are compared with >, a re-associated product can flip a tie.
static float tile_score(const ConvTile& t, const ConvArgs& a, float speed, bool rounds = true) {
    const int nf = t.bn / 16, bm = t.rows ? t.rows * t.cols : t.cols;
    const long long mtiles = t.rows ? (long long)(a.M / (a.Ho * a.Wo)) * ((a.Ho + t.rows - 1) / t.rows) * ((a.Wo + t.cols - 1) / t.cols)
                                    : (long long)((a.M + bm - 1) / bm);
    const int ntiles = (a.n16 + nf - 1) / nf;
    const float fill = (float)a.n16 / (float)(ntiles * nf) * (float)a.M / (float)(mtiles * bm);
    if (!rounds) return speed * fill;
    const long long blocks = mtiles * ntiles;
    const long long per_cu = (blocks + 255) / 256;
    if (t.rows) return speed * fill * (float)blocks / (256.f * (float)per_cu);
    const float occ = (float)blocks / (256.f * (float)per_cu);
    return speed * fill * occ;
}
struct Best {
    float score = -1.f;
    int id;
    void offer(float sc, int tile) { if (sc > score) { score = sc; id = tile; } }
};
// the linear tiles of a table, scored by their 3x3 / 1x1 speed
static void offer_linear(Best& b, int path, const ConvArgs& a) {
    const TileSpan ts = tiles_of(path);
    for (int i = 0; i < ts.n; ++i) {
        const float sp = a.ksize == 3 ? ts.t[i].s3 : ts.t[i].s1;
        if (!ts.t[i].rows && sp > 0.0f) b.offer(tile_score(ts.t[i], a, sp), ts.t[i].id);
    }
}

int choose_conv_tap_variant(int M, int n16) {
    ConvArgs a{};
    a.M = M; a.n16 = n16; a.ksize = 3;
    Best b{-1.f, 7};
    offer_linear(b, CONV_PATH_TAP, a);
    return b.id;
}

int choose_conv_bx3_variant(const ConvArgs& a) {
    Best b{-1.f, 7};
    offer_linear(b, CONV_PATH_BX3, a);
    if (conv_bx3p_supported(a))
        for (const ConvTile& t : kBx3Tiles)
            if (t.rows && t.s3 > 0.f) b.offer(tile_score(t, a, t.s3), t.id);
    return b.id;
}

int choose_conv_tap16_variant(const ConvArgs& a) {
    const bool dbl_ok = a.ksize == 3 && (a.cin & 63) == 0 && a.cin >= 128;
    const int nch = a.cin >> 5;
    const bool patch_ok = conv_p16_supported(a);
    Best b{-1.f, 7};
    for (const ConvTile& t : kF16Tiles) {
        if (t.s3 <= 0.f) continue;
        if (t.rows) {
            if (patch_ok) b.offer(tile_score(t, a, t.s3 * (float)nch / (float)(nch + 1)), t.id);
            continue;
        }
        const bool dbl = t.family == CONV_TAP16D;
        if (dbl && !dbl_ok) continue;
        const int ntiles = (a.n16 + t.bn / 16 - 1) / (t.bn / 16);
        const float reread = 1.0f / (1.0f + 0.25f * (float)(ntiles - 1));        // input re-read per extra channel tile
        b.offer(tile_score(t, a, t.s3) * (dbl ? 1.0f : reread), t.id);
    }
    return b.id;
}

int choose_conv_h2_variant(const ConvArgs& a) {
    const int n16 = a.n16, ksize = a.ksize;
    Best b{-1.f, 220};
    offer_linear(b, CONV_PATH_H2, a);
    int& bv = b.id;
    // 1x1 layers with K >= 192 stream their activations from HBM: the three-stage activation ring (conv_tap_h2p.hip) measured
    // +2..3 % at K = 192, +7..8 % at K = 576 / 1152, -2.5 % at K = 96 (profiles/r5b_tiles_1x1_deep_ring.txt); same results
    if (ksize == 1 && a.cin >= 192 && (bv == 213 || bv == 209)) bv += 30;
    // Round 6: what bounds a long-K 1x1 layer is the LDS-DMA stream of its activation tile, requested again by every 96-channel tile
    // of a pixel tile (conv_1x1_h2s.hip: the kernel is as fast with its MFMAs compiled out).  128 x 192 tiles (8 waves, one workgroup
    // per CU, register weights) halve the requests: +10..14 % on 768 / 960 / 1152 -> 384 / 576, +4..7 % on 384 / 576 -> 384, level or
    // behind on 192-channel outputs (profiles/r6D_1x1_tile_245.txt); bitwise the same results
    if (ksize == 1 && a.w_single && n16 >= 24 && a.cin >= 384 && conv_h2s_supported(a)) bv = 245;
    // ... and the same bytes as 64 x 192 tiles of FOUR waves, two workgroups per CU (two barrier domains instead of eight waves in
    // lock step): +8..10 % over the better of the two on 192 / 384 / 576 -> 192 and 384 / 576 -> 384, level at 768 -> 384, 1152 -> 576,
    // -2 % at K = 1152 -> 384 (profiles/r6L_1x1_tile_247.txt); taken for K < 960 where 192-channel tiles fit
    if (ksize == 1 && a.w_single && n16 >= 12 && (float)(((n16 + 11) / 12) * 12) <= 1.1f * (float)n16 && a.cin >= 192 && a.cin < 960 &&
        conv_h2s_supported(a)) bv = 247;
    // The stride-2 3x3 layers request a 16 KB tile per TAP and 96-channel tile (7.4 TB/s of requests on 96 -> 192): the same tile
    // gives +10..12 % on 96 -> 192, +23..31 % on 192 -> 192 / 384 / 576 (profiles/r6F_s2_tile_246.txt); taken where 192-channel tiles
    // waste at most a fifth of their columns
    if (ksize == 3 && a.stride == 2 && n16 >= 10 && (float)(((n16 + 11) / 12) * 12) <= 1.2f * (float)n16 && conv_h2s3_supported(a)) bv = 246;
    // (as 64 x 192 four-wave tiles, two workgroups per CU: +3..5 % at 96 and 384 input channels, -1..3 % at 192 — profiles/r6N_s2_tile_248.txt)
    if (bv == 246 && a.cin != 192) bv = 248;
    if (!conv_h2p_supported(a)) return bv;
    // stride-1 3x3: every patch row whose family takes the layer (the quad kernel only where the channels fill its tiles)
    for (const ConvTile& t : kH2Tiles) {
        if (!t.rows || t.s3 <= 0.f || !family_takes(t.family, a, t.id)) continue;
        if (t.id == 323 && n16 % 6 != 0) continue;
        // h2r: no round-quantisation term — the persistent workgroups start their next tile's loads under the current tile, and
        // a 2.25-tiles-per-workgroup launch — the players graph's 192 -> 192 at 24 x 40 — still measured 461 vs 377 TFLOP/s
        const bool persistent = t.family == CONV_H2R;
        b.offer(tile_score(t, a, t.id == 325 && !a.w_single ? kH2rThreeProducts : t.s3, !persistent), t.id);
    }
    // cin % 32 == 16 (yolov8m's 48-channel P2 layers): 14 short steps per tile — there the software-pipelined schedule
    // (313: operand reads of the next step under this step's main products) measured +6..9 % although it runs 2 waves
    // per SIMD instead of 3; on whole-chunk layers it loses 10-15 % (profiles/conv_h2_sweep_r3f_pipe.txt).  Same
    // products in the same order: results do not depend on the choice.
    if (bv == 303 && (a.cin & 16)) bv = 313;
    return bv;
}

}  // namespace padel
