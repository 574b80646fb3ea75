// Internal kernel-launch interface of libpadel_hip.so (not part of the C-ABI).
// All activation tensors are fp32 NHWC in HBM: element (n, y, x, c) of a buffer with
// pixel stride `cs` lives at  base[((n*H + y)*W + x)*cs + c].  A layer reads / writes a
// channel slice [choff, choff+C) of such a buffer, which is how torch.cat / chunk of the
// YOLOv8 / TrackNet graphs are realised without ever copying.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace padel {

enum Act : int { ACT_NONE = 0, ACT_SILU = 1, ACT_RELU = 2, ACT_SIGMOID = 3, ACT_LEAKY = 4 };   // LEAKY: nn.LeakyReLU() (slope 0.01): InpaintNet's Conv1DBlock (models.py:83-93)

struct ConvArgs {
    const float* in;      // input buffer base
    const float* w;       // packed weights [Npad][Ktot], K order = (c32 chunk, tap, c16 half)
    const void* w3;       // bf16x3 kernels: the same weights pre-split, [Npad][k-step][hi|mid|lo][32 bf16] (or nullptr)
    const float* bias;    // [Npad]
    const float* res;     // optional residual buffer base (added AFTER the activation, or before it: res_pre) or nullptr
    int res_pre;          // 1 (PA_CONV_RES_PREACT): out = act(conv + bias + res) — ResNet's bottleneck join; h2 and bf16x3 kernels only
    const float* zeros;   // >= 64 bytes of zeros in HBM (source of padded taps)
    const float* in2;     // bf16x3 1x1 and patch kernels: channels [0, up_c) of the input are read from this buffer of HALF the
    int in2_cs, in2_choff, up_c;   // spatial size at [y >> 1][x >> 1] (an absorbed nn.Upsample(2)); nullptr: none; up_c % 32 == 0
    float* out;           // output buffer base
    int in_cs, in_choff;  // input pixel stride (channels) and channel offset of the slice read
    int out_cs, out_choff;
    int res_cs, res_choff;
    int H, W;             // input spatial size
    int Ho, Wo;           // output spatial size
    int cin;              // channels read (multiple of 16)
    int cout;             // real output channels (stores are masked to < cout)
    int n16;              // rows of the packed weight matrix / 16 (cout padded up to 16)
    int ksize, stride;    // 1 or 3 ; 1 or 2   (pad = ksize/2)
    int act;
    int M;                // batch * Ho * Wo
    int n_mtiles;         // ceil(M / BM)
    int n_ntiles;         // bx3 / fp16 kernels (1-D grid): channel tiles per pixel tile
    int tune;             // Tuning::tune (launch_plan.h: kTuneTilePerWorkgroup, kTunePrevGen; no kernel reads another bit)
    int tap_pd;           // 1x1 tap kernel: prefetch distance 2 or 3 (pa_engine_set_tuning "tap_pd")
    int out_f32;          // fp16 / h2 kernels only: 1 = `out` is an fp32 buffer (convs that feed the Detect/Pose decode)
    const float* oscale;  // h2 kernels: [Npad] 1 / (power-of-two scale of the weight row), applied before the bias
    unsigned* ovf_flag;   // h2 kernels: set to 1 when an output value does not fit the fp16 range (h2_common.h)
    unsigned* f16_flag;   // fp16 kernels: the same flag for the fp16 family (f16_epilogue.h), raised where a stored half was clamped or is
                          // NaN; nullptr: no guard.  A field of its own: ovf_flag stays null in the launches of fp16 graphs
    int w_single;         // h2 kernels: 1 = the m plane of the packed weights is all zero (PA_CONV_W_SINGLE): the wm x ah product, its
                          // weight requests and operand reads are skipped — two MFMAs per operand pair (same results: the product is 0)
    const void* wr;       // h2 stride-1 3x3 layers with whole chunks: the weights once more in MFMA operand order [fragment][k-step][h | m][lane][16 B]
                          // (conv_patch_h2r.hip; nullptr: no such copy)
    unsigned long long* dbg;   // tuning only (PADEL_CONV_DBG): per-workgroup s_memtime timeline, see conv_tap.hip
    // m / (Ho*Wo) and rem / Wo without an integer-division sequence (conv_tap.hip prologue): q = (umulhi(n, magic) + n) >> shift,
    // exact for 0 <= n < 2^31 (fill_fastdiv below; the conv kernels' rows satisfy n < 2^31)
    unsigned howo_magic, howo_shift, wo_magic, wo_shift;
};
inline void fill_fastdiv(unsigned d, unsigned* magic, unsigned* shift) {
    unsigned s = 0;
    while ((1ull << s) < d) ++s;
    *magic = (unsigned)((((1ull << 32) * ((1ull << s) - d)) / d) + 1ull);
    *shift = s;
}
// tuning only ("timeline"): u64 words of one workgroup's s_memtime record — header + 4 waves x ring steps x 5 stamps
constexpr int conv_dbg_words(int steps) { return 8 + 4 * steps * 5; }
constexpr int kConvDbgSteps = 64;                       // k-steps kept per wave (ring): the fp32 tap kernel (conv_tap.hip)
constexpr int kConvDbgWords = conv_dbg_words(kConvDbgSteps);

// ---- which kernel runs a conv (conv_select.cpp: host code only) -----------------------------------------------------
// The implicit-GEMM conv on v_mfma_f32_16x16x4_f32 (strict fp32: the cross-check / no-argument leg) is the tap-unrolled LDS-DMA
// ring of conv_tap.hip.  The register-staged LDS kernel of round 1 — its bitwise cross-check until round 5, 75-104 vs 109-124
// TFLOP/s (profiles/r5e_f32_tap_vs_lds.txt) — and three more retired generations live in tools/legacy_conv/ and are not
// built.  Every path has its own table of tile ids:
//   CONV_PATH_TAP  fp32 MFMA tap kernels (conv_tap.hip): ids 6, 7, 9..15, 20
//   CONV_PATH_BX3  fp32 on the bf16 matrix pipe, exact 3-way bf16 split, 6 products, fp32 accumulate (conv_tap_bx3.hip: the tap ids
//                  (3-stage ring) and + 200 (2-stage ring); conv_patch_bx3.hip: 303 / 304 / 306, stride-1 3x3 as 8 x 16-pixel patches)
//   CONV_PATH_H2   activations are fp16 PAIRS (x ~ h + m / 2048) in 16-channel groups of 64 bytes [h x 16 | m x 16], 4 bytes per
//                  channel like fp32 (cs / choff count channels); weights `w` are the pre-split planes [Npad][k-step][h | m][32 fp16],
//                  `oscale` the inverse row scales; three f16 MFMAs per operand pair (h2_common.h)
//   CONV_PATH_F16  in / w / res / out are _Float16 arrays behind the float pointers of ConvArgs (cs and choff count elements);
//                  cin % 32 == 0; weights packed [Npad][Ktot] with K order (64-channel chunk, tap, 32-channel half)
enum ConvPath : int { CONV_PATH_TAP = 0, CONV_PATH_BX3 = 1, CONV_PATH_H2 = 2, CONV_PATH_F16 = 3 };
// workgroup tile of an id: bm output pixels (a patch tile's rows x cols) x bn channels; false: not a tile of this path
bool conv_tile_shape(int path, int id, int* bm, int* bn);
// What a requested tile id runs as on a layer: the tile id AFTER every fall-through (a tile that does not cover the layer hands it
// to a sibling) and a tag for the kernel template family — tap | bx3t, bx3p | h2t (two-stage tap ring), h2d (deep ring), h2s,
// h2s3, h2p, h2q, h2r, h2v, h2w | tap16, tap16d (64-channel k-steps), p16, p16q (profile rows, pa_model_profile_text columns 12 / 13)
struct ConvLaunched { int tile; const char* family; };
enum ConvFamily : int { CONV_TAP, CONV_BX3T, CONV_BX3P, CONV_H2T, CONV_H2D, CONV_H2S, CONV_H2S3, CONV_H2P, CONV_H2Q, CONV_H2R, CONV_H2W, CONV_H2V,
                        CONV_TAP16, CONV_TAP16D, CONV_P16, CONV_P16Q };      // the tags above, in this order (conv_family_name)
const char* conv_family_name(ConvFamily f);
// false: the layer or the tile is not covered.  With a.in2 set (an absorbed nn.Upsample(2); h2 and bf16x3) only kernels that read it resolve.
bool resolve_conv(int path, const ConvArgs& a, int requested, ConvLaunched* out, ConvFamily* family = nullptr);
int conv_timeline_words(const ConvLaunched& k, int ksize);      // u64 words per record of the timeline instantiation of kernel `k` on a ksize layer; 0: it has none
// the launcher of the family resolve_conv named, with the tile it named (conv_tap.hip)
hipError_t launch_conv_family(ConvFamily f, const ConvArgs& a, int tile, hipStream_t s);
// conv_tap.hip reads up to 128 B past the last chunk of a pixel / weight row, so every buffer a conv reads is
// allocated with kConvReadSlack extra bytes
constexpr size_t kConvReadSlack = 512;
// per-layer tile choice (no a.in2: the engine attaches an absorbed upsample after the choice)
int choose_conv_tap_variant(int M, int n16);
int choose_conv_bx3_variant(const ConvArgs& a);
int choose_conv_h2_variant(const ConvArgs& a);
int choose_conv_tap16_variant(const ConvArgs& a);
// h2: does some kernel read this conv's weights in MFMA operand order (ConvArgs::wr)?  w_single: the op's PA_CONV_W_SINGLE flag
bool conv_wants_operand_copy(int ksize, int stride, int cin, bool w_single);
int h2_ksteps(int cin, int ksize);                                // k-steps (128-byte [h | m] records per weight row) of a layer in the packed h2 blob
size_t conv_h2r_copy_bytes(int n16, int cin, int ksize);          // bytes of the operand-order copy of one conv's weights (both planes)

// One launcher per family: launches exactly `tile` (an id of the family's rows in the table) — no fall-through.  A
// hipErrorNotSupported for a tile resolve_conv named is a bug, not a refusal.
hipError_t launch_conv_tapt(const ConvArgs& a, int tile, hipStream_t s);       // conv_tap.hip
hipError_t launch_conv_bx3t(const ConvArgs& a, int tile, hipStream_t s);       // conv_tap_bx3.hip (a.in2: tiles 209 / 213 / 220 only)
hipError_t launch_conv_bx3p(const ConvArgs& a, int tile, hipStream_t s);       // conv_patch_bx3.hip
hipError_t launch_conv_h2t(const ConvArgs& a, int tile, hipStream_t s);        // conv_tap_h2.hip
hipError_t launch_conv_h2d(const ConvArgs& a, int tile, hipStream_t s);        // conv_tap_h2p.hip: 239, 243
hipError_t launch_conv_h2s(const ConvArgs& a, int tile, hipStream_t s);        // conv_1x1_h2s.hip: 244 (4 waves), 245 (8 waves, one workgroup per CU), 247 (four waves)
hipError_t launch_conv_h2s3(const ConvArgs& a, int tile, hipStream_t s);       // ... 246 (8 waves), 248 (four waves)
hipError_t launch_conv_h2p(const ConvArgs& a, int tile, hipStream_t s);        // conv_patch_h2.hip: 303, 304, 313
hipError_t launch_conv_h2q(const ConvArgs& a, int tile, hipStream_t s);        // conv_patch_h2q.hip: 323
hipError_t launch_conv_h2r(const ConvArgs& a, int tile, hipStream_t s);        // conv_patch_h2r.hip: 324 (a wave 4 rows x 3 fragments), 325 (x 2)
hipError_t launch_conv_h2w(const ConvArgs& a, int tile, hipStream_t s);        // conv_patch_h2w.hip: 341..343
hipError_t launch_conv_h2v(const ConvArgs& a, int tile, hipStream_t s);        // conv_patch_h2v.hip: 341..343
hipError_t launch_conv_t16(const ConvArgs& a, int tile, hipStream_t s);        // conv_tap16.hip: families tap16 and tap16d
hipError_t launch_conv_p16(const ConvArgs& a, int tile, hipStream_t s);        // conv_patch16.hip: families p16 (30x) and p16q (32x)
hipError_t launch_h2r_repack(const float* w, void* wr, int n16, int cin, int ksize, hipStream_t s);
// *flag |= 1 when any m-plane bit of `rows_x_ksteps` packed 128-byte k-step records is set (the PA_CONV_W_SINGLE promise, checked once per model)
hipError_t launch_h2_mplane_check(const float* w, long long rows_x_ksteps, unsigned* flag, hipStream_t s);

struct StemArgs {
    const uint8_t* in;    // net input u8 NHWC4 [B][H][W][4]
    const float* w;       // [cout][27] (ky,kx,c) fused BN
    const float* bias;    // [cout]
    float* out;           // NHWC fp32 (or fp16 with out_f16), pixel stride out_cs
    int out_cs, out_choff;
    int H, W, Ho, Wo, cout, B;
    int out_f16;          // 1: `out` is a _Float16 buffer (fp16 models; the stem itself computes in fp32); 2: h2 pairs
    unsigned* ovf_flag;   // out_f16 != 0: raised when a value does not fit the fp16 range (out_f16 == 1: on the value the clamp sees)
    unsigned howo_magic, howo_shift, wo_magic, wo_shift;   // filled by launch_stem (fill_fastdiv): pixel index -> (n, oy, ox)
    const void* opw;      // stem_l1_h2.hip: the stem's weights as MFMA operands + inverse row scales (launch_stem_l1_operands; nullptr: none)
};
hipError_t launch_stem(const StemArgs& a, hipStream_t s);
struct ConvArgs;
// stem_l1_h2.hip: stem + the 3x3 stride-2 conv behind it, one kernel.  Whether it covers a pair reads the two argument structs and
// nothing else (launch_plan.cpp: host code, asked where the launch is planned and once more by the launcher)
bool stem_l1_h2_supported(const StemArgs& st, const ConvArgs& cv);
// ... and, as a third phase of the same kernel, the 1x1 stride-1 conv `cv1` that is the only reader of that conv's map (model.2.cv1
// of a YOLOv8 graph; graph_plan.h: stem_cv1_fusable): the register-weights instantiations, two-product layers, SiLU behind layer 1,
// cv1 over all of layer 1's 2c channels with 2c outputs and an operand-order weight copy.  Layer 1's map is not written then
bool stem_l1_cv1_h2_supported(const StemArgs& st, const ConvArgs& cv, const ConvArgs& cv1);
hipError_t launch_stem_l1_h2(const StemArgs& st, const ConvArgs& cv, const ConvArgs* cv1, hipStream_t s);      // cv1 == nullptr: two phases
// the stem operand block of its register-weights instantiations (cout = 16 / 32 / 48): per 16-channel fragment 2 KB [h | m][lane][16 B]
// of w / 255 row-scaled and split into fp16 pairs, then the cout inverse row scales.  Built from the blob's [cout][27] stem weights
size_t stem_l1_operand_bytes(int cout);                                   // launch_plan.cpp
hipError_t launch_stem_l1_operands(const float* w, int cout, void* blk, hipStream_t s);

// SPPF: three chained MaxPool2d(5,1,2) of slice [choff, choff+c) written to the next three slices
// (f16 == 1 in these three: the buffers hold _Float16 elements; cs / choff / c count elements, c % 8 == 0;
//  f16 == 2: h2 pairs in 16-channel groups, 4 bytes per channel, cs / choff / c count channels)
hipError_t init_misc_kernels();
hipError_t launch_sppf_pool(float* buf, int cs, int choff, int c, int B, int H, int W, hipStream_t s, int f16 = 0, int fused = 1);
// nearest x2 upsample of a slice into a slice of a buffer with twice the spatial size
hipError_t launch_upsample2x(const float* in, int in_cs, int in_choff, float* out, int out_cs, int out_choff,
                             int c, int B, int H, int W, hipStream_t s, int f16 = 0);
// fp32 NHWC -> h2 pairs (n_floats % 16 == 0: whole 16-channel groups)
hipError_t launch_h2_encode(const float* in, float* out, long long n_floats, unsigned* ovf_flag, hipStream_t s);
// MaxPool2d(2,2)
hipError_t launch_maxpool2(const float* in, int in_cs, int in_choff, float* out, int out_cs, int out_choff,
                           int c, int B, int H, int W, hipStream_t s, int f16 = 0);

// ---- ResNet-50 court-keypoint regressor (resnet_ops.hip) ----------------------------------------------
// conv1: Conv 7x7 stride 2 pad 3, 3 -> 64, + bias (BatchNorm folded) + ReLU straight from the u8 NHWC4 network input.  Every byte
// goes through `lut` ([3][256] fp32: the normalised value of colour c, byte b) — the padding is zero in NORMALISED space, which is
// why the normalisation cannot be folded into the weights.  w: [148][64] fp32, row k = (ky * 7 + kx) * 3 + c (row 147: zeros).
struct Stem7Args {
    const uint8_t* in;    // [B][H][W][4] u8
    const float* w;       // [148][64]
    const float* bias;    // [64]
    const float* lut;     // [3][256]
    float* out;           // fp32 or h2 pairs, pixel stride out_cs
    int out_cs, out_choff;
    int H, W, Ho, Wo, B;
    int act;              // ACT_RELU | ACT_NONE
    int out_h2;           // 1: h2 pairs
    unsigned* ovf_flag;
    unsigned howo_magic, howo_shift, wo_magic, wo_shift;   // filled by launch_stem7
};
hipError_t launch_stem7(const Stem7Args& a, hipStream_t s);
// MaxPool2d(3, 2, 1) of an H x W map into an Ho x Wo one (padding = -inf: absent taps are skipped); h2 = 1: h2 pairs ordered like
// every other h2 pool (value, then pair bits); c % 4 == 0 (fp32) / c, choff % 4 == 0 inside 16-channel groups (h2)
hipError_t launch_maxpool3s2(const float* in, int in_cs, int in_choff, float* out, int out_cs, int out_choff,
                             int c, int B, int H, int W, int Ho, int Wo, hipStream_t s, int h2);
// global average pool over the HW pixels of c channels (fp32 sum in pixel order / HW), then nout <= 64 outputs of a linear layer
// (w [nout][c], fp32 FMA chains, one wave per output) + bias -> logits [B][nout], and their sigmoid -> probs [B][nout]
hipError_t launch_gap_fc(const float* in, int in_cs, int in_choff, int c, int B, int HW, const float* w, const float* bias, int nout,
                         float* logits, float* probs, hipStream_t s, int h2);
constexpr int kGapFcMaxC = 4096, kGapFcMaxOut = 64;

// ---- YOLO11 (yolo11_ops.hip) ---------------------------------------------------------------------------
// depthwise Conv 3x3 stride 1 pad 1 over a C-channel slice (C, choffs, pixel strides % 4 == 0): w [9][C] fp32 (tap ky * 3 + kx,
// BatchNorm folded), bias [C]; act ACT_NONE | ACT_SILU; res (optional): a slice added after the activation.  h2 = 1: in / res are
// h2 pairs and so is out, unless out_f32 (a head map).  Absent taps are skipped, not read.
struct DwConvArgs {
    const float* in;
    const float* w;
    const float* bias;
    const float* res;     // nullptr: none
    float* out;
    int in_cs, in_choff, out_cs, out_choff, res_cs, res_choff;
    int C, B, H, W;
    int act;
    int h2, out_f32;
    unsigned* ovf_flag;
};
hipError_t launch_dwconv3(const DwConvArgs& a, hipStream_t s);
// PSA attention over the N = H * W tokens of one map: per image and head, out = softmax_keys((q^T k) * scale) applied to v.
// qkv (pixel stride cs): q of head h at channels q_choff + h * kd, k at k_choff + h * kd, v at v_choff + h * hd; out: hd channels
// per head at out_choff + h * hd.  kd = 32 and hd = 64 only (hipErrorNotSupported otherwise).
struct AttnArgs {
    const float* qkv;
    float* out;
    int cs, q_choff, k_choff, v_choff, out_cs, out_choff;
    int heads, kd, hd, N, B;
    float scale;
    int h2, out_f32;
    unsigned* ovf_flag;
};
hipError_t launch_psa_attn(const AttnArgs& a, hipStream_t s);

// ---- preprocessing -----------------------------------------------------------------
struct LetterboxArgs {
    const uint8_t* src;   // [B][h0][w0][3] u8
    uint8_t* dst;         // [B][nh][nw][4] u8 (4th byte 0)
    int B, h0, w0;        // source size
    int rw, rh;           // resized (unpadded) size
    int top, left;        // letterbox offsets
    int nh, nw;           // network input size
    int mode;             // 0 copy, 1 exact 2x2 area, 2 fixed-point bilinear (cv2 INTER_LINEAR)
    int reverse;          // 1: dst channel c = src channel 2-c
    const int32_t* xtab;  // mode 2: [rw][3] = {sx, a0, a1}
    const int32_t* ytab;  // mode 2: [rh][3] = {sy, b0, b1}
};
hipError_t launch_letterbox(const LetterboxArgs& a, hipStream_t s);

// YUV 4:2:0 -> packed BGR (yuv_convert.hip): n frames at src + i * frame_stride -> n packed frames at dst + i * h * w * 3.
// The caller (pa_yuv420_to_bgr) has checked the geometry; the launcher only picks the vector or the byte instantiation.
struct YuvArgs {
    const uint8_t* src;   // HBM, no alignment guarantee
    uint8_t* dst;
    int n, h, w;          // h, w even
    int nv12;             // 1: interleaved UV rows at off_u (off_v = off_u + 1), 0: I420 planes at off_u / off_v
    int pitch_y, pitch_c; // bytes per luma / chroma row
    int off_u, off_v;     // bytes from the start of a frame
    long long frame_stride;
    int y_off, cy, cvr, cug, cvg, cub;
};
bool yuv_vector_path_ok(const YuvArgs& a);              // every address of this launch allows dword / 16-bit accesses
hipError_t launch_yuv420_to_bgr(const YuvArgs& a, hipStream_t s, int* vec_out = nullptr);      // *vec_out: 1 vector path, 0 byte path

// Marks on packed BGR frames, written as BGR or YUV 4:2:0 (render.hip).  The caller (pa_render) has checked the marks and the
// geometry (render_check.cpp) and staged the RESOLVED mark list (render_marks.h) and first[] in HBM.
struct RenderArgs {
    const uint8_t* src;   // n packed BGR frames
    uint8_t* dst;
    const void* marks;    // pa_mark[first[n]], resolved
    const void* boxes;    // int16 x0, y0, x1, y1 per mark: mark_bbox of each, what the tiles cull by (8 bytes instead of 32)
    const int32_t* first; // [n + 1]
    int n, h, w;
    int out;              // 0 BGR, 1 NV12, 2 I420
    int in_place;         // BGR output with dst == src: a tile no mark meets stores nothing
    int pitch_y, pitch_c, off_u, off_v;
    long long frame_stride;
    int y_off, yr, yg, yb, ur, ug, ub, vr, vg, vb;
#ifdef PADEL_RENDER_PROBE
    unsigned long long* probe;   // tools: {cull, apply, whole kernel} shader-clock cycles summed over the workgroups, and their count
#endif
};
bool render_vector_path_ok(const RenderArgs& a);        // every address of this launch allows dword / 16-bit accesses
hipError_t launch_render(const RenderArgs& a, hipStream_t s, int* vec_out = nullptr);          // *vec_out: 1 vector path, 0 byte path
// the same pass followed by a scale x scale box average (scale 2..4 dividing a.w and a.h): a.h x a.w is the source, the geometry
// fields describe the (a.h / scale) x (a.w / scale) output, in_place is 0
bool render_scaled_vector_path_ok(const RenderArgs& a, int scale);
hipError_t launch_render_scaled(const RenderArgs& a, int scale, hipStream_t s, int* vec_out = nullptr);

// Perspective resample of packed BGR frames (warp.hip).  The caller (pa_warp_perspective) has checked the call (warp_check.cpp) and
// staged the matrices and the valid words in HBM; the launcher only picks the 16-byte or the byte instantiation.
struct WarpArgs {
    const uint8_t* src;   // n packed BGR frames of h x w
    uint8_t* dst;         // n packed BGR frames of oh x ow, not overlapping src
    const double* m;      // [n][9], canvas -> source
    const int32_t* valid; // [n]
    int n, h, w, oh, ow;
    uint32_t fill;        // B | G << 8 | R << 16
};
bool warp_vector_path_ok(const WarpArgs& a);            // ow a multiple of 16 and dst 16-byte aligned
hipError_t launch_warp(const WarpArgs& a, hipStream_t s, int* vec_out = nullptr);            // *vec_out: 1 16-byte path, 0 byte path

// Player density maps on the top-down canvases (heat.hip).  The caller (pa_heat_accumulate) has checked the call (heat_check.cpp) and
// staged everything but the canvases and the state in HBM; the launcher only picks the 16-byte or the byte instantiation.
struct HeatArgs {
    uint8_t* canvas;        // n packed BGR canvases of oh x ow, blended in place
    uint32_t* state;        // planes maps of oh x ow, carried from call to call; not overlapping the canvases
    const uint32_t* lut;    // [256] B | G << 8 | R << 16 per level
    const int32_t* first;   // [n + 1]
    const int32_t* valid;   // [n]
    const int32_t* box;     // [n][4] x0, y0, x1, y1, inclusive: the pixels the discs of frame i can reach (x0 > x1: none)
    const int32_t* pts;     // [first[n]][3] x, y, plane
    int n, oh, ow, planes, r, alpha, show_mask;
    uint32_t full;
};
bool heat_vector_path_ok(const HeatArgs& a);            // ow a multiple of 16, canvases and state 16-byte aligned
hipError_t launch_heat(const HeatArgs& a, hipStream_t s, int* vec_out = nullptr);            // *vec_out: 1 16-byte path, 0 byte path

// Pillow-style separable resample pass over u8 images (coefficients precomputed on host):
// out[b][y][x][c] = clip8((sum_k coef[o][k] * in[...lo[o]+k...] + (1<<21)) >> 22)
struct ResamplePassArgs {
    const uint8_t* in; uint8_t* out;
    int B, in_h, in_w, in_c;      // input dims (in_c = 3 or 4 bytes per pixel)
    int out_h, out_w, out_c;      // output dims
    int vertical;                 // 0: horizontal pass (out_h == in_h), 1: vertical (out_w == in_w)
    const int32_t* bounds;        // [out][2] = {lo, n}
    const int32_t* coefs;         // [out][ksize]
    int ksize;
    int reverse;                  // reverse the 3 colour channels while writing
};
hipError_t launch_resample_pass(const ResamplePassArgs& a, hipStream_t s);

// ---- detect / pose post-processing -------------------------------------------------
struct HeadLevel { const float* buf; int H, W, stride, anchor0; };
struct DecodeArgs {
    HeadLevel lv[3];
    int cs;               // head pixel stride = 64 + nc + nk
    int nc, nk, kdim;
    int A, B;
    float conf;
    const int32_t* classes; int n_classes;   // device array or nullptr
    // outputs: per image candidate list
    float* cand;          // [B][A][6]  x1,y1,x2,y2 (net px), score, cls
    int32_t* cand_idx;    // [B][A] anchor index
    int32_t* cand_cnt;    // [B]
};
hipError_t launch_decode(const DecodeArgs& a, hipStream_t s);

// The fused head tail of h2 Detect / Pose models (head_tail_h2.hip): per level the last 1x1 convs of the box / class / keypoint
// branches (graph_plan.h: HeadTail) and the decode in ONE launch.  The head maps are not written, except the nk keypoint values of
// the anchors that pass, at their place in the map (where nms_kernel reads them).  Candidates are bitwise those of the convs
// followed by decode_kernel.
struct HeadTailConv {
    const float* in;      // h2 pairs, pixel stride in_cs channels, slice at in_choff
    const float* w;       // packed planes [npad][k-step][h | m][32 fp16]
    const float* bias;    // [npad]
    const float* oscale;  // [npad]
    int in_cs, in_choff, cin, n16;
};
struct HeadTailArgs {
    DecodeArgs d;         // lv[l].buf: the head map of level l (keypoint rows of passing anchors only)
    HeadTailConv cv[3][3];   // [level][box 64, class nc, keypoint nk]; cv[l][2].in == nullptr: detect
    int w_single;         // every conv's m plane is all zero (ConvArgs::w_single): two products per operand pair
    int wg_end[3];        // filled by the launcher: workgroups [wg_end[l - 1], wg_end[l]) walk level l
};
bool head_tail_h2_supported(const HeadTailArgs& a);      // the k-step counts have an instantiation, the weights fit the LDS
hipError_t init_head_tail_kernels();                     // per engine: the kernels' dynamic-LDS limit on the current device
hipError_t launch_head_tail_h2(const HeadTailArgs& a, hipStream_t s);

struct NmsArgs {
    const float* cand; const int32_t* cand_idx; const int32_t* cand_cnt;
    uint64_t* keys;       // [B][P2] sort scratch (P2 = pow2 >= A)
    int32_t* order;       // [B][A] scratch
    uint8_t* supp;        // [B][A] scratch
    HeadLevel lv[3];
    int cs, nc, nk, kdim, A, B, P2;
    float iou; int max_det; int max_nms;
    // scale_boxes / scale_coords
    float gain; float pad_x, pad_y;        // rounded pads for boxes
    float kpad_x, kpad_y;                  // unrounded pads for keypoints
    float w0, h0;
    float* out_boxes;     // [B][max_det][6]
    float* out_kpts;      // [B][max_det][K*kdim] or nullptr
    int32_t* out_cnt;     // [B]
};
hipError_t launch_nms(const NmsArgs& a, hipStream_t s);

// ---- ball path (TrackNet) ---------------------------------------------------------------
struct BallAssembleArgs {
    const uint8_t* median;   // [H][W][3] RGB, resized background
    const uint8_t* frames;   // ring [ring][H][W][3] RGB, resized frames
    const float* lut;        // [256] u8 -> float(double(u)/255)
    float* out;              // [B][H][W][32] fp32, 16-byte aligned (or fp16 / h2 pairs: out_f16)
    int B, H, W, ring, first_slot;
    int out_f16;             // 0: fp32; 1: `out` is a _Float16 buffer (fp16 graphs), pad channels 27..31 written as zero;
                             // 2: the TrackNet graph is an h2 graph (h2_common.h)
};
hipError_t launch_ball_assemble(const BallAssembleArgs& a, hipStream_t s);

struct BallEnsembleArgs {
    const float* Y;          // [rows][H][W][cs] window outputs (sigmoid heat maps), slot = channel
    int cs, H, W;
    const int32_t* row0;     // [nout] first buffer row of each output frame
    const int32_t* mode;     // [nout] 0 weighted, 1 mean
    const float* div;        // [nout] divisor for mode 1
    float w[8];              // ensemble weights
    float threshold;
    float* heat;             // [nout][H][W] or nullptr
    uint8_t* mask;           // [nout][H][W] 255 / 0
};
hipError_t launch_ball_ensemble(const BallEnsembleArgs& a, int nout, hipStream_t s);

struct BallLocateArgs {
    const uint8_t* mask;     // [nout][H][W] 255 / 0
    int32_t* label;          // scratch [nout][H][W]
    int32_t* bbox;           // scratch [nout][4][H][W]
    int32_t* rect;           // out [nout][4] = x, y, w, h  (w = -1: foreground list overflow)
    int H, W;
};
hipError_t launch_ball_locate(const BallLocateArgs& a, int nout, hipStream_t s);
// K11: per-byte median over N BGR frames -> RGB background (np.median + uint8 truncation); keep_bgr: the output stays BGR
hipError_t launch_median(const uint8_t* frames, int N, long long frame_bytes, uint8_t* out_rgb, hipStream_t s, bool keep_bgr = false);

// Frame statistics against a reference image and the previous frame (frame_activity.hip; the specification: include/padel_hip.h).
// The caller (pa_frame_activity) has checked the arguments (activity_check.cpp) and chosen band_rows.
struct ActivityArgs {
    const uint8_t* frames;   // n packed BGR frames
    const uint8_t* ref;      // one frame
    const uint8_t* prev;     // the frame before frames[0], or nullptr
    int n, h, w;
    int x0, y0, x1, y1;      // the roi
    int tau;
    int band_rows, bands;    // workgroup (band, frame) takes roi rows [y0 + band * band_rows, ...): activity_check.h
    uint32_t* slab;          // [n][bands][3] partial sums: sad_ref, changed, sad_prev
    unsigned long long* out; // [n][3]
};
hipError_t launch_frame_activity(const ActivityArgs& a, hipStream_t s);

// Colour histograms of rectangles of BGR frames (box_histogram.hip; the specification: include/padel_hip.h).  The caller
// (pa_box_histograms) has checked the arguments (box_histogram_check.cpp); k >= 1.
struct BoxHistArgs {
    const uint8_t* frames;   // packed BGR frames of h x w
    const int32_t* rects;    // [k][5] on the device: frame, x0, y0, x1, y1
    uint32_t* out;           // [k][512] on the device, 8-byte aligned
    int h, w, k;
};
hipError_t launch_box_histograms(const BoxHistArgs& a, hipStream_t s);

}  // namespace padel
