/* libpadel_hip.so — C-ABI of the MI355X (gfx950) inference engine behind the reference's trackers/.
 *
 * The reference is pure Python and has no FFI; the boundary this library replaces is the call the
 * tracker plugins make into their numeric engines:
 *
 *   - `self.model.predict(sample, conf, iou, imgsz, device, classes)` on an `ultralytics.YOLO`
 *       detect model  — trackers/players_tracker/players_tracker.py:351-359   -> pa_yolo_infer()
 *       pose model    — trackers/players_keypoints_tracker/players_keypoints_tracker.py:285-292
 *                       (preceded by the PIL resize of :260-266)               -> pa_yolo_infer()
 *   - `YOLO(model_path)` / `self.model.to(device)` — players_tracker.py:303,338-339 -> pa_model_create()
 *   - `tracknet(x)` on the 27-channel window stack — trackers/ball_tracker/ball_tracker.py:445-446
 *                                                                              -> pa_tracknet_infer()
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer and the
 * library never keeps a caller pointer past return; every call is synchronous at this boundary (the
 * exceptions: the pa_yolo_submit / pa_yolo_wait pair and the stream-ordered pa_yuv420_to_bgr / pa_render below); one
 * engine per GPU, not thread-safe; return 0 on success, non-zero on failure with the message in
 * pa_last_error().  The Python binding (`padel_analytics_amd/engine.py`, ctypes) is the only caller.
 */
#ifndef PADEL_HIP_H
#define PADEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pa_engine pa_engine;
typedef struct pa_model pa_model;

#define PA_ABI_VERSION 5

/* ---- graph description (built on the host from a state_dict; see padel_analytics_amd/graph.py) ---- */

enum pa_op_kind {
    PA_OP_STEM = 1,       /* model.0: Conv 3x3 s2 + SiLU straight from the u8 network input      */
    PA_OP_CONV = 2,       /* Conv kxk (k in 1,3; stride 1,2) + bias + act (+ residual)           */
    PA_OP_SPPF_POOL = 3,  /* three chained MaxPool2d(5,1,2): slice c -> slices c+1..c+3          */
    PA_OP_UPSAMPLE2X = 4, /* nearest x2 of a slice into a slice of a buffer one level finer      */
    PA_OP_MAXPOOL2 = 5,   /* MaxPool2d(2,2) into a buffer one level coarser                      */
    /* ResNet-50 (the court-keypoint regressor, trackers/keypoints_tracker/keypoints_tracker.py:158-168): */
    PA_OP_STEM7 = 6,      /* conv1: Conv 7x7 s2 p3, 3 -> 64 (cout = 64) + bias + ReLU straight from the u8 network input of
                             pa_resnet_infer; w_off: [148][64] fp32, row (ky * 7 + kx) * 3 + c, row 147 zero; `reserved`: offset of
                             the [3][256] fp32 table byte -> normalised value (ToTensor + Normalize; padding is zero in THAT space) */
    PA_OP_MAXPOOL3S2 = 7, /* MaxPool2d(3, 2, 1) into a buffer one level coarser (padding = -inf); fp32 and h2 storage          */
    PA_OP_GAP_FC = 8,     /* mean over the map of the cin-channel input slice (fp32), then cout <= 64 outputs of a linear layer
                             (w_off: [cout][cin], b_off: [cout], fp32 FMA) and their sigmoid (act = PA_ACT_SIGMOID): cout logits and
                             cout probabilities per image, kept by the model (pa_resnet_infer / pa_resnet_read_fc), not in a buffer:
                             out_buf = in_buf.  One per graph                                                                   */
    /* YOLO11 (ultralytics 8.3's default family: C3k2 / C2PSA backbone, depthwise class branch in the head): */
    PA_OP_DWCONV3 = 9,    /* depthwise Conv 3x3 s1 p1 over a cin = cout channel slice (ksize 3, stride 1) + bias + act (NONE | SILU)
                             (+ residual slice, added after the activation); w_off: [9][cin] fp32, tap ky * 3 + kx, BatchNorm folded;
                             b_off: [cin]; npad = cin.  fp32 and h2 storage; the slices read and written must not overlap            */
    PA_OP_PSA_ATTN = 10   /* C2PSA's spatial self-attention over the H * W tokens of one map: per image and head
                             out = softmax_keys((q^T k) * kd^-1/2) applied to v.  stride = heads, ksize = kd (32), npad = hd (64): nothing
                             else is implemented.  The input slice (cin = heads * (2 kd + hd)) holds [q of all heads | k of all heads |
                             v of all heads], head h's q at in_choff + h * kd; the output slice has cout = heads * hd channels.  No
                             weights.  fp32 and h2 storage                                                                            */
};

enum pa_act { PA_ACT_NONE = 0, PA_ACT_SILU = 1, PA_ACT_RELU = 2, PA_ACT_SIGMOID = 3, PA_ACT_LEAKY = 4 /* nn.LeakyReLU(0.01): InpaintNet, reference trackers/ball_tracker/models.py:83-93 */ };

/* activation buffer: fp32 NHWC, spatial size = network input >> level, `channels` floats per pixel */
typedef struct pa_buf_desc {
    int32_t level;
    int32_t channels;
} pa_buf_desc;

typedef struct pa_op_desc {
    int32_t kind;
    int32_t in_buf, in_choff, cin;      /* slice read  (cin multiple of 16 for PA_OP_CONV)          */
    int32_t out_buf, out_choff, cout;   /* slice written (cout = real channels)                     */
    int32_t ksize, stride, act;
    int32_t res_buf, res_choff;         /* residual slice added after the activation (before it: PA_CONV_RES_PREACT); res_buf < 0: none */
    int32_t npad;                       /* PA_OP_CONV: rows of the packed weight matrix (multiple of 16) */
    int32_t reserved;                   /* PA_OP_CONV, fp32 models: offset (in floats, > 0) of the same weights pre-split
                                           into three bf16 planes for the bf16x3 kernels, [npad][k-step][hi|mid|lo][32];
                                           0: not provided.  PA_DTYPE_H2 models: offset (> 0) of the conv's npad per-output-
                                           channel inverse weight-row scales (fp32)                                  */
    int64_t w_off, b_off;               /* offsets (in floats) of packed weights / bias in the blob */
    int32_t flags;                      /* PA_OP_CONV of PA_DTYPE_H2 models: PA_CONV_W_SINGLE = the correction (m) plane of the packed
                                           weights is all zero — the weights are fp16 numbers (what an Ultralytics checkpoint stores)
                                           times the row's power of two, BatchNorm's scale travels in the per-channel output scale
                                           instead — so the kernels skip the wm x ah product: TWO MFMAs per operand pair, not three.
                                           Results do not depend on the flag (the skipped product is exactly zero).  ABI v4
                                           PA_CONV_RES_PREACT (any PA_OP_CONV with a residual slice): out = act(conv + bias + residual)
                                           instead of act(conv + bias) + residual — the join of a ResNet bottleneck.  Implemented by the
                                           h2 and the bf16x3 kernels; fp16 models are refused at pa_model_create, the fp32-MFMA tap
                                           kernels (tuning impl = 0) fail the inference call: nobody applies the other order silently */
    int32_t pad_;
} pa_op_desc;
#define PA_CONV_W_SINGLE 1
#define PA_CONV_RES_PREACT 4

enum pa_task { PA_TASK_DETECT = 0, PA_TASK_POSE = 1, PA_TASK_TRACKNET = 2, PA_TASK_RESNET = 3 /* pa_resnet_infer; head_buf[0] optional (tests) */ };

/* PA_DTYPE_F32: the parity path (fp32 storage, fp32 MFMA: what the reference computes with half=False).
 * PA_DTYPE_F16 (detect / pose only; BASELINE configs[4]): activations and conv weights are fp16, accumulation fp32
 * (v_mfma_f32_16x16x32_f16), biases / stem weights / the Detect-Pose head maps (head_buf) stay fp32; conv weights sit
 * in the blob as fp16 [npad][Ktot] with K order (64-channel chunk, tap, 32-channel half), cin % 32 == 0,
 * w_off still counts 4-byte blob words.  Stored halves are saturated (no infinity reaches HBM), and every kernel that turns an
 * fp32 value x into a stored half of an activation buffer (the conv epilogues, the stem) raises the model's overflow flag iff
 * !(|x| <= 65504), tested on x just before the clamp, behind the residual add: NaN raises, exactly +-65504 does not.  The fp32
 * head maps store x itself and raise nothing.  The caller repeats such a call on a PA_DTYPE_H2 or PA_DTYPE_F32 model.
 * PA_DTYPE_H2 (the fast fp32-equivalent path): every activation is an fp16 PAIR (x ~ h + m / 2048, 22-23 significant
 * bits) stored in 16-channel groups of 64 bytes [h x 16 | m x 16] — 4 bytes per channel like fp32 — written once by its
 * producer; conv weights sit at w_off as pre-split planes [npad][k-step][h | m][32 fp16] of the row-scaled weights, the
 * inverse row scales at `reserved`; a product is three f16 MFMAs instead of the six bf16 ones of the PA_DTYPE_F32 default
 * (csrc/h2_common.h).  Biases, stem weights, head maps and the TrackNet heat map stay fp32.  Values beyond the fp16
 * range (|x| > 65504) raise the model's overflow flag (pa_model_take_overflow): the caller repeats the call on a
 * PA_DTYPE_F32 model.                                                                                         */
enum pa_dtype { PA_DTYPE_F32 = 0, PA_DTYPE_F16 = 1, PA_DTYPE_H2 = 2 };

typedef struct pa_model_desc {
    int32_t task;
    int32_t nc;                 /* classes (detect / pose)                                          */
    int32_t nk, kpt_dim;        /* pose: nk = K * kpt_dim                                           */
    int32_t n_bufs;
    const pa_buf_desc* bufs;
    int32_t n_ops;
    const pa_op_desc* ops;
    int32_t head_buf[3];        /* detect/pose: per-level head maps, channels >= 64 + nc + nk (pixel stride);
                                   tracknet: head_buf[0] = output heat-map buffer                   */
    int32_t in_channels;        /* tracknet: channels of the fp32 input buffer (buffer 0)           */
    int32_t dtype;              /* enum pa_dtype: storage type of activations and conv weights      */
} pa_model_desc;

/* ---- engine ---- */
int pa_abi_version(void);
int pa_device_count(void);
int pa_engine_create(int device_id, pa_engine** out);
void pa_engine_destroy(pa_engine* eng);
/* message of the last failure on this engine (eng may be NULL for creation failures) */
const char* pa_last_error(pa_engine* eng);
int pa_engine_synchronize(pa_engine* eng);

/* raw device memory helpers (bench keeps frames resident in HBM with these) */
int pa_device_malloc(pa_engine* eng, size_t nbytes, void** out_dev);
int pa_device_free(pa_engine* eng, void* dev);
/* Device bytes the library itself holds in this process at the moment, over all engines: weights, plans, lanes, ball sessions
 * and the scratch buffers of the conversion, render and JPEG calls.  Memory handed out by pa_device_malloc is the caller's and
 * is not counted, nor is page-locked host memory.  Read-only; a value that returns to where it was after a model, a session or
 * an engine is destroyed says that everything it owned was released. */
size_t pa_device_bytes_live(void);
int pa_memcpy_h2d(pa_engine* eng, void* dst_dev, const void* src_host, size_t nbytes);
int pa_memcpy_d2h(pa_engine* eng, void* dst_host, const void* src_dev, size_t nbytes);
/* host -> HBM on the engine's copy stream: does not queue behind inference launched from another host
 * thread, so the next batch of frames uploads while the current one computes (the reference decodes and
 * uploads per tracker, trackers/runner.py:215-220; the runner's fan-out mode uploads once per batch)   */
int pa_upload(pa_engine* eng, void* dst_dev, const void* src_host, size_t nbytes);

/* page-lock a caller-owned host range (hipHostRegister) so that uploads from it run at PCIe speed and overlap compute:
 * the frame source of the end-to-end-from-host path (the reference decodes into host memory, trackers/runner.py:215-220).
 * The caller keeps ownership and unregisters before freeing.                                                  */
int pa_host_register(pa_engine* eng, void* ptr, size_t nbytes);
int pa_host_unregister(pa_engine* eng, void* ptr);

/* ---- frames from a decoder: 8-bit YUV 4:2:0 (NV12 / I420) -> the packed BGR bytes every other call consumes ----
 * Nearest-neighbour chroma (each 2 x 2 block of pixels shares one U, V), 20-bit fixed point, all int32:
 *     y = max(0, Y - y_off) * cy + (1 << 19)      u = U - 128      v = V - 128
 *     R = clamp((y + cvr * v) >> 20, 0, 255)    G = clamp((y + cug * u + cvg * v) >> 20, 0, 255)    B = clamp((y + cub * u) >> 20, 0, 255)
 * (>> arithmetic).  The named coefficient tables live in padel_analytics_amd/video.py (YUV_COEFFS).
 * Offsets and pitches are bytes; offsets count from the start of a frame, frame i starts at src + i * frame_stride.  The source
 * needs NO alignment (odd pitches, padded plane heights, frames that start anywhere): the launcher takes dword loads / stores
 * when this call's pointers, pitches, offsets and stride allow it and w % 4 == 0, bytes otherwise.                       */
enum pa_yuv_layout {
    PA_YUV_NV12 = 0,      /* Y plane, then rows of interleaved U, V at off_u (off_v must be off_u + 1); pitch_c >= w */
    PA_YUV_I420 = 1       /* Y plane, U plane at off_u, V plane at off_v; pitch_c >= w / 2                           */
};
typedef struct pa_yuv_desc {
    int32_t layout;               /* enum pa_yuv_layout                      */
    int32_t pitch_y, pitch_c;
    int32_t off_u, off_v;
    int32_t reserved;             /* 0                                        */
    int64_t frame_stride;
    int32_t y_off, cy, cvr, cug, cvg, cub;
} pa_yuv_desc;
/* n frames of h x w (both even, >= 2) -> dst_bgr_dev (HBM): n packed frames at dst + i * h * w * 3.  src: HBM (src_on_device = 1)
 * or host memory.  Refused with an error, nothing launched: odd or too small w / h, n < 1, a pitch smaller than its row, planes
 * that reach into the next frame (frame_stride too small), coefficients that could leave int32.
 * ASYNCHRONOUS on the engine's compute stream — the second exception to "every call is synchronous".  A host src is first copied
 * to an engine-owned staging buffer ON THAT SAME STREAM (grown on demand, freed with the engine), then converted; the caller keeps
 * a page-locked src untouched until the stream has passed the copy (a pageable one is consumed before the call returns).
 * INVARIANT: everything that later reads or overwrites dst, src in HBM, or the staging buffer is ordered behind this call by that
 * one stream, as in pa_yolo_infer's own host path: a following pa_yolo_infer / pa_yolo_submit / pa_resnet_infer / pa_ball_feed on
 * dst sees the converted frames, and the next conversion into the same dst waits for the readers queued before it.  That is what
 * makes ONE staging buffer safe under the trackers' submit / collect pipelining.  Work on another stream (pa_upload's copy
 * stream, another engine) is NOT ordered: pa_engine_synchronize first.                                                    */
int pa_yuv420_to_bgr(pa_engine* eng, const uint8_t* src, int src_on_device, int n, int h, int w,
                     const pa_yuv_desc* d, uint8_t* dst_bgr_dev);
/* tests / tools: which instantiation the last successful pa_yuv420_to_bgr of this engine launched — 1 vector path, 2 byte path,
 * 0 none yet                                                                                                          */
int pa_yuv_last_path(pa_engine* eng);

/* ---- frames to an encoder: marks drawn on packed BGR frames in HBM, written as BGR or as 8-bit YUV 4:2:0 (csrc/render.hip) ----
 * One pass: source BGR -> marks applied in registers, in list order -> BGR or NV12 / I420.  Parity with cv2 / supervision drawing
 * is NOT pinned (neither is installed); the integer rules below are the specification.  Their code is csrc/render_marks.h (host and
 * device), their readable twin padel_analytics_amd/render.py (render_host).
 *
 * A mark is opaque (PA_MARK_BLEND apart); marks apply in list order, a later one overwrites an earlier one.  Coordinates are integers in [-8192, 8191] and
 * may lie outside the frame; frames are at most 8192 x 8192, so every product below fits int64.  Pixel (x, y) is covered by
 *   PA_MARK_DISC     (x - x0)^2 + (y - y0)^2 <= r^2 + r,  r = size in 0..255  (r = 0, 1, 2, 6: 1, 9, 21, 137 pixels)
 *   PA_MARK_SEGMENT  thickness t = size in 1..255, round caps.  d = P1 - P0, L2 = |d|^2, p = P - P0, s = p . d:
 *                      L2 = 0 or s <= 0:  4 |p|^2 <= t^2;    s >= L2:  4 |P - P1|^2 <= t^2;
 *                      otherwise:         4 (p.x d.y - p.y d.x)^2 <= t^2 L2
 *   PA_MARK_FILL     min(x0, x1) <= x <= max(x0, x1) and the same in y (inclusive)
 *   PA_MARK_BOX      inside the FILL rectangle and not inside that rectangle shrunk by t = size (1..255) on every side
 *                    (the border grows inwards)
 *   PA_MARK_GLYPH    character `arg` of the built-in 5 x 7 font at scale k = size in 1..16, the cell's top-left at (x0, y0): font bit
 *                    (i, j) covers the k x k block at (x0 + i k, y0 + j k).  Codes: 0-9 A-Z space : . -   x1, y1 must be 0.
 *   PA_MARK_BLEND    the FILL rectangle (size 0..255 accepted and ignored, as for a fill).  The one kind that is NOT opaque: `arg`
 *                    is the weight a of the mark's colour, in 1..255, and a covered pixel becomes, per channel,
 *                        (p * (256 - a) + c * a + 128) >> 8
 *                    p the channel as the marks BEFORE this one in the list left it, c the mark's channel.  A later mark sees the
 *                    blended value.  (a = 128 over c = 0xffffff: half way to white; p = c stays p for every a.)
 *   PA_MARK_ARC      an axis-parallel elliptical ring cut to octants, opaque: centre (x0, y0), OUTER semi-axes a = x1, b = y1, each in
 *                    1..4095, thickness t = size in 1..255 (the ring grows inwards, like PA_MARK_BOX), octant mask `arg` in 1..255.
 *                    dx = x - x0, dy = y - y0;  in(X, Y, A, B):  X^2 B^2 + Y^2 A^2 <= A^2 B^2  (int64: |dx| <= 16383 and A, B <= 4095
 *                    keep every term below 2^54).  Covered iff all three hold:
 *                      1. in(dx, dy, a, b);
 *                      2. the hole rule  a - t < 1 or b - t < 1 or !in(dx, dy, a - t, b - t),  or the rim rule: one of the four
 *                         neighbours (dx +- 1, dy), (dx, dy +- 1) fails in(., ., a, b) — the 4-neighbour inner boundary of the filled
 *                         ellipse, without which a thin ring of a flat ellipse has gaps between the axes (the two ellipses are closer
 *                         than a pixel there); with it a full ring is 8-connected and closed;
 *                      3. bit k of `arg` is set for the pixel's octant k, taken in the ellipse's parameter space, y pointing down:
 *                         u = dx b, v = dy a; octant 0 is u > 0, 0 <= v < u; octant 1 is u > 0, v >= u; octants 2k and 2k + 1 are the
 *                         same two tests after rotating (u, v) -> (v, -u) k times: octant k is the parameter angle [45 k, 45 (k + 1))
 *                         degrees, half-open.  The centre pixel (u = v = 0) counts as octant 0.
 *                    Every covered pixel lies in x0 - a .. x0 + a, y0 - b .. y0 + b.  Kinds 7 and 9 do not exist.                    */
enum pa_mark_kind { PA_MARK_DISC = 1, PA_MARK_SEGMENT = 2, PA_MARK_FILL = 3, PA_MARK_BOX = 4, PA_MARK_GLYPH = 5, PA_MARK_BLEND = 6,
                    PA_MARK_ARC = 8 };
typedef struct pa_mark {
    int32_t kind;                 /* enum pa_mark_kind                                  */
    int32_t x0, y0, x1, y1;
    int32_t size;                 /* radius, thickness or scale, by kind                */
    uint32_t bgr;                 /* B | G << 8 | R << 16                                */
    int32_t arg;                  /* PA_MARK_GLYPH: character code; PA_MARK_BLEND: weight 1..255; PA_MARK_ARC: octant mask 1..255; otherwise 0 */
} pa_mark;
/* BGR -> YUV 4:2:0, the inverse of pa_yuv420_to_bgr.  All int32, >> arithmetic:
 *     Y = clamp(((yr R + yg G + yb B + (1 << 19)) >> 20) + y_off, 0, 255)                        per pixel
 *     U = clamp(((ur Rs + ug Gs + ub Bs + (1 << 21)) >> 22) + 128, 0, 255)     Rs, Gs, Bs: sums over the 2 x 2 block;  V likewise
 * The named tables are video.YUV_ENC_COEFFS: round(c * 2^20) of the standard matrices (their chroma rows sum to 0: grey gives
 * U = V = 128 exactly).  Geometry of the output (layout, pitches, plane offsets, frame stride) is a pa_yuv_desc whose six decode
 * coefficients are ignored.                                                                                                 */
typedef struct pa_yuv_enc {
    int32_t y_off;
    int32_t yr, yg, yb, ur, ug, ub, vr, vg, vb;
} pa_yuv_enc;
enum pa_render_out { PA_RENDER_BGR = 0, PA_RENDER_YUV420 = 1 };
/* n frames of h x w packed BGR at src_bgr_dev (HBM, frame i at src + i * h * w * 3); frame i carries marks_host[first_host[i] ..
 * first_host[i + 1]) (first_host: n + 1 entries, first[0] = 0, non-decreasing).  out = PA_RENDER_BGR: n packed frames at dst_dev
 * (geom, enc ignored; dst_dev == src_bgr_dev renders in place: every thread reads its own pixels before it writes them, and a
 * tile no mark meets writes nothing); any other overlap of dst and src is the caller's error.  out = PA_RENDER_YUV420: frame i at
 * dst_dev + i * geom->frame_stride as geom lays it out; w, h even.  The source is never written unless dst == src in BGR mode.
 * Refused, nothing launched, the reason in pa_last_error: an unknown kind, a coordinate / size / code / weight / semi-axis / octant mask out of range, a bad first[],
 * n < 1, w or h over 8192, YUV output with odd or too small w / h, a pitch smaller than its row, planes reaching into the next
 * frame, NV12 with off_v != off_u + 1, coefficients that could leave int32.  pa_render_check gives the same answers on the host
 * alone (no engine, no GPU): 0, or 1 with the reason in why[0 .. cap).
 * ASYNCHRONOUS on the engine's compute stream, like pa_yuv420_to_bgr.  The marks and first[] are copied to an engine-owned staging
 * buffer (grown on demand, freed with the engine) before the call returns: the caller may reuse its arrays at once.
 * INVARIANT, as for pa_yuv420_to_bgr: whatever later reads or overwrites dst, overwrites src, or reuses the staging buffer (the
 * next pa_render) is ordered behind this call by that one stream; work on another stream (pa_upload's copy stream, another
 * engine) is NOT ordered: pa_engine_synchronize first.
 * Two store paths, chosen per call from its pointers, pitches, offsets, stride and w % 4: dword loads / stores (16-bit stores for
 * I420's chroma planes) or bytes, which also cover the tail of widths that are no multiple of 4.                          */
int pa_render(pa_engine* eng, const uint8_t* src_bgr_dev, int n, int h, int w, const pa_mark* marks_host, const int32_t* first_host,
              int out, const pa_yuv_desc* geom, const pa_yuv_enc* enc, uint8_t* dst_dev);
int pa_render_check(int n, int h, int w, const pa_mark* marks_host, const int32_t* first_host, int out, const pa_yuv_desc* geom,
                    const pa_yuv_enc* enc, char* why, size_t cap);
/* pa_render at 1 / scale of the source's size, scale in 1..4: an anti-aliased copy that moves 1 / scale^2 of the bytes.  All integer:
 *   F' = the h x w source frame with its marks applied exactly as pa_render applies them — at source resolution, in list order;
 *        mark coordinates stay in SOURCE pixels.
 *   The output frame is ho x wo = (h / scale) x (w / scale); output pixel (X, Y) is, per channel, with s = scale,
 *        D = (sum of F'[s Y + j][s X + i] over 0 <= i, j < s  +  s^2 / 2) / s^2            integer division:
 *        (sum + 2) >> 2,  (sum + 4) / 9,  (sum + 8) >> 4         (csrc/render_scale.h; halves round up)
 *   out = PA_RENDER_BGR stores D (frame i at dst + i * ho * wo * 3); out = PA_RENDER_YUV420 applies pa_yuv_enc's formulas to D: Y per
 *   output pixel, U and V from the sums over each 2 x 2 block of D.  geom describes the OUTPUT frames (ho x wo).
 * scale = 1 is pa_render, byte for byte (in-place rendering included).  Refused, nothing launched: scale outside 1..4, w or h
 * no multiple of scale, YUV output with odd or too small wo / ho, dst == src with scale > 1, and everything pa_render refuses, its
 * geometry tests applied to ho x wo.  pa_render_scaled_check gives the same answers on the host alone; dst_is_src != 0 states that
 * the caller means dst == src.  Stream order, staging and the two store paths (chosen by wo % 4 and this call's addresses) are
 * pa_render's; one pass over HBM: the source is read once, the average is taken in registers.                                */
int pa_render_scaled(pa_engine* eng, const uint8_t* src_bgr_dev, int n, int h, int w, const pa_mark* marks_host, const int32_t* first_host,
                     int scale, int out, const pa_yuv_desc* geom, const pa_yuv_enc* enc, uint8_t* dst_dev);
int pa_render_scaled_check(int n, int h, int w, const pa_mark* marks_host, const int32_t* first_host, int scale, int out,
                           const pa_yuv_desc* geom, const pa_yuv_enc* enc, int dst_is_src, char* why, size_t cap);
/* which instantiation the last successful pa_render / pa_render_scaled of this engine launched — 1 vector path, 2 byte path, 0 none yet */
int pa_render_last_path(pa_engine* eng);
/* host only: the 7 rows (top first) of one glyph of the built-in font, column i (0 = leftmost) in bit i of a row; non-zero for a
 * code outside the font                                                                                                   */
int pa_glyph_rows(int code, uint8_t rows[7]);

/* ---- frames seen from above: packed BGR frames through one homography each (csrc/warp.hip) ----
 * n packed BGR frames of h x w at src_bgr_dev (HBM, frame i at src + i * h * w * 3) become n packed BGR frames of oh x ow at
 * dst_bgr_dev (frame i at dst + i * oh * ow * 3).  Frame i has its own 3 x 3 matrix m = m_host[9 i .. 9 i + 9), row-major, that takes
 * CANVAS pixels to SOURCE pixels, and a word valid_host[i].  fill_bgr is B | G << 8 | R << 16.  The arithmetic is csrc/warp_math.h
 * (host and device), its readable twin padel_analytics_amd/topdown.py (warp_host).  Output pixel (u, v), u the column:
 *   valid == 0: the pixel is fill.
 *   Coordinates, in IEEE double, every operation rounded on its own (no fused multiply-add), in this order:
 *       X = (m0 u + m1 v) + m2      Y = (m3 u + m4 v) + m5      Z = (m6 u + m7 v) + m8
 *     not Z > 0: fill.  sx = X / Z, sy = Y / Z, the correctly rounded quotients.
 *     not (sx > -1 && sx < w && sy > -1 && sy < h): fill.  NaN and infinities fail the comparisons.
 *   Cell and weights, in integers:  qx = (int32) floor(sx * 32), x0 = qx >> 5 (arithmetic shift), wx = qx & 31; the same in y.
 *     (NOT sx - floor(sx): for a tiny negative sx that difference rounds to 1.  sx = -1e-20 is cell -1 with weight 31.)
 *   Sampling: P(x, y) is the source pixel if 0 <= x < w && 0 <= y < h, else fill.  Per channel, all int32:
 *       top = P(x0, y0) (32 - wx) + P(x0 + 1, y0) wx        bot: the same on row y0 + 1
 *       out = (top (32 - wy) + bot wy + 512) >> 10
 *     i.e. float64 bilinear interpolation at the coordinates quantised to 1 / 32, rounded half up.
 * Doubles on purpose: projected_court's project_point is float64, so marks projected on the host and the warped picture agree to
 * far below 1 / 32 pixel.  Bilinear only: no area filter, strong minification aliases.
 * Refused, nothing launched, the reason in pa_last_error: n < 1; h, w, oh or ow outside 1 .. PA_WARP_MAX_DIM; a NULL pointer; a
 * non-finite matrix entry in a frame with valid != 0; dst overlapping src (the call is not in place).  pa_warp_check gives the same
 * answers on the host alone (no engine, no GPU): 0, or 1 with the reason in why[0 .. cap); src and dst are addresses it compares
 * and never reads through.
 * ASYNCHRONOUS on the engine's compute stream, like pa_render, under the same invariant.  The matrices and the valid words are
 * copied to an engine-owned staging buffer (grown on demand, freed with the engine) before the call returns.
 * Two store paths, chosen per call: 16 bytes at a time when ow is a multiple of 16 and dst_bgr_dev is 16-byte aligned, bytes
 * otherwise.                                                                                                                 */
#define PA_WARP_MAX_DIM 4096
int pa_warp_perspective(pa_engine* eng, const uint8_t* src_bgr_dev, int n, int h, int w, const double* m_host, const int32_t* valid_host,
                        uint32_t fill_bgr, uint8_t* dst_bgr_dev, int oh, int ow);
int pa_warp_check(int n, int h, int w, int oh, int ow, const double* m_host, const int32_t* valid_host, const void* src, const void* dst,
                  char* why, size_t cap);
/* which instantiation the last successful pa_warp_perspective of this engine launched — 1 16-byte stores, 2 byte stores, 0 none yet */
int pa_warp_last_path(pa_engine* eng);

/* ---- where the players stood: density maps on the warp's canvases (csrc/heat.hip) ----
 * All integer.  The arithmetic is csrc/heat_math.h (host and device), its readable twin padel_analytics_amd/heatmap.py
 * (accumulate_host).
 * State: `planes` (1 .. PA_HEAT_MAX_PLANES) maps of oh x ow uint32 at state_dev (HBM, plane p at state + p * oh * ow), the CALLER's:
 *   zero at the start, carried from call to call.
 * Points: frame i owns the triples pts_host[3 first_host[i] .. 3 first_host[i + 1]) = (x, y, plane): a canvas pixel (it may lie
 *   outside the canvas), |x|, |y| <= PA_HEAT_MAX_COORD, and the map it goes to.  first_host: n + 1 entries, first[0] = 0,
 *   non-decreasing, at most PA_HEAT_MAX_POINTS per frame.  pts_host may be NULL when first_host[n] is 0.
 * Splat: with radius r in 1 .. PA_HEAT_MAX_RADIUS, a point adds to pixel (u, v) of its map, where d2 = (u - x)^2 + (v - y)^2 < r r,
 *       k(d2) = (255 (r r - d2)) / (r r)            floor division: 255 at the centre, 0 on the rim and beyond
 *   (r = 2: 255, 191 on the four neighbours, 127 on the four diagonals, 1527 in all).  Every addition saturates at 2^32 - 1.
 * Display of frame t (canvas t of canvas_bgr_dev, n packed BGR canvases of oh x ow as pa_warp_perspective leaves them), in place:
 *   D     = the saturating sum, over the planes whose bit is set in show_mask, of the maps AFTER the points of frames 0 .. t of this
 *           call were added;
 *   level = D >= full ? 255 : (D 255) / full,  full in 1 .. PA_HEAT_MAX_FULL;      a = (alpha level) >> 8,  alpha in 0 .. 256;
 *   a > 0: per channel  p = (p (256 - a) + lut[level][c] a + 128) >> 8  — PA_MARK_BLEND's rule; lut_host is 256 x 3 bytes of BGR.
 *   alpha = 0 changes no pixel and still updates the state.
 * valid_host[t] == 0: canvas t is left as it is, and the frame may carry no point.
 * Refused, nothing launched, the reason in pa_last_error — one each: n < 1; oh or ow outside 1 .. PA_WARP_MAX_DIM; planes, r, full or
 * alpha outside its range; a show_mask without a bit or with one at or above planes; a NULL pointer; a first[] that does not start
 * at 0 or decreases; more than PA_HEAT_MAX_POINTS points in a frame; a point beyond +/- PA_HEAT_MAX_COORD or on a plane that is
 * not there; points in a frame with valid == 0; the state overlapping the canvases.  pa_heat_check gives the same answers on the
 * host alone (no engine, no GPU): 0, or 1 with the reason in why[0 .. cap); canvas and state are addresses it compares and never
 * reads through.
 * ASYNCHRONOUS on the engine's compute stream, like pa_warp_perspective, under the same invariant (the state included: what reads
 * it is ordered behind this call by that stream).  The host arrays are copied to an engine-owned staging buffer (grown on demand,
 * freed with the engine) before the call returns.
 * Two store paths, chosen per call: 16 bytes at a time when ow is a multiple of 16 and canvas_bgr_dev and state_dev are 16-byte
 * aligned, single pixels otherwise.                                                                                          */
#define PA_HEAT_MAX_POINTS 64
#define PA_HEAT_MAX_PLANES 4
#define PA_HEAT_MAX_RADIUS 255
#define PA_HEAT_MAX_COORD 32767
#define PA_HEAT_MAX_FULL 16777215
int pa_heat_accumulate(pa_engine* eng, uint8_t* canvas_bgr_dev, int n, int oh, int ow, uint32_t* state_dev, int planes,
                       const int32_t* pts_host, const int32_t* first_host, const int32_t* valid_host, int r, uint32_t full, int alpha,
                       int show_mask, const uint8_t* lut_host);
int pa_heat_check(int n, int oh, int ow, int planes, const int32_t* pts_host, const int32_t* first_host, const int32_t* valid_host, int r,
                  uint32_t full, int alpha, int show_mask, const uint8_t* lut_host, const void* canvas, const void* state, char* why,
                  size_t cap);
/* which instantiation the last successful pa_heat_accumulate of this engine launched — 1 16-byte accesses, 2 single pixels, 0 none yet */
int pa_heat_last_path(pa_engine* eng);

/* ---- frame statistics: is this the court camera?  (csrc/frame_activity.hip; the readable twin is activity.frame_activity_host) ----
 * All integer.  The luma of a BGR pixel is  Y = (29 B + 150 G + 77 R + 128) >> 8  (0 .. 255).
 * For frames f_0 .. f_{n-1} of h x w packed BGR (frame i at frames_bgr_dev + i * h * w * 3), a reference image ref of the same size,
 * an optional frame prev, a rectangle roi = {x0, y0, x1, y1}, half-open, 0 <= x0 < x1 <= w, 0 <= y0 < y1 <= h (NULL: the whole
 * frame) and a threshold tau in 0 .. 255, three uint64 per frame, summed over the pixels of roi:
 *     out[3 i + 0] = sad_ref  = sum |Y(f_i) - Y(ref)|
 *     out[3 i + 1] = changed  = #{ |Y(f_i) - Y(ref)| > tau }          (strict)
 *     out[3 i + 2] = sad_prev = sum |Y(f_i) - Y(f_{i-1})|             f_{-1} = prev if given, otherwise sad_prev of frame 0 is 0
 * The numbers of a frame are exact and depend on that frame, ref and its predecessor alone: not on n, on the frame's place in the
 * batch, on the alignment of a pointer or on how the launch is shaped (workgroups write partial sums to a slab, a second kernel adds
 * them: no atomics).  out_u64 is HOST memory, n x 3; rows beyond n are not touched.
 * Limits (PA_ACTIVITY_MAX_SIDE, PA_ACTIVITY_MAX_FRAMES): h and w at most 16384 — a workgroup's band of at most 16384 pixels keeps
 * every 32-bit partial sum below 2^23 — and n at most 65535, the second grid dimension.
 * pa_frame_activity_check: host only (no engine, no GPU): NULL if pa_frame_activity would accept these arguments, else the reason,
 * a string of static storage in this thread, valid until its next call.  One reason each for: n out of range; h or w out of
 * range; a roi that is empty or leaves the frame; tau outside 0 .. 255.
 * pa_frame_activity: SYNCHRONOUS, on the engine's compute stream, so ordered behind whatever produced the frames there.  Refuses
 * what the check refuses (and a NULL pointer), launching nothing, the reason in pa_last_error.  The slab is an engine-owned buffer
 * grown on demand and freed with the engine.                                                                                 */
#define PA_ACTIVITY_MAX_SIDE 16384
#define PA_ACTIVITY_MAX_FRAMES 65535
const char* pa_frame_activity_check(int n, int h, int w, const int32_t* roi, int tau);
int pa_frame_activity(pa_engine* eng, const uint8_t* frames_bgr_dev, int n, int h, int w, const uint8_t* ref_bgr_dev,
                      const uint8_t* prev_bgr_dev_or_null, const int32_t* roi_or_null, int tau, uint64_t* out_u64);
/* the per-pixel, per-channel median of n BGR frames in HBM (np.median(frames, 0).astype(uint8): an even n gives (a + b) >> 1 of
 * the two middle values), n <= 65535, h and w within PA_ACTIVITY_MAX_SIDE -> h x w x 3 BGR at out_bgr_dev (HBM, not overlapping
 * the frames).  The kernel of pa_ball_background_from_frames (which writes RGB), reachable without a ball session.  SYNCHRONOUS
 * on the compute stream.                                                                                                      */
int pa_frames_median(pa_engine* eng, const uint8_t* frames_bgr_dev, int n, int h, int w, uint8_t* out_bgr_dev);

/* ---- colour histograms of boxes: who is this player?  (csrc/box_histogram.hip; the readable twin is identity.box_histograms_host) ----
 * All integer.  A BGR pixel falls into bin  ((B >> 5) << 6) | ((G >> 5) << 3) | (R >> 5)  (0 .. 511: three bits a channel).
 * For frames of h x w packed BGR (frame i at frames_bgr_dev + i * h * w * 3) and k rectangles rects[5 j .. 5 j + 4] = {frame, x0,
 * y0, x1, y1}, half-open, 0 <= frame < n, 0 <= x0 < x1 <= w, 0 <= y0 < y1 <= h, 512 uint32 per rectangle:
 *     out[512 j + b] = #{ pixels (x, y) of frame rects[5 j], x0 <= x < x1, y0 <= y < y1, whose bin is b }
 * The counts of a rectangle are exact and depend on that rectangle and its frame alone: not on k, on the rectangle's place in the
 * list (a rectangle listed twice gives two equal rows), on the alignment of a pointer or on how the launch is shaped (one workgroup
 * per rectangle adds into histograms in LDS — integer addition, exact in any order — and stores its row with plain stores: no
 * global atomics).  rects and out_u32 are HOST memory, k x 5 and k x 512; rows beyond k are not touched.  k = 0 is accepted and
 * launches nothing (rects may then be NULL).
 * Limits: n, h and w as for pa_frame_activity (PA_ACTIVITY_MAX_FRAMES, PA_ACTIVITY_MAX_SIDE: a rectangle has at most 2^28 pixels, a
 * counter cannot wrap); k at most PA_BOX_HIST_MAX_RECTS.
 * pa_box_histograms_check: host only (no engine, no GPU): NULL if pa_box_histograms would accept these arguments, else the reason,
 * a string of static storage in this thread, valid until its next call.  One reason each for: n out of range; h or w out of
 * range; k out of range; a NULL pointer; a frame index outside 0 .. n - 1; a rectangle that is empty or leaves the frame (the
 * last two name the first offending rectangle).
 * pa_box_histograms: SYNCHRONOUS, on the engine's compute stream, so ordered behind whatever produced the frames there.  Refuses
 * what the check refuses (and a NULL frames or out pointer, with the check's words for NULL), launching nothing, the reason in
 * pa_last_error.  The rectangle list and the counters go through an engine-owned buffer grown on demand and freed with the engine. */
#define PA_BOX_HIST_BINS 512
#define PA_BOX_HIST_MAX_RECTS 16384
const char* pa_box_histograms_check(int n, int h, int w, const int32_t* rects, int k);
int pa_box_histograms(pa_engine* eng, const uint8_t* frames_bgr_dev, int n, int h, int w,
                      const int32_t* rects /* host, k x 5: frame, x0, y0, x1, y1 */, int k, uint32_t* out_u32 /* host, k x 512 */);

/* ---- frames to a file: the YUV 4:2:0 bytes pa_render writes -> one baseline JPEG per frame (Motion-JPEG; csrc/jpeg_encode.hip) ----
 * The bit stream is specified here; its constants are csrc/jpeg_tables.h (host and device), its readable twin
 * padel_analytics_amd/mjpeg.py (encode_host), which produces the same bytes.
 *
 * One frame = one baseline sequential JPEG (ITU-T T.81): 8-bit, three components, Y sampled 2 x 2, Cb and Cr 1 x 1 (4:2:0, MCUs of
 * 16 x 16 pixels: Y00 Y01 Y10 Y11 Cb Cr).  Segments, in this order, 613 bytes up to the scan:
 *     SOI | APP0 "JFIF" 1.01, no units, 1:1, no thumbnail | DQT, one segment, tables 0 (luma) and 1 (chroma), 8-bit, zig-zag order |
 *     SOF0 with the true h and w, Y table 0, Cb / Cr table 1 | DHT, one segment: DC 0, AC 0, DC 1, AC 1, the Annex K tables, in every
 *     frame | DRI ceil(w / 16): a restart interval is one MCU row | SOS | the scan, RSTm (m = interval index mod 8) between the
 *     intervals | EOI
 * Input: frames as a pa_yuv_desc lays them out (either layout, any pitch, plane offsets, frame stride; its decode coefficients are
 * not used); JFIF decoders assume the full-range BT.601 matrix — video.YUV_ENC_COEFFS["bt601_full"] on the rendering side.  w and h
 * even, >= 2; where they are no multiples of 16 a block is completed by repeating the last column and the last row.
 * Arithmetic, all int32, >> arithmetic, descale(x, s) = (x + (1 << (s - 1))) >> s:
 *   samples       x - 128
 *   forward DCT   Loeffler-Ligtenberg-Moshovitz with 13-bit constants (libjpeg's "islow": jpeg_tables.h, fdct8), rows first, then
 *                 columns.  Row pass: outputs 0 and 4 are the sums shifted left by 2 (exact), the six others descale(.., 11): results
 *                 scaled by 4.  Column pass: outputs 0 and 4 descale(.., 2), the others descale(.., 15): results scaled by 8 in all.
 *   quantisation  sign(c) * ((|c| + 4 q) / (8 q)), integer division
 *   tables        q = clamp((base * s + 50) / 100, 1, 255), base the Annex K luminance / chrominance entry, s = 5000 / Q for
 *                 Q < 50, else 200 - 2 Q; Q = quality in 1..100
 * Entropy coding: zig-zag order; DC as the difference to the previous block of the same component in the same restart interval (0
 * at its start), category + bits; AC as run / size symbols with ZRL for 16 zeros and EOB; the Annex K Huffman codes; the last byte
 * of an interval padded with 1-bits; every 0xFF byte of entropy-coded data followed by 0x00.
 *
 * n frames of h x w at src_yuv_dev (HBM) -> the JPEGs back to back in dst_host[0 .. offsets_host[n]); frame i occupies
 * [offsets_host[i], offsets_host[i + 1]) (offsets_host: n + 1 entries, [0] = 0).  0 on success.  If the frames take more than
 * cap bytes, nothing is written to dst_host, offsets_host[n] is the size needed (offsets_host[0] = 0, the others untouched)
 * and the call fails.  Refused, nothing launched, the reason in pa_last_error: n < 1, odd or too small w / h, w > PA_JPEG_MAX_WIDTH
 * (one workgroup stages an MCU row in LDS), quality outside 1..100, a pitch smaller than its row, planes reaching into the next
 * frame, NV12 with off_v != off_u + 1.  pa_jpeg_check gives the same answers on the host alone (no engine, no GPU).
 * SYNCHRONOUS, but ordered on the engine's compute stream: the pa_render that produced src is ahead of it in that stream, nothing
 * runs on another stream.  Scratch (the restart intervals' slots, the gathered frames) belongs to the engine, grows on demand and
 * is freed with it.  A slot holds the worst case of its interval — pa_jpeg_interval_bytes(w): every block 22 + 63 x 26 bits, every
 * byte stuffed — so no input writes outside its slot; slots of at most 256 MiB are in use at a time (larger calls are encoded
 * in sub-batches inside the call).                                                                                          */
#define PA_JPEG_MAX_WIDTH 2560
int pa_jpeg_encode(pa_engine* eng, const uint8_t* src_yuv_dev, int n, int h, int w, const pa_yuv_desc* geom, int quality,
                   uint8_t* dst_host, size_t cap, int64_t* offsets_host);
int pa_jpeg_check(int n, int h, int w, const pa_yuv_desc* geom, int quality, char* why, size_t cap);
/* host only: the most bytes one restart interval of a frame of width w can take, its closing marker included: a slot's capacity */
size_t pa_jpeg_interval_bytes(int w);

/* ---- frames from a file: baseline JPEGs (Motion-JPEG: .avi 'MJPG', .mjpeg) in host memory -> packed BGR in HBM (csrc/jpeg_decode.hip) ----
 * The decoded pixels are specified here: those of libjpeg's default decoder (JDCT_ISLOW, fancy upsampling, JFIF YCbCr -> RGB).  The
 * readable twin is padel_analytics_amd/mjpeg.py (parse_frame, decode_host), which produces the same bytes; the markers are read by
 * host-only code (csrc/jpeg_parse.cpp), the entropy decoder is one header for host and device (csrc/jpeg_entropy.h), the arithmetic
 * another (csrc/jpeg_idct.h).
 *
 * Accepted: one SOF0 frame, 8-bit, three components, the first sampled 2 x 2 and the two others 1 x 1; 8-bit DQT; one interleaved scan
 * over the three components (Ss = 0, Se = 63, Ah = Al = 0); any Huffman tables (ids 0 and 1) in DHT, and WITHOUT any DHT the Annex K
 * tables (the AVI 'MJPG' convention); DRI of any value, intervals that are not whole MCU rows and RSTm wrapping past 7 included; any
 * 1 <= w, h <= PA_JPEG_DEC_MAX_DIM in at most PA_JPEG_DEC_MAX_BYTES; APPn / COM and other segments with a length are skipped by it.
 * Refused, each with its reason:
 * progressive / extended / lossless / arithmetic SOF, 12- or 16-bit data, another sampling, more than one scan, a truncated header,
 * a table the scan names but no segment defined, and (pa_jpeg_decode) frame sizes that differ within a call.
 * A restart interval is found by a scan of the entropy-coded data for FF D0..D7; interval k covers MCUs [k Ri, min((k + 1) Ri, MCUs));
 * a stream without DRI is one interval.  Intervals the data does not hold are empty; more markers than intervals set PA_JPEG_ST_MARKERS.
 * Entropy decoding of one interval: bits MSB first, FF 00 is the byte FF, any other FF xx ends the data; bits past the end read as 0.
 * DC: category (<= 11) + bits, added to the previous block of the component in this interval (0 at its start); AC: run / size symbols
 * (size <= 10), 00 = end of block, F0 = 16 zeros.  A block that cannot be decoded — a bit pattern no code matches, a category beyond
 * those limits, a coefficient index past 63, more bits taken than the interval holds — ends its interval: that block and the rest
 * of the interval's are zero, the reason goes into the frame's status word (PA_JPEG_ST_*), and nothing is read or written out of
 * bounds: a corrupt frame is reported, never a fault.
 * Per block, all int32 with wrap-around, >> arithmetic: coefficient k of the zig-zag times the component's quantiser entry k; then
 * the inverse DCT, one pass over 8 values d0..d7 with descale shift s:
 *     z1 = (d2 + d6) * 4433; t2 = z1 - d6 * 15137; t3 = z1 + d2 * 6270; t0 = (d0 + d4) << 13; t1 = (d0 - d4) << 13
 *     t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
 *     a0 = d7; a1 = d5; a2 = d3; a3 = d1; z1 = a0 + a3; z2 = a1 + a2; z3 = a0 + a2; z4 = a1 + a3; z5 = (z3 + z4) * 9633
 *     a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
 *     a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4
 *     out = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3), each (x + (1 << (s - 1))) >> s
 * over the columns first (s = 11), then over the rows (s = 18); the sample is clamp(x + 128, 0, 255).  (libjpeg's table wraps instead
 * of clamping once |x| >= 384; below that the two agree.)
 * Chroma ("h2v2 fancy"), on the plane of its real size ceil(h / 2) x ceil(w / 2), indices clamped to it: for output row 2 r + v,
 * s[c] = 3 C[r][c] + C[r'][c], r' = r - 1 (v = 0) or r + 1 (v = 1); out[2 c] = (3 s[c] + s[c - 1] + 8) >> 4,
 * out[2 c + 1] = (3 s[c] + s[c + 1] + 7) >> 4; cropped to h x w.
 * Colour, cb -= 128, cr -= 128: R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
 * G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), each clamped to 0..255, stored B, G, R.                                       */
#define PA_JPEG_DEC_MAX_DIM 4096
#define PA_JPEG_DEC_MAX_BYTES (1 << 27)   /* of one frame */
enum { PA_JPEG_ST_CODE = 1, PA_JPEG_ST_INDEX = 2, PA_JPEG_ST_SIZE = 4, PA_JPEG_ST_DATA = 8, PA_JPEG_ST_MARKERS = 16 };
typedef struct pa_jpeg_huff {
    uint8_t bits[16];       /* codes per length 1..16 */
    uint8_t vals[256];      /* symbols in code order */
    int32_t nvals;
} pa_jpeg_huff;
typedef struct pa_jpeg_interval {
    int64_t begin, end;     /* entropy-coded bytes [begin, end) from the start of the frame, markers excluded */
    int32_t first_mcu, mcus;
} pa_jpeg_interval;
typedef struct pa_jpeg_frame_info {
    int32_t w, h, mcus_x, mcus_y;
    int32_t restart_interval;   /* DRI, 0: none */
    int32_t n_intervals;
    int32_t default_huffman;    /* 1: the frame has no DHT, the Annex K tables stand in */
    int32_t status;             /* 0 or PA_JPEG_ST_MARKERS */
    int64_t scan_begin, scan_end;   /* the entropy-coded data: behind SOS .. the marker that ends it (or the end of the bytes) */
    uint8_t quant[3][64];       /* per component, zig-zag order */
    uint8_t comp_dc[3], comp_ac[3], pad_[2];   /* per component: index into dc[] / ac[] */
    pa_jpeg_huff dc[2], ac[2];
} pa_jpeg_frame_info;
/* host only (no engine, no GPU): the markers of one frame -> its description and the first ivl_cap entries of its interval table
 * (info->n_intervals says how many there are).  Non-zero: refused, the reason in why[0 .. cap).                              */
int pa_jpeg_parse(const uint8_t* jpeg, size_t len, pa_jpeg_frame_info* info, pa_jpeg_interval* ivls, size_t ivl_cap, char* why,
                  size_t cap);
/* n JPEGs, frame i at jpegs_host[offsets[i] .. offsets[i + 1]) (offsets: n + 1 entries), all h x w -> packed BGR frames at
 * dst_bgr_dev (HBM, n * h * w * 3 bytes, any alignment), status_host[i] = 0 or the PA_JPEG_ST_* bits of frame i.  0 on success — a
 * frame with a non-zero status is still a success of the call.  Refused, nothing launched, the reason in pa_last_error: what
 * pa_jpeg_parse refuses (with the frame's index) and a frame whose size is not h x w.  SYNCHRONOUS, on the engine's compute stream
 * (a reader of dst queued earlier is ahead of it, nothing runs on another stream).  Three kernels: one wave per restart interval
 * decodes it to int16 coefficients, one thread per block dequantises and inverts the DCT into padded planes, a third pass
 * upsamples and converts.  The scratch (compressed bytes, coefficients, planes: 4.5 bytes per pixel of the padded frame) belongs
 * to the engine, grows on demand and is freed with it; at most 64 frames or 256 MiB of it are in use at a time (larger calls are
 * decoded in sub-batches inside the call).
 * The split path: an interval of at least min_bytes bytes (pa_jpeg_decode_set_split; a stream without restart markers is one interval,
 * the whole frame) is decoded by one workgroup instead of one wave (csrc/jpeg_entropy_split.h).  Its bytes are cut into subsequences
 * of sub_bytes raw bytes (more where 4096 of them would not cover it), one lane each.  A lane decodes its subsequence from the state
 * (bit position, block in MCU, coefficient index) the subsequence before it ended in, in the first round from the guess "a block
 * starts at my first bit"; a state no symbol could be decoded from is replaced by that guess.  Rounds repeat until no exit state
 * changes, at most one per subsequence, after which every state is the serial decoder's; then each subsequence is decoded once more
 * and stores its coefficients at their blocks, DC as differences that one scan per component sums.  Pixels and status words are
 * those specified above bit for bit, damaged intervals included; how many rounds it took depends on the data only.  Shorter
 * intervals keep the one-wave kernel, so a stream without restart markers is one workgroup per frame, one with them one wave per
 * interval.                                                                                                                      */
int pa_jpeg_decode(pa_engine* eng, const uint8_t* jpegs_host, const int64_t* offsets, int n, int h, int w, uint8_t* dst_bgr_dev,
                   int32_t* status_host);
/* Which intervals of later pa_jpeg_decode calls take the split path.  min_bytes: 0 the default, -1 never (every interval on the
 * one-wave kernel), else the length in bytes from which an interval is split.  sub_bytes: 0 the default, else a multiple of 4 in
 * [4, 32768].  Anything else is refused with its reason (pa_last_error(eng); of a NULL engine: pa_last_error(NULL)).  The defaults
 * are measured (profiles/mjpeg_split_bench.txt).                                                                               */
#define PA_JPEG_DEC_SPLIT_MIN_BYTES 7168
#define PA_JPEG_DEC_SPLIT_SUB_BYTES 128
int pa_jpeg_decode_set_split(pa_engine* eng, int64_t min_bytes, int32_t sub_bytes);
/* tests, tools: of the last successful pa_jpeg_decode: out[0] intervals on the split path, out[1] their subsequences, out[2] the
 * largest number of rounds any of them took (the kernel writes it beside the status word), out[3] intervals on the one-wave kernel */
int pa_jpeg_decode_last_split(pa_engine* eng, int64_t out[4]);
/* tests: 1 if the last successful pa_jpeg_decode wrote its pixels with 16-byte stores (w a multiple of 16 and dst 16-byte aligned),
 * 2 if with byte stores, 0: none yet                                                                                          */
int pa_jpeg_decode_last_path(pa_engine* eng);
/* tools: while profiling is on (pa_engine_set_profiling) a pa_jpeg_decode also times its stages; ms[0 .. 5) of the last such call:
 * reading the markers of all frames (host clock), the upload of the compressed bytes and tables, the entropy pass, the IDCT pass,
 * the colour pass (HIP events on the compute stream, summed over the call's sub-batches)                                     */
int pa_jpeg_decode_last_times(pa_engine* eng, double ms[5]);

/* tools: device time of whatever is queued on the engine's compute stream between the two calls, from a pair of HIP events
 * recorded on that stream (tools/yuv_bench.py times the asynchronous pa_yuv420_to_bgr with it).  pa_engine_timer_stop waits for
 * its event and returns the milliseconds between the two.                                                              */
int pa_engine_timer_start(pa_engine* eng);
int pa_engine_timer_stop(pa_engine* eng, float* ms);

/* tuning knobs (tests / tools only).  Defaults come from the environment ONCE at pa_engine_create
 * (PADEL_CONV_IMPL=tap|lds, PADEL_CONV_VARIANT, PADEL_CONV_TUNE, PADEL_CONV_TAP_PD, PADEL_GRAPH, PADEL_ALIAS).
 * keys: "impl" (2 bf16x3 kernels = default, 0 fp32-MFMA tap kernels, 1 fp32-MFMA LDS cross-check kernel),
 * "variant" (forced tile id, -1 auto), "tune" (bit word; bits 0..3 are kept, csrc/launch_plan.h names the ones that select anything),
 * "tap_pd" (2|3), "graph" (hipGraph replay of the op list), "alias" (liveness-shared activation arena),
 * "timeline" (s_memtime-instrumented 3x3 kernel, dump to pa_engine_set_timeline_path),
 * "lanes" (2 = default: a YOLO model may run alternate in-flight tickets on a second lane, 1: one lane; PADEL_LANES),
 * "fuse_stem_cv1" (1 = default: an h2 YOLOv8 graph computes model.2.cv1, the 1x1 conv behind model.1, inside the fused stem +
 * model.1 kernel and never writes model.1's map, 0: that conv is a launch of its own; same bits; off while profiling or collecting
 * a timeline; PADEL_FUSE_STEM_CV1; pa_model_last_stem_path tells which ran) */
int pa_engine_set_tuning(pa_engine* eng, const char* key, int value);
int pa_engine_set_timeline_path(pa_engine* eng, const char* path);

/* ---- models ---- */
/* weights: packed blob produced by the host graph builder; copied to HBM, caller keeps ownership.
 * weights == NULL: the blob is allocated zero-filled and filled by pa_engine_bcast_weights (ranks that did
 * not load the checkpoint)                                                                             */
int pa_model_create(pa_engine* eng, const pa_model_desc* desc, const float* weights, size_t n_floats,
                    pa_model** out);
void pa_model_destroy(pa_model* m);
/* PA_DTYPE_H2 and PA_DTYPE_F16 models: *out = 1 if any activation written since the last call did not fit the fp16 range
 * (h2: |x| > 65504 of a pair's value; fp16: !(|x| <= 65504) of the fp32 value about to be clamped and stored, NaN included).
 * The results of those inferences are invalid: repeat them on a model of a wider type (fp16 -> h2 or fp32, h2 -> fp32).  Then
 * clears the flag.  Always 0 for PA_DTYPE_F32 models                                                                   */
int pa_model_take_overflow(pa_model* m, int* out);
/* frames / windows processed per replay of the graph (activation buffers are sized for it); default 64 */
int pa_model_set_max_batch(pa_model* m, int max_batch);
/* activation bytes of the current plan: the liveness-shared arena actually allocated, and the sum of the
 * logical buffers it replaces */
int pa_model_plan_bytes(pa_model* m, size_t* arena_bytes, size_t* logical_bytes);

/* tests: overwrite every byte of the planned activation arena (0xFF = NaN patterns in fp32 and fp16).  A following
 * inference must be unaffected: no kernel may read a byte nobody wrote since (h2 / fp32 graphs; fp16 graphs rely on
 * zero-initialised pad channels and are excluded).  The u8 network input of a YOLO / ResNet plan is overwritten as well:
 * the preprocessing of the next call writes all four bytes of every pixel                                     */
int pa_model_fill_arena(pa_model* m, int byte_value);

enum pa_pre_mode {
    PA_PRE_LETTERBOX = 0,   /* ultralytics LetterBox(auto, stride 32), cv2 INTER_LINEAR, pad 114    */
    PA_PRE_PIL_STRETCH = 1  /* PIL Image.resize((imgsz, imgsz)) bicubic, then LetterBox == identity */
};

typedef struct pa_yolo_params {
    int32_t imgsz;            /* 640 / 1280                                                         */
    int32_t pre_mode;         /* enum pa_pre_mode                                                   */
    int32_t channel_reverse;  /* 1: network channel c = frame channel 2-c      */
    int32_t letterbox_auto;   /* LetterBox auto flag (1 when all frames of the call share a shape)  */
    float conf, iou;
    int32_t max_det;          /* <= 300 rows are returned per image                                 */
    int32_t n_classes;        /* 0: keep every class                                                */
    const int32_t* classes;   /* host array                                                         */
    int32_t frames_on_device; /* 1: `frames` is an HBM pointer from pa_device_malloc                */
} pa_yolo_params;

/* frames: n x h x w x 3 uint8 (HWC).  out_boxes: n x max_det x 6 {x1,y1,x2,y2,conf,cls} in source
 * pixels; out_kpts: n x max_det x nk (NULL for detect); out_counts: n.                              */
int pa_yolo_infer(pa_model* m, const uint8_t* frames, int n, int h, int w, const pa_yolo_params* p,
                  float* out_boxes, float* out_kpts, int32_t* out_counts);

/* The same call in two halves, for pipelined batch loops (round 4): pa_yolo_submit enqueues everything pa_yolo_infer does
 * — preprocessing, network, decode, NMS, the result copies — behind whatever the engine's stream holds at the call and returns a
 * ticket WITHOUT waiting; pa_yolo_wait blocks until that ticket's results are in the caller's arrays.  Submitting batch
 * k + 1 before waiting for batch k keeps the GPU busy while the host collects results and prepares the next call (the
 * reference's `predict` is synchronous per batch, players_tracker.py:351-359: its GPU idles there).
 * LANES.  A ticket runs on one of the model's (at most two) lanes: a stream of its own with its own network input, activation
 * arena and post-processing buffers.  A submit that finds the model's previous ticket still in flight (not waited for) goes to
 * the other lane — allocated then, if the memory is there; otherwise the model stays on one lane — so that the workgroups of two
 * batches share the chip (tuning "lanes", PADEL_LANES = 1 | 2).  Every ticket's results are bitwise what pa_yolo_infer gives.
 * ORDERING, as observed by the caller, is still that of ONE stream: a ticket runs behind everything enqueued on the engine's
 * stream before its submit (a conversion, a decode, a render: it sees their frames), and everything enqueued on the engine's
 * stream after the submit — the next conversion into the same frame buffer, a render, a read-back, pa_engine_synchronize,
 * pa_model_take_overflow — runs behind the ticket.  Two tickets with nothing between their submits but waits may run at the same
 * time; work put on the engine's stream between two submits orders the second ticket behind the first, as before lanes.
 * Tickets need NOT complete in submission order: pa_yolo_wait may be called in any order and returns when its own ticket is
 * done.  pa_yolo_infer and pa_yolo_postprocess run on lane 0 and return with every outstanding ticket of either lane complete.
 * Requirements: frames in HBM (frames_on_device = 1), n <= max_batch, no profiling; out_* must be page-locked
 * (pa_host_register) and must not be touched between submit and wait — the ONE place where the library keeps caller
 * pointers past return.  At most PA_MAX_INFLIGHT tickets per model; the plan
 * (source size, imgsz, batch) must not change while tickets are in flight.  `overflow` (may be NULL): 1 if an activation of
 * an h2 or fp16 model has left the fp16 range by the time this ticket finished (sticky until pa_model_take_overflow, and shared by the
 * lanes: a ticket always sees its own overflow, and may see its neighbour's): the results of this and of later tickets are then
 * not to be used (see pa_dtype); 0 for fp32 models.                                                                                */
#define PA_MAX_INFLIGHT 4
int pa_yolo_submit(pa_model* m, const uint8_t* frames, int n, int h, int w, const pa_yolo_params* p,
                   float* out_boxes, float* out_kpts, int32_t* out_counts, int* ticket);
int pa_yolo_wait(pa_model* m, int ticket, int* overflow);

/* decode + NMS + rescale alone, on CALLER-SUPPLIED head maps (tests: hand-derived known answers for the Detect / Pose
 * inference branch, ops.non_max_suppression, scale_boxes — players_tracker.py:351-359 [upstream]): heads[l] =
 * n x H_l x W_l x c fp32 in the pa_yolo_head_shape layout of the plan for source size h x w (n <= max_batch); outputs as
 * pa_yolo_infer                                                                                               */
int pa_yolo_postprocess(pa_model* m, const float* const* heads, int n, int h, int w, const pa_yolo_params* p,
                        float* out_boxes, float* out_kpts, int32_t* out_counts);

/* raw head maps of the last pa_yolo_infer call (level 0..2): n x H_l x W_l x c fp32 (c from
 * pa_yolo_head_shape; channels [0,64) box DFL logits, [64,64+nc) class logits, then nk keypoint values).
 * h2 models whose heads end in the usual 1x1 convs do not write these maps in a plain call (tuning fuse_head: the convs and the
 * decode run as one kernel): pa_yolo_read_head then computes them on demand, for the images of the last call, from the convs'
 * inputs, which the plan keeps until the next call; further reads copy what the first one computed */
int pa_yolo_head_shape(pa_model* m, int level, int* h, int* w, int* c);
int pa_yolo_read_head(pa_model* m, int level, int n, float* out);
/* which post-processing the model's last pa_yolo_infer / pa_yolo_submit / pa_yolo_postprocess took: 0 decode_kernel over head
 * maps, 1 the fused head tail (the heads' last convs and the decode in one kernel, no head map)                            */
int pa_yolo_last_post_path(pa_model* m);
/* lanes (pa_yolo_submit): how many the model's current plan has allocated (0 before a plan, 1, 2), and the lane (0 | 1) its last
 * pa_yolo_infer / pa_yolo_submit / pa_yolo_postprocess ran on.  pa_yolo_read_head, pa_yolo_read_netin and
 * pa_yolo_last_post_path refer to that lane.  pa_model_plan_bytes reports ONE lane's plan                              */
int pa_model_lanes_allocated(pa_model* m);
/* tests: passes of the Pillow resample of the model's current plan — 0 (no plan, letterbox, or a source of the target size), 1 (one
 * axis changes), 2 (both: the horizontal pass writes a temporary that the vertical pass reads; every lane has its own)       */
int pa_yolo_resample_passes(pa_model* m);
int pa_model_last_lane(pa_model* m);
/* which form of the fused stem kernel the model's last replay of its op list launched: 1 stem + model.1 + the 1x1 conv behind it
 * (tuning fuse_stem_cv1), 0 anything else (that conv ran as a launch of its own, or the graph has no such conv)                  */
int pa_model_last_stem_path(pa_model* m);

/* the u8 network input (NHWC4: R,G,B,0 as the network sees them) the last pa_yolo_infer call built from its
 * first n frames — byte-exact check of the letterbox (cv2 INTER_LINEAR) / Pillow-bicubic preprocessing */
int pa_yolo_netin_shape(pa_model* m, int* h, int* w);
int pa_yolo_read_netin(pa_model* m, int n, uint8_t* out);

/* generic graph forward (TrackNet): x = n x H x W x C_in fp32 NHWC (C_in = channels of buffer 0) ->
 * contents of buffer head_buf[0]: n x (H>>level) x (W>>level) x channels fp32 */
int pa_tracknet_infer(pa_model* m, const float* x, int n, int h, int w, int x_on_device, float* out,
                      int out_on_device);

/* ---- court keypoints: torchvision ResNet-50 regressor (trackers/keypoints_tracker/keypoints_tracker.py:264-312) ----
 * frames: n x h x w x 3 uint8 BGR.  Each is turned to RGB, resized to 224 x 224 as transforms.Resize does on a PIL image (Pillow
 * BILINEAR: horizontal pass, then vertical, 22-bit fixed point), normalised inside the stem and run through the graph of a
 * PA_TASK_RESNET model.  out_xy: n x cout sigmoid outputs of the graph's PA_OP_GAP_FC (24 = 12 keypoints x (x, y) as fractions of
 * the frame size); out_logits (optional): the same before the sigmoid.  A graph without that op (unit tests) takes out_xy = NULL. */
int pa_resnet_infer(pa_model* m, const uint8_t* frames, int n, int h, int w, int frames_on_device, float* out_xy, float* out_logits);
/* the u8 network input (n x 224 x 224 x 4: R, G, B, 0) the last pa_resnet_infer call built from its first n frames */
int pa_resnet_read_netin(pa_model* m, int n, uint8_t* out);
/* results of the PA_OP_GAP_FC op of the last replay of ANY graph that has one (n x cout each, either may be NULL) */
int pa_resnet_read_fc(pa_model* m, int n, float* out_xy, float* out_logits);
/* tests: contents of buffer head_buf[0] of a PA_TASK_RESNET model after the last pa_resnet_infer call, n x H x W x channels fp32 */
int pa_resnet_read_head(pa_model* m, int n, float* out);

/* host only (no GPU needed; tests): the coefficient tables of one Pillow resample pass in_size -> out_size as the device kernels
 * use them — filter 0 = BICUBIC (a = -0.5), 1 = BILINEAR; 22-bit fixed point.  *ksize = taps per output; bounds: out_size x 2
 * {first input index, taps used}; coefs: out_size x ksize (coefs_cap = its capacity in elements).  bounds = coefs = NULL: only
 * *ksize is returned.                                                                                                       */
int pa_pil_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* coefs, int coefs_cap, int* ksize);

/* ---- ball path: streaming TrackNet session (trackers/ball_tracker/ball_tracker.py:373-523) ----
 * Frames are fed in stream order; every frame is Pillow-bicubic-resized to 512x288 on the device once
 * (iterable.py:188), windows of 8 consecutive frames + the background are run through the TrackNet
 * model, the 8 overlapping window outputs of each frame are ensembled (ball_tracker.py:449-509) and
 * thresholded at 0.5 (predict.py:184).  The caller gets one 288x512 uint8 mask (255/0) per frame, in
 * frame order, and turns it into coordinates (predict.py:7-39) on the host.
 * The TrackNet model may have any storage type: fp32, h2 pairs, or PA_DTYPE_F16 (fp16 activations and
 * weights, fp32 accumulation; window assembly writes halves, the sigmoid head map stays fp32, so the
 * ensemble, threshold and locate steps are the same for all three).                                  */
typedef struct pa_ball pa_ball;
int pa_ball_create(pa_model* tracknet, int src_h, int src_w, pa_ball** out);
void pa_ball_destroy(pa_ball* b);
/* background: src_h x src_w x 3 uint8 RGB (np.median(...).astype(uint8), iterable.py:70-78); also resets
 * the stream state                                                                                     */
int pa_ball_set_background(pa_ball* b, const uint8_t* median_rgb);
/* background = per-pixel median of the first n BGR frames, computed on the device with np.median + uint8
 * truncation semantics (iterable.py:59-78); out_median_rgb (optional) receives the src_h x src_w x 3 RGB
 * median; also resets the stream state                                                                 */
int pa_ball_background_from_frames(pa_ball* b, const uint8_t* frames_bgr, int n, int frames_on_device,
                                   uint8_t* out_median_rgb);
/* frames: n x src_h x src_w x 3 uint8 BGR (n <= the model's max_batch).  flush != 0 after the last
 * frames of the clip emits the 7 tail frames.  Outputs, each optional (NULL) but at least one of
 * masks / rects: out_masks (n + 7) x 288 x 512 bytes; out_heat (n + 7) x 288 x 512 fp32 ensembled heat
 * maps; out_rects (n + 7) x 4 int32 {x, y, w, h} = predict_location (predict.py:7-39) of each mask
 * (largest bounding rectangle among the 8-connected components; all zero: empty mask; w = -1: too many
 * foreground pixels for the device list, use the mask).                                               */
int pa_ball_feed(pa_ball* b, const uint8_t* frames_bgr, int n, int frames_on_device, int flush,
                 uint8_t* out_masks, float* out_heat, int32_t* out_rects, int* out_count);

/* predict_location on caller-supplied masks (n x 288 x 512 uint8, n <= max_batch + 7) -> n x 4 {x, y, w, h} */
int pa_ball_locate(pa_ball* b, const uint8_t* masks, int n, int32_t* out_rects);

/* tests: one image of the session's Pillow-bicubic resize, 288 x 512 x 3 bytes RGB — byte-exact check of that preprocessing.
 * frame < 0: the resized background of the last pa_ball_set_background / pa_ball_background_from_frames; otherwise frame `frame`
 * (counted from 0 since the background was set) of the ring, which keeps the last max_batch + 7 frames fed */
int pa_ball_read_resized(pa_ball* b, long long frame, uint8_t* out);

/* ---- multi-GPU: one process per GPU, frames shard by batch, the ONLY collective is the one-time broadcast
 * of the packed weight blob from the rank that loaded the checkpoint; RCCL over xGMI,
 * HBM to HBM, no host bounce.  The reference has no distributed code (single `.to(device)`,
 * trackers/tracker.py:172-174) — this replaces "load the .pt in every process".
 * Bootstrap: rank 0 calls pa_comm_unique_id (128 bytes), the host side ships the bytes to the other ranks
 * out of band (torch.distributed store / any channel), every rank calls pa_engine_comm_init.          */
int pa_comm_unique_id(void* out, size_t cap);
int pa_engine_comm_init(pa_engine* eng, const void* unique_id, size_t id_bytes, int nranks, int rank);
void pa_engine_comm_destroy(pa_engine* eng);
int pa_engine_bcast_weights(pa_engine* eng, pa_model* m, int root);
/* same, with a separate source on the root: the root sends src's blob, EVERY rank (the root too) receives into dst, a
 * model created from a NULL blob; other ranks pass src = NULL                                               */
int pa_engine_bcast_weights_from(pa_engine* eng, pa_model* src, pa_model* dst, int root);
/* in-place broadcast of nbytes of device memory (e.g. the ball tracker's background median) */
int pa_engine_bcast(pa_engine* eng, void* dev_ptr, size_t nbytes, int root);
/* max over ranks of one double (bench: step time of the slowest rank) */
int pa_engine_allreduce_max(pa_engine* eng, double* value);
/* ABI v5 (round 6) — the sharded runner's result gather on the communicator the library owns, instead of torch.distributed
 * (trackers/runner.py has no counterpart: the reference runs one process).  Every rank contributes `nbytes` bytes of HOST memory
 * (its packed partial results; lengths differ per rank, 0 allowed).  Two calls, two collectives, no padding to the longest rank:
 * pa_engine_gather_sizes — ncclAllGather of the lengths: sizes[r] = rank r's nbytes, on every rank;
 * pa_engine_gather       — one ncclSend per rank / nranks - 1 ncclRecv on the root inside a group: on `root`, `recv` (capacity
 *                          recv_cap >= sum of sizes) receives the buffers back to back in rank order; other ranks pass recv = NULL.
 * `sizes` of the second call are the first call's.  nranks == 1 (or no communicator): host copies.                          */
int pa_engine_gather_sizes(pa_engine* eng, size_t nbytes, uint64_t* sizes);
int pa_engine_gather(pa_engine* eng, const void* send, size_t nbytes, void* recv, size_t recv_cap, const uint64_t* sizes, int root);

/* ---- host-native ByteTrack: `self.byte_track.update_with_detections(detections)`,
 * trackers/players_tracker/players_tracker.py:367-369 (constructed at :311 with frame_rate = fps; supervision
 * defaults track_activation_threshold .25, lost_track_buffer 30, minimum_matching_threshold .8).  Stateful and
 * sequential in frame order; pure host code (no GPU needed).  One call consumes a batch of frames in order:
 * boxes n_frames x stride x 6 {x1,y1,x2,y2,conf,cls} (pa_yolo_infer layout, stride = max_det), counts n_frames,
 * keep (optional) n_frames x stride bytes — 0 drops the box before tracking (polygon-zone filter,
 * players_tracker.py:364-365); out_ids n_frames x stride: public track id of each box, -1 = dropped
 * (unmatched / unconfirmed / filtered).  Thresholds are doubles: the same values the Python twin compares with.     */
typedef struct pa_bytetrack pa_bytetrack;
int pa_bytetrack_create(double track_activation_threshold, int lost_track_buffer, double minimum_matching_threshold,
                        int frame_rate, pa_bytetrack** out);
void pa_bytetrack_destroy(pa_bytetrack* b);
void pa_bytetrack_reset(pa_bytetrack* b);
int pa_bytetrack_update_batch(pa_bytetrack* b, const float* boxes, const int32_t* counts, const uint8_t* keep,
                              int n_frames, int stride, int32_t* out_ids);

/* ---- profiling (bench.py roofline): per-op device times of the LAST inference, HIP events on the
 * engine's stream.  kinds/ms/flops are host arrays of capacity cap; returns the number of records. */
int pa_engine_set_profiling(pa_engine* eng, int enable);
int pa_model_last_profile(pa_model* m, int cap, int32_t* kinds, float* ms, double* flops, int32_t* ksizes);
/* same records as CSV text: kind,ksize,M,cout,cin,stride,mf,nf,ms,flops,res,tile,family per line (mf, nf: the REQUESTED workgroup
 * tile's pixels and channels; res: 1 if the conv adds a residual input it has to read; tile, family: the tile id the conv
 * dispatcher launched after every fall-through and the tag of the kernel family that ran — h2t, h2d, h2s, h2s3, h2p, h2q, h2r,
 * h2v, h2w | bx3t, bx3p | tap | tap16, tap16d, p16, p16q; -1 and empty for ops that are not convs); returns bytes written */
int pa_model_profile_text(pa_model* m, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PADEL_HIP_H */
