// What the engine decides about a graph before anything runs (graph_plan.cpp: host code only, no HIP runtime call; tested on
// the CPU through tests/graph_plan_main.cpp): the refusals of a malformed description, which upsample is never materialised,
// which activation buffers share bytes, the letterbox geometry and the resize tables.  A refusal returns 1 with its text in `err`.
#pragma once
#include "../../include/padel_hip.h"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace padel {

inline bool is_head_buf(const pa_model_desc& d, int b) { return b == d.head_buf[0] || b == d.head_buf[1] || b == d.head_buf[2]; }

// the only thing between a malformed description and an out-of-bounds kernel read
int validate_desc(const pa_model_desc* d, size_t n_floats, std::string& err);
// fold_src: conv op i -> the upsample op it can absorb (-1: none); fold_dst: upsample op j -> its absorbing conv (-1: none)
void find_upsample_folds(const pa_model_desc& d, std::vector<int>& fold_src, std::vector<int>& fold_dst);
// op i is the stem, op i + 1 a 3x3 stride-2 conv over exactly the stem's channels, and nothing else reads the stem's output
bool stem_fusable(const pa_model_desc& d, size_t i);
// ... and, in an h2 graph, op i + 2 is a 1x1 stride-1 conv with SiLU and no residual that reads ALL of op i + 1's output and nothing
// else, both convs are two-product layers (PA_CONV_W_SINGLE), op i + 1 has SiLU, and no other op reads or writes op i + 1's buffer
// (model.2.cv1 behind model.1 of a YOLOv8 graph): the fused stem kernel may compute op i + 2 as well and never write op i + 1's map
bool stem_cv1_fusable(const pa_model_desc& d, size_t i);

// The tail of a Detect / Pose head of an h2 model: on every level the ops that write head_buf[l] are exactly a 1x1, stride-1 conv
// without activation or residual for the 64 box logits (channel 0), one for the nc class logits (channel 64) and, iff nk > 0, one
// for the nk keypoint values (channel 64 + nc); each reads a non-head buffer that no later op writes, absorbs no upsample, and
// nothing reads the head maps.  op[l][0 | 1 | 2]: the box / class / keypoint conv of level l (-1: no keypoint conv).  Anything else
// — a partial match, a test graph with one conv into a head buffer, another dtype or task — is `found == false`.  The engine may
// then run the three convs and the decode as one kernel (head_tail_h2.hip) and never write the maps.
struct HeadTail {
    bool found = false;
    int op[3][3] = {{-1, -1, -1}, {-1, -1, -1}, {-1, -1, -1}};
};
HeadTail find_head_tail(const pa_model_desc& d, const std::vector<int>& fold_src);

struct BufferPlan {
    std::vector<size_t> off, bytes;            // per logical buffer: byte offset into the arena, bytes (slack included, multiple of 256)
    size_t arena_bytes = 0, logical_bytes = 0; // bytes of the plan with / without liveness aliasing
};
// tail (optional, found): the inputs of its convs stay live past the last op, like the head maps — the fused kernel reads them
// after the op list, and pa_yolo_read_head computes the maps from them on demand
int plan_activations(const pa_model_desc& d, const std::vector<int>& fold_src, int net_h, int net_w, int batch, bool alias,
                     BufferPlan& out, std::string& err, const HeadTail* tail = nullptr);

struct YoloGeometry {
    int rw = 0, rh = 0, top = 0, left = 0, net_h = 0, net_w = 0, lb_mode = 0;   // lb_mode 0 copy, 1 exact 2x2 area, 2 cv2 bilinear tables
    struct { int H, W, stride, anchor0; } lv[3]{};
    int A = 0, P2 = 0;                         // anchors per image, the next power of two (sort scratch)
};
int yolo_geometry(int h0, int w0, int imgsz, int pre_mode, int letterbox_auto, YoloGeometry& g, std::string& err);

// cv2.resize INTER_LINEAR u8: [dst][3] = {source index, weight of it, weight of the next} in 1/2048
void cv2_linear_table(int src, int dst, std::vector<int32_t>& tab);
// Pillow ImagingResample precompute_coeffs + normalize_coeffs_8bpc: bounds [out][2] = {lo, n}, kk [out][ksize] in 1/2^22; -> ksize
enum { PIL_BICUBIC = 0, PIL_BILINEAR = 1 };
int pil_coeffs(int in_size, int out_size, std::vector<int32_t>& bounds, std::vector<int32_t>& kk, int filter = PIL_BICUBIC);

// Geometry checks of pa_yuv420_to_bgr.  *span = bytes of src the kernel may read: the last frame's start plus the extent of one
// frame's planes.
int yuv_validate(int n, int h, int w, const pa_yuv_desc* d, size_t* span, std::string& err);

}  // namespace padel
