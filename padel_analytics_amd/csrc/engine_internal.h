// Shared by the engine's translation units (engine*.cpp); not part of the C-ABI (include/padel_hip.h).
//   engine.cpp           engine and model lifecycle, tuning, memory and timer calls, the arena, the replay of a step list (run_ops /
//                        run_graph), profile text
//   engine_pre.cpp       preprocessing shared by the model families: frame staging, the Pillow resample, YUV -> BGR
//   engine_yolo.cpp      YOLO plan (per lane), prepare, enqueue, post-processing, tickets and their lanes, read-backs
//   engine_tracknet.cpp  pa_tracknet_infer and the ball session
//   engine_resnet.cpp    the ResNet-50 court-keypoint regressor
//   engine_render.cpp    pa_render: marks on BGR frames -> BGR / YUV 4:2:0 (the refusals and the font: render_check.cpp, host only)
//   engine_warp.cpp      pa_warp_perspective: BGR frames through a homography each (the refusals: warp_check.cpp, host only)
//   engine_heat.cpp      pa_heat_accumulate: density maps on the top-down canvases (the refusals: heat_check.cpp, host only)
//   engine_jpeg.cpp      pa_jpeg_encode: YUV 4:2:0 frames in HBM -> baseline JPEGs in host memory (the refusals, tables and header: jpeg_check.cpp, host only)
//   engine_jpeg_decode.cpp  pa_jpeg_decode: baseline JPEGs in host memory -> BGR frames in HBM (the markers: jpeg_parse.cpp, host only)
//   engine_activity.cpp  pa_frame_activity, pa_frames_median: frame statistics for the court-view filter (the refusals: activity_check.cpp, host only);
//                        pa_box_histograms: colour histograms of player boxes (the refusals: box_histogram_check.cpp, host only)
//   engine_comm.cpp      RCCL
//   device_mem.h         DevMem<T> / PinMem<T>: the owner of every device (page-locked host) allocation of these files; the
//                        hooks it allocates through, and the count of live bytes, are engine.cpp's
// What is decided about a graph on the host alone lives in graph_plan.cpp, which kernel runs a conv in conv_select.cpp, what one
// replay launches and with which arguments (struct Tuning, struct Step) in launch_plan.cpp.
#pragma once
#include "../../include/padel_hip.h"
#include "graph_plan.h"
#include "launch_plan.h"
#include "lane_plan.h"
#include "device_mem.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

using namespace padel;

struct pa_comm;
struct JpegScratch;
struct JpegDecScratch;

struct pa_engine {
    int dev = 0;
    // The main stream: everything but the YOLO lanes runs on it, and it is what orders the engine's work (padel_hip.h).  It is
    // handed out by main_stream() alone, which counts the hand-outs: a lane forks from the main stream (fork_lane) only when
    // something other than a ticket's join was put on it since that lane last forked, so a user that did not go through the
    // accessor would be work a lane does not wait for.  The member is private: such a use does not compile.
    hipStream_t main_stream() { ++main_seq_; return main_; }
    // ... and for a host-side wait alone (hipStreamSynchronize, a null test): nothing is enqueued, so nothing is counted — a wait
    // between two submits must not put the second ticket's lane behind the first ticket's join.  What the host does after such a
    // wait is complete before the next submit is made, so no lane has to fork for it.  Never hand this to a call that enqueues.
    hipStream_t main_stream_wait_only() const { return main_; }
    hipError_t create_streams();                 // engine.cpp
    void destroy_streams();
    // lane_stream[i] waits for what the main stream holds (nothing to do when only joins were enqueued since its last fork)
    hipError_t fork_lane(int i);
    // the main stream waits for ev, recorded on a lane stream: what is enqueued on the main stream later runs behind that ticket
    hipError_t join_lane(hipEvent_t ev) { return hipStreamWaitEvent(main_, ev, 0); }
    hipError_t sync_lanes();                     // both lane streams drained (the main stream is the caller's business)
    // The lanes' streams belong to the engine, not to the model: the runner walks its trackers one after the other, and the
    // runtime maps streams onto a handful of hardware queues (two streams on one queue do not overlap), so three models bring
    // no six streams.  A model's Lane carries the stream it runs on.
    hipStream_t lane_stream[kMaxLanes] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr;   // uploads that must not queue behind compute (pa_upload)
    std::string err;
    bool profiling = false;
    DevMem<float> zeros;      // 256 B of zeros: source of padded conv taps
    Tuning t;
    int tuning_epoch = 0;     // bumped by pa_engine_set_tuning: captured graphs of an older epoch are discarded
    std::string timeline_path;
    pa_comm* comm = nullptr;  // RCCL communicator (pa_engine_comm_init), optional
    DevMem<uint8_t> yuv_stage;   // pa_yuv420_to_bgr: raw YUV bytes of a host source, filled and read on the main stream only
    int yuv_last_path = 0;    // 1 vector, 2 byte: what the last pa_yuv420_to_bgr launched (pa_yuv_last_path)
    hipEvent_t timer_ev[2]{};  // pa_engine_timer_start / _stop, created on first use
    DevMem<uint8_t> render_stage;   // pa_render: the resolved marks and first[] of the call in flight, filled and read on the main stream only
    DevMem<uint8_t> activity_stage; // pa_frame_activity: the results and the workgroups' partial sums of the call in flight (the call is synchronous)
    DevMem<uint8_t> box_stage;      // pa_box_histograms: the rows of counters and the rectangle list of the call in flight (synchronous too)
    int render_last_path = 0; // 1 vector, 2 byte: what the last pa_render launched (pa_render_last_path)
    DevMem<uint8_t> warp_stage;     // pa_warp_perspective: the matrices and valid words of the call in flight, filled and read on the main stream only
    int warp_last_path = 0;   // 1 16-byte stores, 2 byte stores: what the last pa_warp_perspective launched (pa_warp_last_path)
    DevMem<uint8_t> heat_stage;     // pa_heat_accumulate: lut, first, valid, boxes and points of the call in flight, filled and read on the main stream only
    int heat_last_path = 0;   // 1 16-byte accesses, 2 byte accesses: what the last pa_heat_accumulate launched (pa_heat_last_path)
    JpegScratch* jpeg = nullptr;   // pa_jpeg_encode: slots, tables and the gathered frames, grown on demand, used on the main stream only (engine_jpeg.cpp)
    JpegDecScratch* jpeg_dec = nullptr;   // pa_jpeg_decode: compressed bytes, tables, coefficients and planes, likewise (engine_jpeg_decode.cpp)
    int jpeg_dec_last_path = 0;    // 1 vector, 2 byte: what the last pa_jpeg_decode launched for its colour pass (pa_jpeg_decode_last_path)
    long long jpeg_dec_split_min = 0;   // pa_jpeg_decode_set_split as given: 0 the default, -1 never; an interval of at least this many bytes is split
    int jpeg_dec_split_sub = 0;         // ... its subsequences' bytes, 0 the default
    long long jpeg_dec_last_split[4] = {0, 0, 0, 0};   // pa_jpeg_decode_last_split
private:
    hipStream_t main_ = nullptr;
    unsigned long long main_seq_ = 1;                  // hand-outs of main_
    unsigned long long forked_seq_[kMaxLanes] = {0, 0};   // main_seq_ at the lane's last fork
    hipEvent_t fork_ev_[kMaxLanes] = {nullptr, nullptr};
};

extern thread_local std::string g_err;      // errors of calls that have no engine yet (pa_last_error(NULL))

#define PA_FAIL(eng, ...)                                        \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        if (eng) (eng)->err = _b; else g_err = _b;               \
        return 1;                                                \
    } while (0)

#define PA_HIP(eng, call)                                                                  \
    do {                                                                                   \
        const hipError_t _e = static_cast<hipError_t>(call);   /* (a DevMem reports the runtime's code as int) */ \
        if (_e != hipSuccess) {                                                            \
            (void)hipGetLastError();   /* reported here: must not surface again at the next launch's hipGetLastError() */ \
            PA_FAIL(eng, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                  \
    } while (0)

struct ProfRec { int kind; int ksize; double flops; hipEvent_t e0, e1; float ms; int M, cout, cin, stride, mf, nf, res; int tile; const char* family; };      // tile, family: what the conv dispatcher launched (ConvLaunched; -1 / "" for other ops)
enum { PROF_PRE = 100, PROF_DECODE = 101, PROF_NMS = 102 };      // `kind` of the profile rows that are not ops of the graph

// The two-pass Pillow resample of u8 HWC frames (sh x sw x 3 -> dh x dw): its tables on the device and the temporary between
// the passes (engine_pre.cpp).  No table for an axis that already has the target size, d_tmp only when both axes change.
struct ResamplePlan {
    int sh = 0, sw = 0, dh = 0, dw = 0;
    DevMem<int32_t> d_hb, d_hk, d_vb, d_vk;
    int hks = 0, vks = 0;
    DevMem<uint8_t> d_tmp;   // the temporary between the passes (a second lane allocates as much)
};

// A lane: everything ONE in-flight YOLO batch writes on the device, so that two batches of a model can run at the same time on two
// streams.  Lane 0 is the plan's (every model has it; TrackNet / ResNet models use nothing else and run it on the main stream);
// lane 1 of a YOLO model is allocated by the first pa_yolo_submit that finds lane 0's ticket still in flight (lane_plan.h).
// Audit of every device pointer plan_yolo, plan_buffers, run_ops, run_post, head_tail_convs and run_tail_ops hand to a kernel.  What
// the op list's launches get is made from the base pointers of ONE struct, PlanPointers (launch_plan.h; plan_pointers in engine.cpp
// fills it per replay), and every one of them stands before the first replay of a plan and until free_plan or the model's end: the
// arena / bptr and d_fc are plan_buffers', d_netin is plan_yolo's / pa_resnet_infer's plan, released by free_lane alone; d_w and d_ovf
// are pa_model_create's, e->zeros pa_engine_create's; d_wr is allocated once by ensure_operand_copies, which run_graph calls in front
// of every replay.  A weight broadcast rewrites d_w and d_wr in place (wr_valid goes false, the copies are rebuilt into the same
// block).  A step list is rebuilt per replay and kept by no one but the lane's own vector, so it holds no pointer past these.
//   per lane (written per batch): arena / bptr (every activation, in / in2 / out / res of the convs, the head-tail convs' inputs,
//     lv[].buf), d_fc, d_stage, d_netin, the Pillow resample temporary (lane 0: ResamplePlan::d_tmp, lane 1: d_rs_tmp), d_cand,
//     d_cidx, d_ccnt, d_keys, d_order, d_supp, d_oboxes, d_okpts, d_ocnt, the timeline scratch (allocated per launch), and the
//     captured graphs, which hold these pointers;
//   shared, read-only while tickets run: d_w (w, bias, oscale, w3, lut), d_wr (wr, opw; rebuilt on the main stream, then a host
//     wait), d_xtab / d_ytab, the resample tables d_hb / d_hk / d_vb / d_vk, d_classes (replaced only after a main-stream wait,
//     which the joins make a wait for every ticket), e->zeros, the caller's frames;
//   shared, sticky by design: d_ovf (kernels only ever set it; a ticket reads it back after its own kernels, so it sees its own
//     overflow; a neighbour's can only make it report 1 early, which callers treat as "recompute").  d_frames is pa_yolo_infer's
//     alone (host frames; a submit refuses them).
// Freed by: the type.  Every member that owns device memory is a DevMem, so `L = Lane{}` (free_lane) and the model's destructor
// release a lane whole; the graphs are destroyed by free_lane, the stream is the engine's.
struct Lane {
    bool allocated = false;
    hipStream_t stream = nullptr;          // e->lane_stream[i] (YOLO models; not owned), nullptr: the model runs on the main stream
    DevMem<char> arena;                    // what bptr points into
    std::vector<float*> bptr;
    DevMem<float> d_fc;                    // graphs with a PA_OP_GAP_FC op: [max_batch][kGapFcMaxOut] logits, then as many probabilities (plan_buffers)
    DevMem<float> d_stage;                 // h2 generic graphs: fp32 input staged here before it is encoded
    DevMem<uint8_t> d_netin;
    HeadLevel lv[3]{};
    DevMem<float> d_cand; DevMem<int32_t> d_cidx, d_ccnt;
    DevMem<uint64_t> d_keys; DevMem<int32_t> d_order; DevMem<uint8_t> d_supp;
    DevMem<float> d_oboxes, d_okpts; DevMem<int32_t> d_ocnt;
    std::vector<Step> steps;               // the launches of the replay being enqueued (build_steps): rebuilt per call, capacity kept
    std::map<int, hipGraphExec_t> graphs;  // op-list replay per batch size (tuning "graph")
    std::map<int, int> graph_stem_path;    // ... and the pa_model_last_stem_path of each capture
    DevMem<uint8_t> d_rs_tmp;              // lane 1: its own temporary between the resample passes (lane 0 uses the plan's)
    LaneState st;                          // pick_lane's view
    size_t device_bytes() const {          // what the lane holds on the device (pa_model::lane_bytes)
        return arena.bytes() + d_fc.bytes() + d_stage.bytes() + d_netin.bytes() + d_cand.bytes() + d_cidx.bytes() + d_ccnt.bytes() + d_keys.bytes() +
               d_order.bytes() + d_supp.bytes() + d_oboxes.bytes() + d_okpts.bytes() + d_ocnt.bytes() + d_rs_tmp.bytes();
    }
};

struct pa_model {
    pa_engine* e = nullptr;
    pa_model_desc d{};
    std::vector<pa_buf_desc> bufs;
    std::vector<pa_op_desc> ops;
    std::vector<int> fold_src;             // conv op i -> index of the upsample op it can absorb (-1: none), find_upsample_folds
    std::vector<char> stem_fuse;           // op i -> 1: stem_fusable (the stem and the stride-2 3x3 behind it can run as one kernel), 2: stem_cv1_fusable
                                           // too (and the 1x1 behind that conv), 0: neither
    HeadTail tail;                         // the heads' last 1x1 convs, if the graph ends the way find_head_tail wants it
    DevMem<float> d_w;
    size_t n_w = 0;
    // h2 models: the h planes of the two-product stride-1 3x3 convs once more in MFMA operand order (conv_patch_h2r.hip), built on
    // the device from d_w before the first replay and again after a weight broadcast (ensure_operand_copies)
    DevMem<char> d_wr;
    std::vector<long long> wr_off;         // op -> byte offset into d_wr, -1: no copy
    bool wr_valid = false;
    DevMem<unsigned> d_ovf;                // h2 and fp16 models: sticky "a value did not fit fp16" flag (pa_model_take_overflow)
    int fc_nout = 0;                       // outputs of that op (0: the graph has none)
    int max_batch = 64;
    Lane ln[kMaxLanes];                    // ln[0]: the plan's; ln[1]: lazily, YOLO models only
    int last_lane = 0;                     // the lane of the model's last call (pa_yolo_read_head, pa_yolo_read_netin, pa_model_last_lane)
    bool lane1_refused = false;            // the second lane did not fit this plan (second_lane_fits, or a failed allocation): not tried again
    double conv_flops = 0;                 // conv FLOPs of one replay at max_batch (second_lane_wanted)
    size_t lane_bytes = 0;                 // device bytes of one lane of this plan

    // plan
    bool planned = false;
    int p_h0 = 0, p_w0 = 0, p_imgsz = 0, p_pre = 0, p_auto = 0, p_batch = 0;
    int net_h = 0, net_w = 0;
    int rw = 0, rh = 0, top = 0, left = 0, lb_mode = 0;
    size_t arena_bytes = 0, logical_bytes = 0;   // bytes of the plan with / without liveness aliasing
    unsigned h_ovf = 0;                    // overflow flag as read back by the last pa_yolo_infer calls (h2 and fp16 models)
    bool ovf_cached = false;               // h_ovf is current: no kernel of this model has run since it was read
    // pa_yolo_submit / pa_yolo_wait: tickets in flight.  slot = ticket % PA_MAX_INFLIGHT; h_pin[slot]: the overflow flag as the
    // stream read it back after that ticket's kernels (page-locked: a pageable destination would make the copy block the host)
    PinMem<unsigned> h_pin;
    hipEvent_t tk_ev[PA_MAX_INFLIGHT]{};
    bool tk_busy[PA_MAX_INFLIGHT]{};
    int tk_lane[PA_MAX_INFLIGHT]{};        // the lane a ticket in flight runs on
    int next_ticket = 0, n_inflight = 0;
    std::vector<int32_t> classes_host;     // what d_classes holds (set_classes: uploaded again only when the caller's list changes)
    int graph_epoch = -1;                  // engine tuning epoch the graphs were captured under
    DevMem<uint8_t> d_frames;
    DevMem<int32_t> d_xtab, d_ytab;                               // cv2 bilinear tables
    ResamplePlan rs;                                              // PIL tables
    // post
    int A = 0, P2 = 0;
    YoloGeometry geom;                     // of the plan (a second lane is planned from it)
    DevMem<int32_t> d_classes;
    int last_n = 0;
    int last_post_path = 0;                // pa_yolo_last_post_path: 0 decode_kernel on head maps, 1 the fused head tail
    int last_stem_path = 0;                // pa_model_last_stem_path: 1 the last replay ran the 1x1 behind layer 1 inside the fused stem kernel
    bool heads_stale = false;              // the last call ran the fused head tail: the head maps are not there (pa_yolo_read_head computes them)
    std::vector<ProfRec> prof;
    size_t n_prof = 0;
};

// ---- engine.cpp
// does the model's dtype raise d_ovf (h2 pairs and the fp16 family; fp32 models never do)?
inline bool guards_range(const pa_model* m) { return m->d.dtype == PA_DTYPE_H2 || m->d.dtype == PA_DTYPE_F16; }
// (the profile's events go onto the stream the profiled kernels run on)
ProfRec* prof_begin(pa_model* m, hipStream_t s, size_t idx, int kind, int ksize, double flops);
inline void prof_end(hipStream_t s, ProfRec* r) { if (r) hipEventRecord(r->e1, s); }
int finish_profile(pa_model* m, size_t n_rec);
void free_plan(pa_model* m);                         // both lanes; the caller has synchronised the main stream, the lanes are drained here
// the arena of one lane of a model whose net_h x net_w is set: allocation, memsets (on s), bptr, d_fc
int plan_buffers(pa_model* m, Lane& L, int batch, hipStream_t s);
void free_lane(Lane& L);                             // the graphs, then `L = Lane{}` with the stream kept; drains nothing: the CALLER has waited for the lane's stream
// run_ops on lane L and stream s, or (tuning "graph", not while profiling) the replay of its capture for this batch size.
// skip_tail: the steps marked `tail` are left out (the caller's head_fused: its run_post launches the fused kernel instead)
int run_graph(pa_model* m, Lane& L, hipStream_t s, int n, size_t* pi, bool skip_tail);
// The fused head tail applies to the next replay of a planned model: tuning fuse_head, an h2 model whose plan found the tail, a
// shape head_tail_h2.hip has, no profiling, no timeline.  Evaluated once per call (yolo_enqueue) and handed to run_graph and run_post.
bool head_fused(const pa_model* m);
void head_tail_convs(const pa_model* m, const Lane& L, HeadTailArgs& a);      // a.cv and a.w_single of a planned model (a.d: the caller's)
int run_tail_ops(pa_model* m, Lane& L, hipStream_t s, int n);   // the tail convs alone, from their inputs (still live): the head maps of the lane's last call

// ---- engine_jpeg.cpp
void jpeg_scratch_free(pa_engine* e);                 // waits for the stream first, then deletes the scratch

// ---- engine_jpeg_decode.cpp
void jpeg_dec_scratch_free(pa_engine* e);             // waits for the stream first, destroys the events, deletes the scratch

// ---- engine_pre.cpp
hipError_t upload_table(pa_engine* e, DevMem<int32_t>& d, const std::vector<int32_t>& v);
// grow d_frames to max_batch frames if need be and copy nb host frames into it (on the stream); *src then names the device copy
int stage_frames(pa_model* m, const uint8_t** src, int nb, size_t frame_bytes, hipStream_t s);
// tables + temporary for sh x sw -> dh x dw over at most max_batch frames; identity_pass: a source that already has the target
// size still gets a 1-tap vertical table (the ball session: its pass also reorders channels into 3-byte pixels)
int resample_plan(pa_engine* e, ResamplePlan* rs, int sh, int sw, int dh, int dw, int filter, int max_batch, bool identity_pass = false);
// the one or two passes (horizontal first) of n frames into dst with out_c (3 | 4) bytes per pixel; the last pass reverses channels.
// tmp: the temporary between the passes in place of the plan's (a second lane's own, as large as the plan's)
hipError_t resample_enqueue(const ResamplePlan& rs, const uint8_t* src, uint8_t* dst, int n, int out_c, int reverse, hipStream_t s, uint8_t* tmp = nullptr);
