// What one replay of an op list launches, and with which arguments (launch_plan.cpp: host code only, no HIP runtime call; tested on
// the CPU through tests/launch_plan_main.cpp).  build_steps reads the description, the tuning, the network size, the batch and a
// handful of base pointers and returns the launches in order; the engine's loop (engine.cpp: run_ops) only walks them.
#pragma once
#include "graph_plan.h"
#include "kernels.h"

#include <string>
#include <vector>

namespace padel {

// Tuning knobs: read from the environment ONCE at pa_engine_create (PADEL_CONV_IMPL=tap|bx3, PADEL_CONV_VARIANT,
// PADEL_CONV_TUNE, PADEL_CONV_TAP_PD, PADEL_GRAPH, PADEL_ALIAS, PADEL_LANES), changed afterwards only through
// pa_engine_set_tuning — the replay loop never touches getenv.
struct Tuning {
    int impl = 2;        // 2 (default): bf16x3 kernels — fp32 values split exactly into 3 bf16, 6 products on the bf16
                         // pipe, fp32 accumulate (admitted by the same parity criteria as the fp32-MFMA kernels);
                         // 0: tap-unrolled LDS-DMA fp32-MFMA kernels, 1: LDS kernel (their bitwise cross-check)
    int variant = -1;    // forced tile id (tests / tools), -1: per-layer heuristic
    int tune = 1;        // the tuning word: kTune* below are all of its bits that anything reads.  Bits 0 and 1 (once s_setprio around MFMA
                         // clusters and a staggered workgroup start) are read by no kernel any more; the default stays 1.  The engine
                         // keeps bits 0..3 of what pa_engine_set_tuning "tune" / PADEL_CONV_TUNE give it (engine.cpp: knob_tune), so
                         // every value of the word runs product kernels
    int tap_pd = 2;      // prefetch distance of the 1x1 tap kernel
    int graph = 0;       // 1: replay the op list of a (model, batch) from a captured hipGraph
    int timeline = 0;    // 1: 3x3 tap launches of the 64x96 tile run the s_memtime-instrumented instantiation
    int alias = 1;       // 1: activation buffers share one arena by liveness, 0: disjoint ranges
    int fuse_stem = 1;   // 1: h2 YOLOv8 graphs run model.0 (stem) + model.1 (3x3 stride 2) as ONE kernel (stem_l1_h2.hip; default since round 4, 0 = two kernels)
    int fuse_stem_cv1 = 1;   // 1: where the op behind a fused stem + layer 1 is a 1x1 stride-1 two-product SiLU conv over all of layer 1's channels
                         // and layer 1's only reader (model.2.cv1; graph_plan.h: stem_cv1_fusable), the kernel computes it too and layer 1's
                         // map is never written; 0: that conv is a launch of its own.  Bitwise the same maps; off while profiling or collecting
                         // a timeline (the profile keeps the conv's row)
    int w_single = 1;    // 1 (default): h2 convs whose packed weights have an all-zero m plane (PA_CONV_W_SINGLE) skip the wm x ah product;
                         // 0 (tests): all three products everywhere — bitwise the same results
    int fuse_sppf = 1;   // 1: h2 graphs run the three chained 5x5 max-pools of SPPF as ONE kernel (sppf_h2_kernel: keys in LDS, separable passes); 0 = three launches.  Bitwise the same maps
    int fuse_head = 1;   // 1: h2 Detect / Pose models whose plan found the head tail (graph_plan.h: HeadTail) run the heads' last 1x1 convs and the
                         // decode as ONE kernel (head_tail_h2.hip) and never write the head maps; 0: the convs, then decode_kernel.  Bitwise the same
                         // detections; off while profiling or collecting a timeline (the profile keeps its rows)
    int lanes = 2;       // 2: a YOLO model whose submit finds its last ticket still in flight gets a second lane (struct Lane) and alternate
                         // tickets run on two streams; 1: everything on lane 0.  Bitwise the same results
    int fold_up = 1;     // 1: an nn.Upsample(2) whose only reader is a bf16x3 1x1 conv is never materialised (the conv
                         // fetches those channels at [y >> 1][x >> 1] of the coarse map), 0: run the upsample kernel
};
// The bits of Tuning::tune / ConvArgs::tune.  Every kernel they select computes the same results bitwise (tests pass 5, 8 and 9)
constexpr int kTuneTilePerWorkgroup = 4;     // bit 2: conv_patch_h2r.hip launches one workgroup per tile instead of 2 persistent ones per CU
constexpr int kTunePrevGen = 8;              // bit 3: the previous kernel generation — h2w instead of h2v (conv_select.cpp), the weight-ring
                                             // fused stem instead of the register-weights one (launch_plan.cpp, stem_l1_h2.hip)
constexpr int kTuneMask = 15;                // bits 0..3: what the engine keeps of a tuning word

// ---- a conv's request ------------------------------------------------------------------------------------------------
int choose_conv_tile(int path, const ConvArgs& a);      // the path's chooser (kernels.h)
// An nn.Upsample(2) in front of a conv that may be read through ConvArgs::in2 instead of being run (find_upsample_folds)
struct ConvUp { const float* in2; int cs, choff, c; };
struct ConvRequest {
    int tile;                // requested: the forced one, or the path's chooser on the arguments WITHOUT in2
    bool resolved;           // false: no kernel of the tile's chain covers the layer
    ConvLaunched ran;        // what runs after every fall-through ({-1, ""}: not resolved)
    ConvFamily family;
};
// The one rule: choose without in2, attach `up` (if any), resolve; where no kernel of the tile's chain reads the coarse map, detach
// it again (the upsample then runs) and resolve without.  a: complete but for in2 / in2_cs / in2_choff / up_c, which this sets.
ConvRequest request_conv(int path, ConvArgs& a, int forced, const ConvUp* up);

// ---- the operand-order weight copies of an h2 model (ConvArgs::wr, StemArgs::opw) -----------------------------------------
size_t stem_l1_operand_bytes(int cout);
// op -> byte offset of its copy in the operand block (-1: none); -> bytes of the block
size_t operand_copy_offsets(const pa_model_desc& d, const std::vector<char>& stem_fuse, std::vector<long long>& off);

// ---- the steps -------------------------------------------------------------------------------------------------------
// Every base pointer a step's arguments are made from.  The engine fills it from a model and one of its lanes; each is allocated
// before the first replay of a plan and lives until free_plan or the model's end (engine_internal.h: the audit at struct Lane).
struct PlanPointers {
    float* const* bptr;          // the lane's activation buffers (its arena)
    const float* blob;           // the weight blob
    const char* wr;              // the operand-copy block ...
    const long long* wr_off;     // ... and op -> offset into it (operand_copy_offsets); nullptr: the copies are not built
    const float* zeros;          // the zero page
    unsigned* ovf;               // the overflow flag
    const uint8_t* netin;        // the lane's u8 network input (nullptr: the model has none)
    float* fc;                   // the lane's pooled-linear-head outputs
    int p_batch;                 // the batch the lane was planned for (the probabilities follow p_batch rows of logits)
};

// the plain argument sets of the pool / upsample / pooled-linear-head launchers (kernels.h), under one name per parameter
struct SliceArgs {
    float* in; int in_cs, in_choff;
    float* out; int out_cs, out_choff;
    int c, B, H, W, Ho, Wo;      // H, W: the launcher's H, W (gap-fc: H = its HW); Ho, Wo: launch_maxpool3s2 only
    int fmt;                     // the launcher's last parameter: the dtype (sppf, upsample, maxpool2) or h2 0 | 1 (maxpool3s2, gap-fc)
    int fused;                   // launch_sppf_pool
    const float* w; const float* bias; int nout; float* logits; float* probs;     // launch_gap_fc
};

struct Step {
    int op, n_ops;               // the op it starts at and how many it covers (2: the fused stem + layer 1)
    int kind;                    // pa_op_desc::kind of `op`
    bool tail;                   // one of HeadTail::op[][]: the fused head tail runs it in place of this step
    ConvArgs conv;               // PA_OP_CONV, and layer 1 of a fused stem
    // The 1x1 behind layer 1 inside the fused stem kernel (tuning fuse_stem_cv1; stem_l1_cv1_h2_supported).  The stem's step carries
    // that conv's arguments (has_cv1, cv1), the conv's own step is marked stem_cv1: a plain replay launches (stem, conv, cv1) as one
    // kernel and leaves the marked step out; a replay that profiles or collects a timeline launches both steps as they are
    bool has_cv1, stem_cv1;
    ConvArgs cv1;
    int path;                    // ConvPath
    int requested;               // tile id asked for
    ConvFamily family;           // what it resolved to ...
    ConvLaunched ran;            // ... ({-1, ""}: not a conv step)
    union {                      // by kind
        StemArgs stem;           // PA_OP_STEM (n_ops == 2: launch_stem_l1_h2(stem, conv))
        Stem7Args stem7;
        DwConvArgs dw;
        AttnArgs attn;
        SliceArgs sl;            // PA_OP_SPPF_POOL, PA_OP_UPSAMPLE2X, PA_OP_MAXPOOL2, PA_OP_MAXPOOL3S2, PA_OP_GAP_FC
    };
    // the static columns of its profile row (mf, nf: the REQUESTED tile's shape; tile / family are `ran`)
    int ksize; double flops; int M, cout, cin, stride, mf, nf, res;
};

// The launches of one replay for n images, in order, into `out` (cleared first; its capacity is kept).  1: a refusal, its text in
// `err`, and `out` empty — nothing of the replay is enqueued then.  A conv that does not resolve is refused with the text the
// failed launch used to give: `not_supported` is the runtime's string for hipErrorNotSupported, which host-only code cannot ask for.
int build_steps(const pa_model_desc& d, const std::vector<int>& fold_src, const std::vector<char>& stem_fuse,
                const HeadTail& tail, const Tuning& t, const PlanPointers& p, int net_h, int net_w, int n, std::vector<Step>& out,
                std::string& err, const char* not_supported = "operation not supported");

}  // namespace padel
