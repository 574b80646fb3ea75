// Host-only decisions about a graph (graph_plan.h).  No HIP runtime call: compiled with g++ like conv_select.cpp, and driven on
// the CPU by tests/graph_plan_main.cpp.
#include "graph_plan.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace padel {

#define FAIL(...)                                                \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        err = _b;                                                \
        return 1;                                                \
    } while (0)

// ------------------------------------------------------------------------------- model description
int validate_desc(const pa_model_desc* d, size_t n_floats, std::string& err) {
    if (d->n_bufs <= 0 || d->n_ops <= 0 || !d->bufs || !d->ops) FAIL("model desc: empty graph");
    const bool f16 = d->dtype == PA_DTYPE_F16, h2 = d->dtype == PA_DTYPE_H2;
    if (d->dtype != PA_DTYPE_F32 && d->dtype != PA_DTYPE_F16 && d->dtype != PA_DTYPE_H2) FAIL("model desc: dtype %d", d->dtype);
    // (a TASK_TRACKNET graph in fp16 is a generic op list run through pa_tracknet_infer — conv unit tests; the ball
    // session itself is fp32 only, see pa_ball_create)
    const int kalign = f16 ? 31 : 15, valign = f16 ? 7 : 3;      // conv K granularity, 16-byte vector granularity (elements)
    for (int i = 0; i < d->n_bufs; ++i)
        if (d->bufs[i].level < 0 || d->bufs[i].level > 6 || d->bufs[i].channels <= 0 || (d->bufs[i].channels & 3))
            FAIL("model desc: buffer %d (level %d, channels %d)", i, d->bufs[i].level, d->bufs[i].channels);
    auto okslice = [&](int b, int off, int c) {
        return b >= 0 && b < d->n_bufs && off >= 0 && c > 0 && off + c <= d->bufs[b].channels;
    };
    if (h2)          // h2 buffers are made of whole 16-channel groups (the fp32 head maps excepted)
        for (int i = 0; i < d->n_bufs; ++i)
            if (!is_head_buf(*d, i) && (d->bufs[i].channels & 15)) FAIL("model desc: h2 buffer %d has %d channels", i, d->bufs[i].channels);
    for (int i = 0; i < d->n_ops; ++i) {
        const pa_op_desc& o = d->ops[i];
        // (the pooled linear head writes no buffer: its cout counts outputs kept by the model, checked with the op below)
        if (o.kind != PA_OP_GAP_FC && !okslice(o.out_buf, o.out_choff, o.cout)) FAIL("op %d: bad output slice", i);
        // fp16 pools / upsample move 16-byte vectors at pixel x width halves (pool5_kernel<f16x8>, maxpool2_kernel<f16x8>,
        // upsample2x_kernel<f16x8>): a width of 8k + 4 halves would misalign every second pixel
        if (f16 && (o.kind == PA_OP_SPPF_POOL || o.kind == PA_OP_UPSAMPLE2X || o.kind == PA_OP_MAXPOOL2) &&
            ((d->bufs[o.out_buf].channels & 7) || (o.in_buf >= 0 && o.in_buf < d->n_bufs && (d->bufs[o.in_buf].channels & 7))))
            FAIL("op %d: fp16 pool / upsample buffers must be a multiple of 8 channels wide", i);
        const bool from_netin = o.kind == PA_OP_STEM || o.kind == PA_OP_STEM7;      // reads the u8 network input, not a buffer
        if (h2 && !from_netin && (((o.in_choff | o.cin) & 15) || (!is_head_buf(*d, o.out_buf) && (o.out_choff & 3))))
            FAIL("op %d: h2 slices must start on a 16-channel group", i);
        if (!from_netin && !okslice(o.in_buf, o.in_choff, o.cin)) FAIL("op %d: bad input slice", i);
        if (o.kind == PA_OP_CONV) {
            if ((o.cin & kalign) || (o.in_choff & valign) || (o.ksize != 1 && o.ksize != 3) || (o.stride != 1 && o.stride != 2))
                FAIL("op %d: unsupported conv (cin %d choff %d k %d s %d)", i, o.cin, o.in_choff, o.ksize, o.stride);
            if (o.npad < o.cout || (o.npad & 15)) FAIL("op %d: npad %d for cout %d", i, o.npad, o.cout);
            const size_t ksteps3 = (size_t)h2_ksteps(o.cin, o.ksize);      // (the bf16x3 planes walk K in the same k-steps)
            const size_t wn = h2 ? (size_t)o.npad * ksteps3 * 32 : (size_t)o.npad * o.cin * o.ksize * o.ksize / (f16 ? 2 : 1);
            if (o.w_off < 0 || (o.w_off & 3) || (size_t)o.w_off + wn > n_floats || o.b_off < 0 ||
                (size_t)o.b_off + o.npad > n_floats)
                FAIL("op %d: weights outside the blob", i);
            if (o.res_buf >= 0 && !okslice(o.res_buf, o.res_choff, o.cout)) FAIL("op %d: bad residual slice", i);
            if (o.flags & PA_CONV_RES_PREACT) {
                if (o.res_buf < 0) FAIL("op %d: PA_CONV_RES_PREACT without a residual slice", i);
                if (f16) FAIL("op %d: PA_CONV_RES_PREACT is not implemented for fp16 storage (h2 and fp32 / bf16x3 models only)", i);
            }
            if (h2) {
                if (o.reserved <= 0 || (o.reserved & 3) || (size_t)o.reserved + o.npad > n_floats) FAIL("op %d: h2 row scales outside the blob", i);
                if (o.res_buf >= 0 && (o.res_choff & 3)) FAIL("op %d: h2 residual slice alignment", i);
            } else if (o.reserved < 0 || (o.reserved & 3) || (o.reserved > 0 && (size_t)o.reserved + (size_t)o.npad * 48 * ksteps3 > n_floats))
                FAIL("op %d: bf16x3 weights outside the blob", i);
            const int lin = d->bufs[o.in_buf].level, lout = d->bufs[o.out_buf].level;
            if (lout != lin + (o.stride == 2 ? 1 : 0)) FAIL("op %d: level mismatch", i);
        } else if (o.kind == PA_OP_STEM) {
            if ((o.cout & 15) || (size_t)o.w_off + (size_t)o.cout * 27 > n_floats || (size_t)o.b_off + o.cout > n_floats)
                FAIL("op %d: bad stem", i);
            if (d->bufs[o.out_buf].level != 1) FAIL("op %d: stem output must be level 1", i);
        } else if (o.kind == PA_OP_SPPF_POOL) {
            if ((o.cin & valign) || (o.in_choff & valign) || o.in_buf != o.out_buf || !okslice(o.in_buf, o.in_choff, 4 * o.cin))
                FAIL("op %d: bad sppf slices", i);
        } else if (o.kind == PA_OP_UPSAMPLE2X) {
            if (d->bufs[o.out_buf].level != d->bufs[o.in_buf].level - 1 || o.cin != o.cout || ((o.cin | o.in_choff | o.out_choff) & valign))
                FAIL("op %d: bad upsample", i);
        } else if (o.kind == PA_OP_MAXPOOL2) {
            if (d->bufs[o.out_buf].level != d->bufs[o.in_buf].level + 1 || o.cin != o.cout || ((o.cin | o.in_choff | o.out_choff) & valign))
                FAIL("op %d: bad maxpool", i);
        } else if (o.kind == PA_OP_MAXPOOL3S2) {
            if (f16) FAIL("op %d: MaxPool2d(3, 2, 1) is not implemented for fp16 storage", i);
            if (d->bufs[o.out_buf].level != d->bufs[o.in_buf].level + 1 || o.cin != o.cout || ((o.cin | o.in_choff | o.out_choff) & 3))
                FAIL("op %d: bad 3x3 stride-2 maxpool", i);
        } else if (o.kind == PA_OP_STEM7) {
            if (f16) FAIL("op %d: the 7x7 stem is not implemented for fp16 storage", i);
            if (o.cout != 64 || o.w_off < 0 || (o.w_off & 3) || (size_t)o.w_off + 148 * 64 > n_floats || o.b_off < 0 || (o.b_off & 3) ||
                (size_t)o.b_off + 64 > n_floats || o.reserved <= 0 || (size_t)o.reserved + 768 > n_floats || (o.out_choff & (h2 ? 15 : 3)) ||
                (o.act != PA_ACT_RELU && o.act != PA_ACT_NONE))
                FAIL("op %d: bad 7x7 stem", i);
            if (d->bufs[o.out_buf].level != 1) FAIL("op %d: stem output must be level 1", i);
        } else if (o.kind == PA_OP_GAP_FC) {
            if (f16) FAIL("op %d: the pooled linear head is not implemented for fp16 storage", i);
            if (o.out_buf != o.in_buf || (o.cin & 3) || (o.in_choff & 3) || o.cin > kGapFcMaxC || o.cout < 1 || o.cout > kGapFcMaxOut || o.w_off < 0 ||
                (size_t)o.w_off + (size_t)o.cout * o.cin > n_floats || o.b_off < 0 || (size_t)o.b_off + o.cout > n_floats || o.act != PA_ACT_SIGMOID)
                FAIL("op %d: bad pooled linear head", i);
            for (int k = 0; k < i; ++k) if (d->ops[k].kind == PA_OP_GAP_FC) FAIL("op %d: a graph has one pooled linear head", i);
        } else if (o.kind == PA_OP_DWCONV3) {
            if (f16) FAIL("op %d: the depthwise conv is not implemented for fp16 storage", i);
            if (o.ksize != 3 || o.stride != 1 || o.cin != o.cout || ((o.cin | o.in_choff | o.out_choff) & 3) ||
                d->bufs[o.out_buf].level != d->bufs[o.in_buf].level || (o.act != PA_ACT_NONE && o.act != PA_ACT_SILU))
                FAIL("op %d: bad depthwise conv (3x3, stride 1, cin = cout, act none | SiLU)", i);
            if (o.w_off < 0 || (o.w_off & 3) || (size_t)o.w_off + (size_t)9 * o.cin > n_floats || o.b_off < 0 || (o.b_off & 3) ||
                (size_t)o.b_off + o.cin > n_floats)
                FAIL("op %d: weights outside the blob", i);
            if (h2 && is_head_buf(*d, o.in_buf)) FAIL("op %d: a depthwise conv cannot read an fp32 head map of an h2 model", i);
            if (o.in_buf == o.out_buf && o.in_choff < o.out_choff + o.cout && o.out_choff < o.in_choff + o.cin)
                FAIL("op %d: a depthwise conv cannot write the slice it reads", i);
            if (o.res_buf >= 0 && (!okslice(o.res_buf, o.res_choff, o.cout) || (o.res_choff & 3) || d->bufs[o.res_buf].level != d->bufs[o.out_buf].level ||
                                   (h2 && is_head_buf(*d, o.res_buf))))
                FAIL("op %d: bad residual slice", i);
        } else if (o.kind == PA_OP_PSA_ATTN) {
            if (f16) FAIL("op %d: PSA attention is not implemented for fp16 storage", i);
            if (o.ksize != 32 || o.npad != 64)
                FAIL("op %d: PSA attention is implemented for key dim 32 and head dim 64 only (got kd %d, hd %d)", i, o.ksize, o.npad);
            if (o.stride < 1 || o.cin != o.stride * 128 || o.cout != o.stride * 64 || ((o.in_choff | o.out_choff) & 3) ||
                d->bufs[o.out_buf].level != d->bufs[o.in_buf].level)
                FAIL("op %d: bad PSA attention (heads %d, cin %d, cout %d)", i, o.stride, o.cin, o.cout);
            if (h2 && is_head_buf(*d, o.in_buf)) FAIL("op %d: PSA attention cannot read an fp32 head map of an h2 model", i);
            if (o.in_buf == o.out_buf && o.in_choff < o.out_choff + o.cout && o.out_choff < o.in_choff + o.cin)
                FAIL("op %d: PSA attention cannot write the slice it reads", i);
        } else {
            FAIL("op %d: unknown kind %d", i, o.kind);
        }
    }
    if (d->task == PA_TASK_DETECT || d->task == PA_TASK_POSE) {
        for (int l = 0; l < 3; ++l) {
            const int b = d->head_buf[l];
            if (b < 0 || b >= d->n_bufs || d->bufs[b].channels < 64 + d->nc + d->nk || d->bufs[b].level != 3 + l ||
                d->bufs[b].channels != d->bufs[d->head_buf[0]].channels)
                FAIL("model desc: head buffer %d", l);
        }
        if (d->nk && (d->kpt_dim < 2 || d->kpt_dim > 3 || d->nk % d->kpt_dim)) FAIL("model desc: kpt shape");
    }
    return 0;
}

// nn.Upsample(scale_factor=2) + torch.cat is never materialised where the consumer allows it.  Upsample op j
// (coarse slice S[so, so + c) -> fine slice X[xo, xo + c)) is absorbed by conv i when: i is a stride-1 conv of an h2 model or
// with bf16x3 weights — 1x1 (YOLOv8's FPN joins) or 3x3 with cin % 32 == 0 (TrackNet's decoder blocks) — whose input slice
// starts at X[xo] and covers the c channels (c % 32 == 0), nothing else reads those channels of X, and nothing overwrites the
// source slice between j and i.  Whether the absorption is USED is decided per replay by the step builder (launch_plan.cpp:
// request_conv under tuning fold_up; the coarse map is attached and kept where resolve_conv names a kernel that reads it — the
// 1x1 tap tiles, and for a 3x3 consumer the patch kernel); the upsample op is a step iff that conv did not keep it: one decision.  The liveness plan keeps S
// alive until i either way.
void find_upsample_folds(const pa_model_desc& d, std::vector<int>& fold_src, std::vector<int>& fold_dst) {
    const int nops = d.n_ops;
    fold_src.assign(nops, -1);
    fold_dst.assign(nops, -1);
    auto overlap = [](int a0, int an, int b0, int bn) { return a0 < b0 + bn && b0 < a0 + an; };
    for (int j = 0; j < nops; ++j) {
        const pa_op_desc& u = d.ops[j];
        if (u.kind != PA_OP_UPSAMPLE2X || (u.cin & 31)) continue;
        if (is_head_buf(d, u.out_buf)) continue;
        int reader = -1, readers = 0;
        for (int k = 0; k < nops; ++k) {
            const pa_op_desc& o = d.ops[k];
            if (k == j) continue;
            bool reads = false;
            if (o.kind == PA_OP_CONV) {
                reads = (o.in_buf == u.out_buf && overlap(o.in_choff, o.cin, u.out_choff, u.cin)) ||
                        (o.res_buf == u.out_buf && overlap(o.res_choff, o.cout, u.out_choff, u.cin));
            } else if (o.kind == PA_OP_DWCONV3) {
                reads = (o.in_buf == u.out_buf && overlap(o.in_choff, o.cin, u.out_choff, u.cin)) ||
                        (o.res_buf >= 0 && o.res_buf == u.out_buf && overlap(o.res_choff, o.cout, u.out_choff, u.cin));
            } else if (o.kind == PA_OP_SPPF_POOL) {
                reads = o.in_buf == u.out_buf && overlap(o.in_choff, 4 * o.cin, u.out_choff, u.cin);
            } else if (o.kind != PA_OP_STEM && o.kind != PA_OP_STEM7) {
                reads = o.in_buf == u.out_buf && overlap(o.in_choff, o.cin, u.out_choff, u.cin);
            }
            if (reads) { reader = k; ++readers; }
        }
        if (readers != 1 || reader < j) continue;
        const pa_op_desc& c = d.ops[reader];
        const bool shape_ok = c.kind == PA_OP_CONV && c.stride == 1 && (c.ksize == 1 || (c.ksize == 3 && (c.cin & 31) == 0));
        if (!shape_ok || c.reserved <= 0 || c.in_buf != u.out_buf || c.in_choff != u.out_choff || c.cin < u.cin ||
            fold_src[reader] >= 0)
            continue;
        bool clobbered = false;
        for (int k = j + 1; k < reader && !clobbered; ++k) {
            const pa_op_desc& o = d.ops[k];
            const int wc = o.kind == PA_OP_SPPF_POOL ? 4 * o.cin : o.cout;
            clobbered = o.out_buf == u.in_buf && overlap(o.out_choff, wc, u.in_choff, u.cin);
        }
        if (clobbered) continue;
        fold_src[reader] = j;
        fold_dst[j] = reader;
    }
}

bool stem_fusable(const pa_model_desc& d, size_t i) {
    if (i + 1 >= (size_t)d.n_ops) return false;
    const pa_op_desc& st = d.ops[i];
    const pa_op_desc& c = d.ops[i + 1];
    if (c.kind != PA_OP_CONV || c.ksize != 3 || c.stride != 2 || c.in_buf != st.out_buf || c.in_choff != st.out_choff || c.cin != st.cout ||
        c.res_buf >= 0)
        return false;
    if (is_head_buf(d, st.out_buf)) return false;
    for (size_t k = 0; k < (size_t)d.n_ops; ++k) {
        if (k == i || k == i + 1) continue;
        const pa_op_desc& o = d.ops[k];
        if (o.kind != PA_OP_STEM && o.in_buf == st.out_buf) return false;
        if ((o.kind == PA_OP_CONV || o.kind == PA_OP_DWCONV3) && o.res_buf == st.out_buf) return false;
    }
    return true;
}

bool stem_cv1_fusable(const pa_model_desc& d, size_t i) {
    if (d.dtype != PA_DTYPE_H2 || !stem_fusable(d, i) || i + 2 >= (size_t)d.n_ops) return false;
    const pa_op_desc& l1 = d.ops[i + 1];
    const pa_op_desc& c = d.ops[i + 2];
    if (l1.act != PA_ACT_SILU || !(l1.flags & PA_CONV_W_SINGLE) || is_head_buf(d, l1.out_buf)) return false;
    if (c.kind != PA_OP_CONV || c.ksize != 1 || c.stride != 1 || c.act != PA_ACT_SILU || !(c.flags & PA_CONV_W_SINGLE) || c.res_buf >= 0) return false;
    if (c.in_buf != l1.out_buf || c.in_choff != l1.out_choff || c.cin != l1.cout) return false;      // all of layer 1's output, nothing else
    if (c.out_buf == l1.out_buf || c.out_buf == d.ops[i].out_buf) return false;
    for (size_t k = 0; k < (size_t)d.n_ops; ++k) {          // layer 1's map has no other reader (any op that touches its buffer counts)
        if (k == i + 1 || k == i + 2) continue;
        const pa_op_desc& o = d.ops[k];
        const bool reads_in = o.kind != PA_OP_STEM && o.kind != PA_OP_STEM7;
        if (reads_in && o.in_buf == l1.out_buf) return false;
        if ((o.kind == PA_OP_CONV || o.kind == PA_OP_DWCONV3) && o.res_buf == l1.out_buf) return false;
        if (o.kind != PA_OP_GAP_FC && o.out_buf == l1.out_buf) return false;      // nor another writer: its bytes are not there
    }
    return true;
}

HeadTail find_head_tail(const pa_model_desc& d, const std::vector<int>& fold_src) {
    HeadTail none, t;
    if ((d.task != PA_TASK_DETECT && d.task != PA_TASK_POSE) || d.dtype != PA_DTYPE_H2 || d.nc < 1 || d.nk < 0) return none;
    for (int l = 0; l < 3; ++l)
        if (d.head_buf[l] < 0 || d.head_buf[l] >= d.n_bufs) return none;
    const int want = d.nk > 0 ? 3 : 2;
    for (int i = 0; i < d.n_ops; ++i) {
        const pa_op_desc& o = d.ops[i];
        const bool reads_in = o.kind != PA_OP_STEM && o.kind != PA_OP_STEM7;
        if (reads_in && is_head_buf(d, o.in_buf)) return none;                       // somebody reads a head map
        if ((o.kind == PA_OP_CONV || o.kind == PA_OP_DWCONV3) && o.res_buf >= 0 && is_head_buf(d, o.res_buf)) return none;
        if (o.kind == PA_OP_GAP_FC || !is_head_buf(d, o.out_buf)) continue;          // (the pooled linear head writes no buffer)
        int l = 0;
        while (d.head_buf[l] != o.out_buf) ++l;
        if (d.head_buf[(l + 1) % 3] == o.out_buf || d.head_buf[(l + 2) % 3] == o.out_buf) return none;      // one buffer for two levels
        if (o.kind != PA_OP_CONV || o.ksize != 1 || o.stride != 1 || o.act != PA_ACT_NONE || o.res_buf >= 0) return none;
        if (i < (int)fold_src.size() && fold_src[i] >= 0) return none;
        const int c = o.out_choff == 0 ? 0 : o.out_choff == 64 ? 1 : (d.nk > 0 && o.out_choff == 64 + d.nc) ? 2 : -1;
        if (c < 0 || o.cout != (c == 0 ? 64 : c == 1 ? d.nc : d.nk) || t.op[l][c] >= 0) return none;
        for (int k = i + 1; k < d.n_ops; ++k)                                        // its input must still be there after the op list
            if (d.ops[k].kind != PA_OP_GAP_FC && d.ops[k].out_buf == o.in_buf) return none;
        t.op[l][c] = i;
    }
    for (int l = 0; l < 3; ++l)
        for (int c = 0; c < want; ++c)
            if (t.op[l][c] < 0) return none;
    t.found = true;
    return t;
}

// ------------------------------------------------------------------------------- activation memory plan
// Every logical buffer of the graph needs batch * H * W * channels floats, but most
// are dead most of the time (a C2f's scratch dies with the C2f): buffers whose live ranges on the op list do not
// overlap share bytes of ONE arena (first-fit by offset over the buffers ordered by first use).  A buffer is
// live from the first op that touches it to the last one; the network input of a TrackNet graph (buffer 0) is
// live from before op 0, head buffers stay live past the last op (decode / NMS / pa_yolo_read_head read them), and so do the
// inputs of a head tail the caller passes (find_head_tail).
// Aliased bytes always hold finite fp32 activations, so a zero-weighted pad channel still contributes exactly 0.
int plan_activations(const pa_model_desc& d, const std::vector<int>& fold_src, int net_h, int net_w, int batch, bool alias,
                     BufferPlan& out, std::string& err, const HeadTail* tail) {
    int maxl = 0;
    for (int i = 0; i < d.n_bufs; ++i) maxl = std::max(maxl, d.bufs[i].level);
    const int mask = (1 << maxl) - 1;
    if ((net_h & mask) || (net_w & mask)) FAIL("network input %dx%d is not a multiple of %d", net_h, net_w, mask + 1);
    const int nb = d.n_bufs, nops = d.n_ops;
    std::vector<int> first(nb, nops + 1), last(nb, -2);
    auto touch = [&](int b, int i) { if (b >= 0 && b < nb) { first[b] = std::min(first[b], i); last[b] = std::max(last[b], i); } };
    for (int i = 0; i < nops; ++i) {
        const pa_op_desc& o = d.ops[i];
        if (o.kind != PA_OP_STEM && o.kind != PA_OP_STEM7) touch(o.in_buf, i);
        touch(o.out_buf, i);
        if ((o.kind == PA_OP_CONV || o.kind == PA_OP_DWCONV3) && o.res_buf >= 0) touch(o.res_buf, i);
        if (o.kind == PA_OP_CONV && fold_src[i] >= 0) touch(d.ops[fold_src[i]].in_buf, i);   // an absorbed upsample's source
    }
    if (d.task == PA_TASK_TRACKNET) touch(0, -1);
    const bool f16 = d.dtype == PA_DTYPE_F16;
    for (int l = 0; l < 3; ++l) touch(d.head_buf[l], nops + 1);
    if (tail && tail->found)          // the fused head tail reads its convs' inputs after the op list
        for (int l = 0; l < 3; ++l)
            for (int c = 0; c < 3; ++c)
                if (tail->op[l][c] >= 0) touch(d.ops[tail->op[l][c]].in_buf, nops + 1);
    // fp16 models: the head maps are the only fp32 buffers; they never share bytes with fp16 buffers, so a pad
    // channel that is read under a zero weight always holds a finite fp16 value, never reinterpreted fp32 bits
    if (f16) for (int l = 0; l < 3; ++l) touch(d.head_buf[l], -1);
    std::vector<size_t> bytes(nb), off(nb, 0);
    size_t logical = 0;
    for (int i = 0; i < nb; ++i) {
        const size_t H = net_h >> d.bufs[i].level, W = net_w >> d.bufs[i].level;
        const size_t es = (f16 && !is_head_buf(d, i)) ? 2 : 4;
        bytes[i] = ((size_t)batch * H * W * d.bufs[i].channels * es + kConvReadSlack + 255) & ~(size_t)255;
        logical += bytes[i];
    }
    size_t total = 0;
    if (alias) {
        std::vector<int> order(nb);
        for (int i = 0; i < nb; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return first[a] < first[b]; });
        std::vector<int> act;                                     // placed buffers still live, sorted by offset
        for (int b : order) {
            if (last[b] < first[b]) continue;                     // never touched: offset 0, never accessed
            act.erase(std::remove_if(act.begin(), act.end(), [&](int a) { return last[a] < first[b]; }), act.end());
            size_t o = 0;
            for (int a : act) {
                if (o + bytes[b] <= off[a]) break;
                o = std::max(o, off[a] + bytes[a]);
            }
            off[b] = o;
            act.insert(std::upper_bound(act.begin(), act.end(), b, [&](int x, int y) { return off[x] < off[y]; }), b);
            total = std::max(total, o + bytes[b]);
        }
    } else {
        for (int i = 0; i < nb; ++i) { off[i] = total; total += bytes[i]; }
    }
    out.off = std::move(off);
    out.bytes = std::move(bytes);
    out.arena_bytes = total;
    out.logical_bytes = logical;
    return 0;
}

// ------------------------------------------------------------------------------- YOLO preprocessing geometry and head levels
int yolo_geometry(int h0, int w0, int imgsz, int pre_mode, int letterbox_auto, YoloGeometry& g, std::string& err) {
    const int S = imgsz;
    if (S <= 0 || (S & 31)) FAIL("imgsz %d must be a positive multiple of 32", S);
    if (pre_mode == PA_PRE_LETTERBOX) {
        const double r = std::min((double)S / h0, (double)S / w0);
        g.rw = (int)std::nearbyint(w0 * r);
        g.rh = (int)std::nearbyint(h0 * r);
        double dw = S - g.rw, dh = S - g.rh;
        if (letterbox_auto) { dw = std::fmod(dw, 32.0); dh = std::fmod(dh, 32.0); }
        dw /= 2; dh /= 2;
        g.top = (int)std::nearbyint(dh - 0.1);
        const int bottom = (int)std::nearbyint(dh + 0.1);
        g.left = (int)std::nearbyint(dw - 0.1);
        const int right = (int)std::nearbyint(dw + 0.1);
        g.net_h = g.rh + g.top + bottom;
        g.net_w = g.rw + g.left + right;
        if (w0 == g.rw && h0 == g.rh) g.lb_mode = 0;
        else if (w0 == 2 * g.rw && h0 == 2 * g.rh) g.lb_mode = 1;
        else g.lb_mode = 2;
    } else if (pre_mode == PA_PRE_PIL_STRETCH) {
        g.net_h = g.net_w = S;
        g.rw = g.rh = S; g.top = g.left = 0; g.lb_mode = 0;
    } else {
        FAIL("unknown pre_mode %d", pre_mode);
    }
    int a0 = 0;
    for (int l = 0; l < 3; ++l) {
        g.lv[l].H = g.net_h >> (3 + l);
        g.lv[l].W = g.net_w >> (3 + l);
        g.lv[l].stride = 8 << l;
        g.lv[l].anchor0 = a0;
        a0 += g.lv[l].H * g.lv[l].W;
    }
    g.A = a0;
    if (g.A >= 65536) FAIL("%d anchors per image exceed the 16-bit sort key", g.A);
    g.P2 = 1;
    while (g.P2 < g.A) g.P2 <<= 1;
    return 0;
}

// ---- host-side coefficient tables --------------------------------------------------------------
// cv2.resize INTER_LINEAR u8: source index and the two 11-bit weights per output (oracle/yolov8_ref.py:cv2_linear_coeffs is the
// numpy statement of the same arithmetic; tests/test_letterbox_geometry_host.py compares them number for number).
// The fraction is SINGLE precision on purpose: OpenCV's generic resize path declares `float fx` and does
// `fx = (float)((dx + 0.5) * scale_x - 0.5); sx = cvFloor(fx); fx -= sx; cbuf[0] = 1.f - fx; cbuf[1] = fx;`, then
// `saturate_cast<short>(cbuf[k] * 2048)` (half to even).  Double precision here gives another weight, by one unit, on a few outputs
// of most odd size pairs (725 -> 362, output 71: 620 / 1428 in float, 619 / 1429 in double) and on none of a 16:9 source to 640.
// This rests on reading OpenCV's source; it has not been checked against a run of cv2 (none is installed where this is tested).
void cv2_linear_table(int src, int dst, std::vector<int32_t>& tab) {
    tab.resize((size_t)dst * 3);
    const double scale = (double)src / dst;
    for (int d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= s;
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src - 1) { s = src - 1; f = 0.f; }
        tab[d * 3 + 0] = s;
        tab[d * 3 + 1] = (int)std::nearbyint((1.f - f) * 2048.f);
        tab[d * 3 + 2] = (int)std::nearbyint(f * 2048.f);
    }
}

// Pillow ImagingResample precompute_coeffs + normalize_coeffs_8bpc, bicubic a = -0.5
static double pil_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static double pil_bilinear(double x) {          // Pillow's triangle filter (Image.BILINEAR), support 1
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
int pil_coeffs(int in_size, int out_size, std::vector<int32_t>& bounds, std::vector<int32_t>& kk, int filter) {
    const double scale = (double)in_size / out_size;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == PIL_BILINEAR ? 1.0 : 2.0) * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            const double arg = (x + xmin - center + 0.5) * ss;
            k[x] = filter == PIL_BILINEAR ? pil_bilinear(arg) : pil_bicubic(arg);
            ww += k[x];
        }
        for (int x = 0; x < xmax; ++x) {
            double v = ww != 0.0 ? k[x] / ww : k[x];
            kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << 22)) : (int)(0.5 + v * (1 << 22));
        }
        bounds[xx * 2] = xmin;
        bounds[xx * 2 + 1] = xmax;
    }
    return ksize;
}

// ------------------------------------------------------------------------------- YUV 4:2:0 -> BGR
int yuv_validate(int n, int h, int w, const pa_yuv_desc* d, size_t* span, std::string& err) {
    if (!d) FAIL("pa_yuv420_to_bgr: descriptor is NULL");
    if (w < 2 || h < 2 || (w & 1) || (h & 1)) FAIL("pa_yuv420_to_bgr: %d x %d frames: 4:2:0 needs an even width and height of at least 2", w, h);
    if (n < 1 || n > 65535) FAIL("pa_yuv420_to_bgr: n = %d frames outside [1, 65535]", n);
    if (d->layout != PA_YUV_NV12 && d->layout != PA_YUV_I420) FAIL("pa_yuv420_to_bgr: unknown layout %d", d->layout);
    const bool nv12 = d->layout == PA_YUV_NV12;
    const int crow = nv12 ? w : w / 2;                    // bytes of one chroma row
    if (d->pitch_y < w) FAIL("pa_yuv420_to_bgr: pitch_y %d is smaller than a luma row of %d bytes", d->pitch_y, w);
    if (d->pitch_c < crow) FAIL("pa_yuv420_to_bgr: pitch_c %d is smaller than a chroma row of %d bytes", d->pitch_c, crow);
    if (d->off_u < 0 || d->off_v < 0) FAIL("pa_yuv420_to_bgr: negative plane offset (off_u %d, off_v %d)", d->off_u, d->off_v);
    if (nv12 && d->off_v != d->off_u + 1) FAIL("pa_yuv420_to_bgr: NV12 needs off_v == off_u + 1 (off_u %d, off_v %d)", d->off_u, d->off_v);
    const long long y_end = (long long)(h - 1) * d->pitch_y + w;
    const long long c_len = (long long)(h / 2 - 1) * d->pitch_c + crow;
    const long long extent = std::max(y_end, std::max(d->off_u + c_len, nv12 ? 0ll : d->off_v + c_len));
    if (extent > 0x7fffffffll) FAIL("pa_yuv420_to_bgr: a frame of %lld bytes is beyond 2 GiB", extent);
    if (d->frame_stride < extent)
        FAIL("pa_yuv420_to_bgr: frame_stride %lld is smaller than the %lld bytes the planes of one frame span (they would overlap the next frame)",
                (long long)d->frame_stride, extent);
    // the formula stays inside int32 for every byte value (the named tables reach 5.94e8)
    const auto mag = [](int32_t c) { return (long long)(c < 0 ? -(long long)c : c); };
    const long long worst = 255 * mag(d->cy) + (1 << 19) + 128 * std::max(mag(d->cvr), std::max(mag(d->cug) + mag(d->cvg), mag(d->cub)));
    if (d->y_off < 0 || d->y_off > 255 || worst > 0x7fffffffll) FAIL("pa_yuv420_to_bgr: coefficients leave int32 (worst case %lld) or y_off %d outside [0, 255]", worst, d->y_off);
    *span = (size_t)(n - 1) * (size_t)d->frame_stride + (size_t)extent;
    return 0;
}

}  // namespace padel
