// Host-only: what one replay of an op list launches (launch_plan.h).  No HIP runtime call: compiled with g++ like graph_plan.cpp and
// conv_select.cpp, and driven on the CPU by tests/launch_plan_main.cpp.  This is the only place that knows which op becomes a
// launch (an absorbed upsample and layer 1 behind a fused stem do not) and which pointer, stride and size each launch gets.
#include "launch_plan.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace padel {

int choose_conv_tile(int path, const ConvArgs& a) {
    return path == CONV_PATH_H2 ? choose_conv_h2_variant(a) : path == CONV_PATH_F16 ? choose_conv_tap16_variant(a)
           : path == CONV_PATH_BX3 ? choose_conv_bx3_variant(a) : choose_conv_tap_variant(a.M, a.n16);
}

ConvRequest request_conv(int path, ConvArgs& a, int forced, const ConvUp* up) {
    ConvRequest r{forced >= 0 ? forced : choose_conv_tile(path, a), false, ConvLaunched{-1, ""}, CONV_TAP};
    if (up) {          // the first up_c channels come from the coarse map
        a.in2 = up->in2; a.in2_cs = up->cs; a.in2_choff = up->choff; a.up_c = up->c;
        if ((r.resolved = resolve_conv(path, a, r.tile, &r.ran, &r.family))) return r;
        a.in2 = nullptr; a.in2_cs = a.in2_choff = a.up_c = 0;          // no kernel of this tile's chain reads it: the upsample runs
    }
    r.resolved = resolve_conv(path, a, r.tile, &r.ran, &r.family);
    if (!r.resolved) r.ran = ConvLaunched{-1, ""};
    return r;
}

// stem (h2 output, c = 16 / 32 / 48 channels) followed by a 3x3 stride-2 conv over exactly those channels with 2c outputs
bool stem_l1_h2_supported(const StemArgs& st, const ConvArgs& a) {
    const int c = st.cout;
    return st.out_f16 == 2 && (c == 16 || c == 32 || c == 48) && a.ksize == 3 && a.stride == 2 && a.cin == c && a.n16 * 16 == 2 * c &&
           a.cout == 2 * c && a.H == st.Ho && a.W == st.Wo && a.Ho == (st.Ho + 1) / 2 && a.Wo == (st.Wo + 1) / 2 && a.w && a.oscale &&
           a.ovf_flag && !a.in2 && !a.res && (st.Ho & 1) == 0 && (st.Wo & 1) == 0;
}

// ... with cv1, a 1x1 stride-1 conv over exactly that conv's 2c outputs with 2c outputs of its own, as the kernel's third phase.  The
// first line is what launch_stem_l1_h2 asks before it picks a register-weights instantiation: the third phase exists in those only
bool stem_l1_cv1_h2_supported(const StemArgs& st, const ConvArgs& a, const ConvArgs& b) {
    return stem_l1_h2_supported(st, a) && a.w_single && a.wr && st.opw && (st.W & 3) == 0 && !(a.tune & kTunePrevGen) &&
           a.act == ACT_SILU && !a.out_f32 && a.out &&
           b.ksize == 1 && b.stride == 1 && b.cin == a.cout && b.cout == a.cout && b.n16 * 16 == b.cout && b.H == a.Ho && b.W == a.Wo &&
           b.Ho == a.Ho && b.Wo == a.Wo && b.M == a.M && b.in == a.out && b.in_cs == a.out_cs && b.in_choff == a.out_choff &&
           b.w_single && b.wr && b.w && b.bias && b.oscale && b.out && b.ovf_flag && !b.in2 && !b.res;
}

size_t stem_l1_operand_bytes(int cout) { return (size_t)(cout / 16) * 2048 + (size_t)cout * sizeof(float); }

size_t operand_copy_offsets(const pa_model_desc& d, const std::vector<char>& stem_fuse, std::vector<long long>& off) {
    off.assign(d.n_ops, -1);
    size_t total = 0;
    for (int i = 0; i < d.n_ops; ++i) {
        const pa_op_desc& o = d.ops[i];
        if (o.kind == PA_OP_STEM && stem_fuse[i] && (o.cout == 16 || o.cout == 32 || o.cout == 48)) {
            off[i] = (long long)total;             // the fused stem + layer-1 kernel's stem operand block
            total += (stem_l1_operand_bytes(o.cout) + 2047) / 2048 * 2048;
            continue;
        }
        // (the 1x1 behind a fused stem + layer 1 is read from a copy at every width: conv_wants_operand_copy stops at cin = 64, and
        //  the third phase of stem_l1_h2.hip also takes the 32 -> 32 layer of a yolov8n graph)
        const bool stem_cv1 = i >= 2 && stem_fuse[i - 2] == 2;
        if (o.kind != PA_OP_CONV || !(stem_cv1 || conv_wants_operand_copy(o.ksize, o.stride, o.cin, (o.flags & PA_CONV_W_SINGLE) != 0))) continue;
        off[i] = (long long)total;
        total += conv_h2r_copy_bytes(o.npad / 16, o.cin, o.ksize);
    }
    return total;
}

namespace {

struct Builder {
    const pa_model_desc& d;
    const std::vector<int>& fold_src;
    const Tuning& t;
    const PlanPointers& p;
    int net_h, net_w, n;

    const void* operand_copy(int i) const { return (p.wr_off && p.wr_off[i] >= 0) ? (const void*)(p.wr + p.wr_off[i]) : nullptr; }

    // ConvArgs of conv op i, its path (kernel choice: bf16x3 by default, tap kernels by tuning, conv_tap16 for fp16 models), the
    // tile it is requested with (a forced variant picks the tile of whichever path is selected) and what that resolves to.  An
    // absorbed upsample (find_upsample_folds) is attached where the requested tile resolves to a kernel that reads it: the 1x1
    // tap tiles, and for a 3x3 consumer the patch kernel.  -> resolved
    bool conv(int i, Step& st) const {
        const pa_op_desc& o = d.ops[i];
        const pa_buf_desc& ob = d.bufs[o.out_buf];
        const pa_buf_desc& ib = d.bufs[o.in_buf];
        const int Ho = net_h >> ob.level, Wo = net_w >> ob.level;
        ConvArgs& a = st.conv;
        a = ConvArgs{};
        a.in = p.bptr[o.in_buf]; a.in_cs = ib.channels; a.in_choff = o.in_choff;
        a.out = p.bptr[o.out_buf]; a.out_cs = ob.channels; a.out_choff = o.out_choff;
        a.res = o.res_buf >= 0 ? p.bptr[o.res_buf] : nullptr;
        a.res_cs = o.res_buf >= 0 ? d.bufs[o.res_buf].channels : 0; a.res_choff = o.res_choff;
        a.res_pre = (o.res_buf >= 0 && (o.flags & PA_CONV_RES_PREACT)) ? 1 : 0;
        a.zeros = p.zeros;
        a.w = p.blob + o.w_off; a.bias = p.blob + o.b_off;
        a.H = net_h >> ib.level; a.W = net_w >> ib.level; a.Ho = Ho; a.Wo = Wo;
        a.cin = o.cin; a.cout = o.cout; a.n16 = o.npad / 16; a.ksize = o.ksize; a.stride = o.stride; a.act = o.act;
        a.M = n * Ho * Wo;
        fill_fastdiv((unsigned)(Ho * Wo), &a.howo_magic, &a.howo_shift);
        fill_fastdiv((unsigned)Wo, &a.wo_magic, &a.wo_shift);
        a.tune = t.tune; a.tap_pd = t.tap_pd;
        const bool f16 = d.dtype == PA_DTYPE_F16, h2 = d.dtype == PA_DTYPE_H2;
        const bool use_bx3 = !f16 && !h2 && t.impl == 2 && o.reserved > 0;
        a.w3 = use_bx3 ? (const void*)(p.blob + o.reserved) : nullptr;
        a.out_f32 = (f16 || h2) && is_head_buf(d, o.out_buf);
        st.path = h2 ? CONV_PATH_H2 : f16 ? CONV_PATH_F16 : use_bx3 ? CONV_PATH_BX3 : CONV_PATH_TAP;
        if (h2) {
            a.oscale = p.blob + o.reserved;
            a.ovf_flag = p.ovf;
            a.w_single = (o.flags & PA_CONV_W_SINGLE) && t.w_single ? 1 : 0;
            a.wr = operand_copy(i);
        }
        if (f16) a.f16_flag = p.ovf;          // the fp16 family's range guard (f16_epilogue.h)
        ConvUp up{};
        const bool fold = (h2 || use_bx3) && t.fold_up && fold_src[i] >= 0;
        if (fold) {
            const pa_op_desc& u = d.ops[fold_src[i]];
            up = ConvUp{p.bptr[u.in_buf], d.bufs[u.in_buf].channels, u.in_choff, u.cin};
        }
        const ConvRequest r = request_conv(st.path, a, t.variant, fold ? &up : nullptr);
        st.requested = r.tile; st.ran = r.ran; st.family = r.family;
        return r.resolved;
    }

    void stem(int i, StemArgs& a) const {
        const pa_op_desc& o = d.ops[i];
        const pa_buf_desc& ob = d.bufs[o.out_buf];
        a = StemArgs{};
        a.in = p.netin; a.w = p.blob + o.w_off; a.bias = p.blob + o.b_off;
        a.out = p.bptr[o.out_buf]; a.out_cs = ob.channels; a.out_choff = o.out_choff;
        a.H = net_h; a.W = net_w; a.Ho = net_h >> ob.level; a.Wo = net_w >> ob.level; a.cout = o.cout; a.B = n;
        a.out_f16 = d.dtype == PA_DTYPE_F16 ? 1 : d.dtype == PA_DTYPE_H2 ? 2 : 0;
        a.ovf_flag = p.ovf;
        a.opw = operand_copy(i);
    }
};

int refuse(std::vector<Step>& out, std::string& err, const char* fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof(b), fmt, ap);
    va_end(ap);
    err = b;
    out.clear();
    return 1;
}

}  // namespace

int build_steps(const pa_model_desc& d, const std::vector<int>& fold_src, const std::vector<char>& stem_fuse,
                const HeadTail& tail, const Tuning& t, const PlanPointers& p, int net_h, int net_w, int n, std::vector<Step>& out,
                std::string& err, const char* not_supported) {
    const Builder b{d, fold_src, t, p, net_h, net_w, n};
    const bool h2 = d.dtype == PA_DTYPE_H2;
    out.clear();
    int cv1_op = -1;          // the conv that the fused stem step in front of it also carries (Step::has_cv1)
    for (int i = 0; i < d.n_ops; ++i) {
        const pa_op_desc& o = d.ops[i];
        const pa_buf_desc& ob = d.bufs[o.out_buf];
        const int Ho = net_h >> ob.level, Wo = net_w >> ob.level;
        Step st{};
        st.op = i; st.n_ops = 1; st.kind = o.kind; st.ran = ConvLaunched{-1, ""};
        st.stem_cv1 = i == cv1_op;
        for (int l = 0; l < 3 && tail.found; ++l)
            for (int c = 0; c < 3; ++c) st.tail = st.tail || tail.op[l][c] == i;
        if (o.kind == PA_OP_CONV) {
            const bool resolved = b.conv(i, st);
            const ConvArgs& a = st.conv;
            // act(conv + bias + residual) exists in the h2 and bf16x3 epilogues; the other families refuse instead of applying the other order
            if (a.res_pre && st.path != CONV_PATH_H2 && st.path != CONV_PATH_BX3)
                return refuse(out, err, "op %d: PA_CONV_RES_PREACT needs the h2 or the bf16x3 kernels (tuning impl = 2, bf16x3 weights in the blob), not the %s family",
                              i, st.path == CONV_PATH_F16 ? "fp16" : "fp32-MFMA tap");
            if (!resolved) return refuse(out, err, "op %d (kind %d) launch failed: %s", i, o.kind, not_supported);
            if (a.in2)          // the upsample in front of it is read through in2: it is no launch
                for (size_t k = out.size(); k-- > 0;)
                    if (out[k].op == fold_src[i]) { out.erase(out.begin() + (long)k); break; }
            conv_tile_shape(st.path, st.requested, &st.mf, &st.nf);            // profile rows carry BM, BN of the REQUESTED workgroup tile
            st.ksize = o.ksize; st.flops = 2.0 * a.M * (double)o.cout * o.cin * o.ksize * o.ksize;
            st.M = a.M; st.cout = o.cout; st.cin = o.cin; st.stride = o.stride; st.res = a.res != nullptr;
        } else if (o.kind == PA_OP_STEM) {
            b.stem(i, st.stem);
            st.ksize = 3; st.flops = 2.0 * n * Ho * Wo * (double)o.cout * 27;
            // tuning "fuse_stem": the stem and the stride-2 3x3 behind it (its only reader) as one kernel; the conv is no step of
            // its own (the profile shows both under the stem's record)
            if (t.fuse_stem && h2 && stem_fuse[i]) {
                b.conv(i + 1, st);
                if (stem_l1_h2_supported(st.stem, st.conv)) {
                    st.n_ops = 2;
                    // tuning "fuse_stem_cv1": the 1x1 behind layer 1 (its only reader: stem_fuse == 2) as the kernel's third phase.
                    // That conv KEEPS its step, marked `stem_cv1`: a replay that profiles or collects a timeline runs it there
                    if (t.fuse_stem_cv1 && stem_fuse[i] == 2) {
                        Step c1{};
                        if (b.conv(i + 2, c1) && stem_l1_cv1_h2_supported(st.stem, st.conv, c1.conv)) { st.cv1 = c1.conv; st.has_cv1 = true; cv1_op = i + 2; }
                    }
                    ++i;
                } else {
                    st.conv = ConvArgs{};              // two launches: the conv has its own turn
                }
                st.path = st.requested = 0; st.family = CONV_TAP; st.ran = ConvLaunched{-1, ""};          // (a stem's row names no conv kernel)
            }
        } else if (o.kind == PA_OP_SPPF_POOL) {
            st.sl = SliceArgs{p.bptr[o.in_buf], d.bufs[o.in_buf].channels, o.in_choff, nullptr, 0, 0, o.cin, n, Ho, Wo, 0, 0, (int)d.dtype, t.fuse_sppf,
                              nullptr, nullptr, 0, nullptr, nullptr};
            st.ksize = 5;
        } else if (o.kind == PA_OP_UPSAMPLE2X) {
            // a step unless its fold_dst conv keeps in2: that conv's turn takes it out again (same decision, made once)
            st.sl = SliceArgs{p.bptr[o.in_buf], d.bufs[o.in_buf].channels, o.in_choff, p.bptr[o.out_buf], ob.channels, o.out_choff, o.cin, n, Ho / 2, Wo / 2,
                              0, 0, (int)d.dtype, 0, nullptr, nullptr, 0, nullptr, nullptr};
        } else if (o.kind == PA_OP_MAXPOOL2) {
            st.sl = SliceArgs{p.bptr[o.in_buf], d.bufs[o.in_buf].channels, o.in_choff, p.bptr[o.out_buf], ob.channels, o.out_choff, o.cin, n, Ho * 2, Wo * 2,
                              0, 0, (int)d.dtype, 0, nullptr, nullptr, 0, nullptr, nullptr};
            st.ksize = 2;
        } else if (o.kind == PA_OP_MAXPOOL3S2) {
            const int lin = d.bufs[o.in_buf].level;
            st.sl = SliceArgs{p.bptr[o.in_buf], d.bufs[o.in_buf].channels, o.in_choff, p.bptr[o.out_buf], ob.channels, o.out_choff, o.cin, n,
                              net_h >> lin, net_w >> lin, Ho, Wo, h2 ? 1 : 0, 0, nullptr, nullptr, 0, nullptr, nullptr};
            st.ksize = 3;
        } else if (o.kind == PA_OP_STEM7) {
            if (!p.netin) return refuse(out, err, "op %d: the 7x7 stem reads the u8 network input of pa_resnet_infer", i);
            Stem7Args& a = st.stem7;
            a = Stem7Args{};
            a.in = p.netin; a.w = p.blob + o.w_off; a.bias = p.blob + o.b_off; a.lut = p.blob + o.reserved;
            a.out = p.bptr[o.out_buf]; a.out_cs = ob.channels; a.out_choff = o.out_choff;
            a.H = net_h; a.W = net_w; a.Ho = Ho; a.Wo = Wo; a.B = n; a.act = o.act;
            a.out_h2 = (h2 && !is_head_buf(d, o.out_buf)) ? 1 : 0;
            a.ovf_flag = p.ovf;
            st.ksize = 7; st.flops = 2.0 * n * Ho * Wo * 64.0 * 147.0;
            st.M = n * Ho * Wo; st.cout = 64; st.cin = 3; st.stride = 2;
        } else if (o.kind == PA_OP_GAP_FC) {
            const int lin = d.bufs[o.in_buf].level;
            st.sl = SliceArgs{p.bptr[o.in_buf], d.bufs[o.in_buf].channels, o.in_choff, nullptr, 0, 0, o.cin, n, (net_h >> lin) * (net_w >> lin), 0, 0, 0,
                              h2 ? 1 : 0, 0, p.blob + o.w_off, p.blob + o.b_off, o.cout, p.fc, p.fc + (size_t)p.p_batch * kGapFcMaxOut};
            st.flops = 2.0 * n * (double)o.cout * o.cin;
            st.M = n; st.cout = o.cout; st.cin = o.cin;
        } else if (o.kind == PA_OP_DWCONV3) {
            DwConvArgs& a = st.dw;
            a = DwConvArgs{};
            a.in = p.bptr[o.in_buf]; a.in_cs = d.bufs[o.in_buf].channels; a.in_choff = o.in_choff;
            a.w = p.blob + o.w_off; a.bias = p.blob + o.b_off;
            a.out = p.bptr[o.out_buf]; a.out_cs = ob.channels; a.out_choff = o.out_choff;
            if (o.res_buf >= 0) { a.res = p.bptr[o.res_buf]; a.res_cs = d.bufs[o.res_buf].channels; a.res_choff = o.res_choff; }
            a.C = o.cin; a.B = n; a.H = Ho; a.W = Wo; a.act = o.act;
            a.h2 = h2 ? 1 : 0; a.out_f32 = (h2 && is_head_buf(d, o.out_buf)) ? 1 : 0; a.ovf_flag = p.ovf;
            st.ksize = 3; st.flops = 2.0 * n * Ho * Wo * (double)o.cin * 9.0;
            st.M = n * Ho * Wo; st.cout = o.cout; st.cin = o.cin; st.stride = 1; st.res = o.res_buf >= 0;
        } else if (o.kind == PA_OP_PSA_ATTN) {
            AttnArgs& a = st.attn;
            a = AttnArgs{};
            a.heads = o.stride; a.kd = o.ksize; a.hd = o.npad;
            a.qkv = p.bptr[o.in_buf]; a.cs = d.bufs[o.in_buf].channels;
            a.q_choff = o.in_choff; a.k_choff = o.in_choff + a.heads * a.kd; a.v_choff = o.in_choff + 2 * a.heads * a.kd;
            a.out = p.bptr[o.out_buf]; a.out_cs = ob.channels; a.out_choff = o.out_choff;
            a.N = Ho * Wo; a.B = n; a.scale = (float)(1.0 / std::sqrt((double)a.kd));
            a.h2 = h2 ? 1 : 0; a.out_f32 = (h2 && is_head_buf(d, o.out_buf)) ? 1 : 0; a.ovf_flag = p.ovf;
            st.flops = 2.0 * n * (double)a.heads * a.N * (double)a.N * (a.kd + a.hd);
            st.M = n * a.N; st.cout = o.cout; st.cin = o.cin; st.stride = a.heads;
        }
        out.push_back(st);
    }
    return 0;
}

}  // namespace padel
