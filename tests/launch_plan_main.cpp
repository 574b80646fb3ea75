// Stand-alone harness over csrc/launch_plan.cpp (tests/test_launch_plan_host.py builds it with g++ against launch_plan.cpp,
// graph_plan.cpp and conv_select.cpp; no GPU, no HIP runtime, no engine library).
//
// stdin: `graph` blocks as tests/graph_plan_main.cpp reads them (graph_desc_read.h), and commands about the graph read last:
//   tuning <key> <value> | tuning reset      a field of struct Tuning by its pa_engine_set_tuning key (kept across graphs)
//   steps net_h net_w batch n                ->  one line per step (launch_plan_print.h), [refused: <message>], end <count>
//   tail net_h net_w batch n                 ->  tail <op> ...          the ops of the steps marked `tail`
// The base pointers are made-up addresses, one region per owner, never dereferenced: the arena as plan_activations lays it out for
// `batch` (the engine's plan_buffers), the blob, the operand block (built: operand_copy_offsets), the zero page, the flag, the u8
// network input where the graph has a stem, the pooled-linear-head outputs where it has that op.
#include "graph_plan.h"
#include "launch_plan.h"
#include "launch_plan_print.h"
#include "graph_desc_read.h"

#include <cstring>

using namespace padel;

static const struct { const char* key; int Tuning::*field; } kKeys[] = {
    {"impl", &Tuning::impl}, {"variant", &Tuning::variant}, {"tune", &Tuning::tune}, {"tap_pd", &Tuning::tap_pd}, {"alias", &Tuning::alias},
    {"fold_up", &Tuning::fold_up}, {"fuse_stem", &Tuning::fuse_stem}, {"fuse_sppf", &Tuning::fuse_sppf}, {"w_single", &Tuning::w_single},
};

int main() {
    pa_model_desc d{};
    std::vector<pa_buf_desc> bufs;
    std::vector<pa_op_desc> ops;
    long long n_floats = 0;
    Tuning t;
    std::vector<Step> steps;
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "graph")) {
            if (!read_graph(d, bufs, ops, n_floats)) return 2;
        } else if (!strcmp(cmd, "tuning")) {
            char key[32];
            int v = 0;
            if (scanf("%31s", key) != 1) return 2;
            if (!strcmp(key, "reset")) { t = Tuning{}; continue; }
            if (scanf("%d", &v) != 1) return 2;
            bool known = false;
            for (const auto& k : kKeys) if (!strcmp(k.key, key)) { t.*k.field = v; known = true; }
            if (!known) { fprintf(stderr, "launch_plan_main: unknown tuning key '%s'\n", key); return 2; }
        } else if (!strcmp(cmd, "steps") || !strcmp(cmd, "tail")) {
            int nh = 0, nw = 0, batch = 0, n = 0;
            if (scanf("%d %d %d %d", &nh, &nw, &batch, &n) != 4) return 2;
            std::vector<int> fold_src, fold_dst;
            find_upsample_folds(d, fold_src, fold_dst);
            std::vector<char> stem_fuse(ops.size());
            bool has_stem = false, has_fc = false;
            for (size_t i = 0; i < ops.size(); ++i) {
                stem_fuse[i] = stem_fusable(d, i);
                has_stem = has_stem || ops[i].kind == PA_OP_STEM || ops[i].kind == PA_OP_STEM7;
                has_fc = has_fc || ops[i].kind == PA_OP_GAP_FC;
            }
            const HeadTail tail = find_head_tail(d, fold_src);
            BufferPlan bp;
            std::string err;
            if (plan_activations(d, fold_src, nh, nw, batch, t.alias != 0, bp, err, &tail)) { printf("refused: %s\nend 0\n", err.c_str()); continue; }
            std::vector<long long> wr_off;
            const size_t wr_bytes = d.dtype == PA_DTYPE_H2 ? operand_copy_offsets(d, stem_fuse, wr_off) : 0;
            const auto base = [](int k) { return (char*)((uintptr_t)k << 40); };
            std::vector<float*> bptr(bufs.size());
            lp::bufs().clear();
            for (size_t i = 0; i < bufs.size(); ++i) { bptr[i] = (float*)(base(1) + bp.off[i]); lp::bufs().push_back((const char*)bptr[i]); }
            const size_t netin_bytes = has_stem ? (size_t)batch * nh * nw * 4 : 0, fc_bytes = has_fc ? (size_t)batch * 2 * kGapFcMaxOut * sizeof(float) : 0;
            lp::regions() = {{"arena", base(1), bp.arena_bytes + kConvReadSlack}, {"blob", base(2), (size_t)n_floats * 4 + kConvReadSlack},
                             {"wr", base(3), wr_bytes ? wr_bytes + 8192 : 0}, {"zeros", base(4), 256}, {"flag", base(5), 256},
                             {"netin", base(6), netin_bytes}, {"fc", base(7), fc_bytes}};
            const PlanPointers p{bptr.data(), (const float*)base(2), wr_bytes ? base(3) : nullptr, d.dtype == PA_DTYPE_H2 ? wr_off.data() : nullptr,
                                 (const float*)base(4), (unsigned*)base(5), netin_bytes ? (const uint8_t*)base(6) : nullptr,
                                 fc_bytes ? (float*)base(7) : nullptr, batch};
            const bool refused = build_steps(d, fold_src, stem_fuse, tail, t, p, nh, nw, n, steps, err) != 0;
            if (!strcmp(cmd, "tail")) {
                printf("tail");
                for (const Step& s : steps) if (s.tail) printf(" %d", s.op);
                printf("\n");
                continue;
            }
            for (const Step& s : steps) {
                const SliceArgs& v = s.sl;
                switch (s.kind) {
                    case PA_OP_CONV: lp::conv(s.op, s.path, s.requested, s.ran, s.conv); break;
                    case PA_OP_STEM: if (s.n_ops == 2) lp::stem_l1(s.op, s.stem, s.conv); else lp::stem(s.op, s.stem); break;
                    case PA_OP_SPPF_POOL: lp::sppf(s.op, v.in, v.in_cs, v.in_choff, v.c, v.B, v.H, v.W, v.fmt, v.fused); break;
                    case PA_OP_UPSAMPLE2X: lp::resize("upsample2x", s.op, v.in, v.in_cs, v.in_choff, v.out, v.out_cs, v.out_choff, v.c, v.B, v.H, v.W, v.fmt); break;
                    case PA_OP_MAXPOOL2: lp::resize("maxpool2", s.op, v.in, v.in_cs, v.in_choff, v.out, v.out_cs, v.out_choff, v.c, v.B, v.H, v.W, v.fmt); break;
                    case PA_OP_MAXPOOL3S2: lp::maxpool3s2(s.op, v.in, v.in_cs, v.in_choff, v.out, v.out_cs, v.out_choff, v.c, v.B, v.H, v.W, v.Ho, v.Wo, v.fmt); break;
                    case PA_OP_STEM7: lp::stem7(s.op, s.stem7); break;
                    case PA_OP_GAP_FC: lp::gap_fc(s.op, v.in, v.in_cs, v.in_choff, v.c, v.B, v.H, v.w, v.bias, v.nout, v.logits, v.probs, v.fmt); break;
                    case PA_OP_DWCONV3: lp::dwconv3(s.op, s.dw); break;
                    case PA_OP_PSA_ATTN: lp::psa_attn(s.op, s.attn); break;
                }
            }
            if (refused) printf("refused: %s\n", err.c_str());
            printf("end %zu\n", steps.size());
        } else {
            fprintf(stderr, "launch_plan_main: unknown command '%s'\n", cmd);
            return 2;
        }
    }
    return 0;
}
