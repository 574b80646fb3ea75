// Stand-alone harness over the stem + layer 1 + 1x1 decisions of csrc/graph_plan.cpp and csrc/launch_plan.cpp
// (tests/test_stem_cv1_plan_host.py builds it with g++ against graph_plan.cpp, launch_plan.cpp and conv_select.cpp; no GPU, no HIP
// runtime, no engine library).
//
// stdin: graphs in the text form of tests/graph_plan_main.cpp (graph / header / buffers / ops), then commands about the graph
// read last, one answer line each:
//   fusable                         ->  fusable <op> <0 | 1 | 2> ...    per PA_OP_STEM op: 0 nothing, 1 stem_fusable, 2 stem_cv1_fusable too
//   steps net_h net_w n cv1 tune    ->  steps <op>:<n_ops>:<has_cv1>:<stem_cv1> ...    build_steps with the engine's stem_fuse values,
//                                       synthetic base pointers and operand copies, tuning fuse_stem_cv1 = cv1 and tune = tune
//   copies                          ->  copies <op>:<bytes> ...         the ops operand_copy_offsets gives a copy (engine's stem_fuse)
#include "launch_plan.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace padel;

static std::vector<char> engine_stem_fuse(const pa_model_desc& d) {
    std::vector<char> f(d.n_ops);
    for (int i = 0; i < d.n_ops; ++i) f[i] = stem_cv1_fusable(d, i) ? 2 : stem_fusable(d, i) ? 1 : 0;
    return f;
}

int main() {
    pa_model_desc d{};
    std::vector<pa_buf_desc> bufs;
    std::vector<pa_op_desc> ops;
    long long n_floats = 0;
    char cmd[32];
    std::string err;
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "graph")) {
            int nb = 0, no = 0;
            if (scanf("%d %d", &nb, &no) != 2 || nb < 0 || no < 0) return 2;
            d = pa_model_desc{};
            if (scanf("%d %d %d %d %d %d %d %d %d %lld", &d.task, &d.dtype, &d.nc, &d.nk, &d.kpt_dim, &d.head_buf[0], &d.head_buf[1], &d.head_buf[2],
                      &d.in_channels, &n_floats) != 10)
                return 2;
            bufs.assign(nb, pa_buf_desc{});
            ops.assign(no, pa_op_desc{});
            for (auto& b : bufs) if (scanf("%d %d", &b.level, &b.channels) != 2) return 2;
            for (auto& o : ops) {
                long long w_off = 0, b_off = 0;
                if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %d %d", &o.kind, &o.in_buf, &o.in_choff, &o.cin, &o.out_buf, &o.out_choff,
                          &o.cout, &o.ksize, &o.stride, &o.act, &o.res_buf, &o.res_choff, &o.npad, &o.reserved, &w_off, &b_off, &o.flags, &o.pad_) != 18)
                    return 2;
                o.w_off = w_off; o.b_off = b_off;
            }
            d.n_bufs = nb; d.bufs = bufs.data();
            d.n_ops = no; d.ops = ops.data();
        } else if (!strcmp(cmd, "fusable")) {
            const std::vector<char> f = engine_stem_fuse(d);
            printf("fusable");
            for (int i = 0; i < d.n_ops; ++i)
                if (ops[i].kind == PA_OP_STEM) printf(" %d %d", i, (int)f[i]);
            printf("\n");
        } else if (!strcmp(cmd, "copies")) {
            std::vector<long long> off;
            const std::vector<char> f = engine_stem_fuse(d);
            const size_t total = operand_copy_offsets(d, f, off);
            printf("copies");
            for (int i = 0; i < d.n_ops; ++i) {
                if (off[i] < 0) continue;
                long long next = (long long)total;
                for (int k = 0; k < d.n_ops; ++k) if (off[k] > off[i] && off[k] < next) next = off[k];
                printf(" %d:%lld", i, next - off[i]);
            }
            printf("\n");
        } else if (!strcmp(cmd, "steps")) {
            int nh = 0, nw = 0, n = 0, cv1 = 0, tune = 0;
            if (scanf("%d %d %d %d %d", &nh, &nw, &n, &cv1, &tune) != 5) return 2;
            std::vector<int> src, dst;
            find_upsample_folds(d, src, dst);
            const std::vector<char> f = engine_stem_fuse(d);
            const HeadTail tail = find_head_tail(d, src);
            std::vector<long long> wr_off;
            operand_copy_offsets(d, f, wr_off);
            // synthetic, distinct, 256-byte aligned addresses: nothing is dereferenced on the host
            std::vector<float*> bptr(bufs.size());
            for (size_t i = 0; i < bufs.size(); ++i) bptr[i] = reinterpret_cast<float*>((uintptr_t)0x10000000u * (i + 1));
            Tuning t;
            t.fuse_stem_cv1 = cv1;
            t.tune = tune;
            const PlanPointers p{bptr.data(), reinterpret_cast<const float*>((uintptr_t)0x1000), reinterpret_cast<const char*>((uintptr_t)0x2000000),
                                 wr_off.data(), reinterpret_cast<const float*>((uintptr_t)0x3000), reinterpret_cast<unsigned*>((uintptr_t)0x4000),
                                 reinterpret_cast<const uint8_t*>((uintptr_t)0x5000), nullptr, n};
            std::vector<Step> steps;
            if (build_steps(d, src, f, tail, t, p, nh, nw, n, steps, err)) { printf("refused: %s\n", err.c_str()); continue; }
            printf("steps");
            for (const Step& s : steps) printf(" %d:%d:%d:%d", s.op, s.n_ops, s.has_cv1 ? 1 : 0, s.stem_cv1 ? 1 : 0);
            printf("\n");
        } else {
            fprintf(stderr, "stem_cv1_plan_main: unknown command '%s'\n", cmd);
            return 2;
        }
    }
    return 0;
}
