// Stand-alone harness over the head-tail decisions of csrc/graph_plan.cpp (tests/test_head_tail_plan_host.py builds it with g++
// against graph_plan.cpp and conv_select.cpp; no GPU, no HIP runtime, no engine library).
//
// stdin: graphs in the text form of tests/graph_plan_main.cpp (graph / header / buffers / ops), then commands about the graph
// read last, one answer line each:
//   tail                                  ->  tail 0 | tail 1 <box op> <class op> <keypoint op | -1>  x 3 levels
//   plan net_h net_w batch alias with     ->  plan <arena bytes> <logical bytes> <offset>:<bytes> ...   with = 1: the tail's inputs
//                                             stay live to the end (what the engine plans), 0: plan_activations without a tail
#include "graph_plan.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace padel;

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
        } else if (!strcmp(cmd, "tail")) {
            std::vector<int> src, dst;
            find_upsample_folds(d, src, dst);
            const HeadTail t = find_head_tail(d, src);
            printf("tail %d", t.found ? 1 : 0);
            if (t.found)
                for (int l = 0; l < 3; ++l) for (int c = 0; c < 3; ++c) printf(" %d", t.op[l][c]);
            printf("\n");
        } else if (!strcmp(cmd, "plan")) {
            int nh = 0, nw = 0, batch = 0, alias = 0, with = 0;
            if (scanf("%d %d %d %d %d", &nh, &nw, &batch, &alias, &with) != 5) return 2;
            std::vector<int> src, dst;
            find_upsample_folds(d, src, dst);
            const HeadTail t = find_head_tail(d, src);
            BufferPlan bp;
            if (plan_activations(d, src, nh, nw, batch, alias != 0, bp, err, with ? &t : nullptr)) { printf("refused: %s\n", err.c_str()); continue; }
            printf("plan %zu %zu", bp.arena_bytes, bp.logical_bytes);
            for (size_t i = 0; i < bufs.size(); ++i) printf(" %zu:%zu", bp.off[i], bp.bytes[i]);
            printf("\n");
        } else {
            fprintf(stderr, "head_tail_plan_main: unknown command '%s'\n", cmd);
            return 2;
        }
    }
    return 0;
}
