// Stand-alone harness over csrc/graph_plan.cpp (tests/test_graph_plan_host.py builds it with g++ against graph_plan.cpp and
// conv_select.cpp; no GPU, no HIP runtime, no engine library).
//
// stdin, lines:
//   graph n_bufs n_ops
//   task dtype nc nk kpt_dim head_buf0 head_buf1 head_buf2 in_channels n_floats
//   level channels                                         x n_bufs
//   kind in_buf in_choff cin out_buf out_choff cout ksize stride act res_buf res_choff npad reserved w_off b_off flags pad_   x n_ops
//                                                          (every field of pa_op_desc in struct order)
// then commands about the graph read last, one answer line each:
//   validate                         ->  ok | refused: <message>
//   folds                            ->  folds <upsample>:<conv> ...
//   stem                             ->  stem <op> ...                      ops for which stem_fusable holds
//   plan net_h net_w batch alias     ->  plan <arena bytes> <logical bytes> <offset>:<bytes> ... (one pair per buffer) | refused: <message>
// and commands that need no graph:
//   geometry h0 w0 imgsz pre_mode letterbox_auto  ->  geometry rw rh top left net_h net_w lb_mode H0 W0 H1 W1 H2 W2 A P2 | refused: <message>
//   cv2 src dst                      ->  cv2 <index> <w0> <w1> ...          cv2_linear_table, 3 numbers per output
//   pil in out filter                ->  pil <ksize> <bounds ...> | <coefs ...>
//
// -DGRAPH_PLAN_PARENT: the same main inside a scratch translation unit that has already included the engine.cpp of a commit
// that predates graph_plan.cpp and defined these functions (graph_plan.h's signatures) as adapters onto that commit's own
// static ones.  This is how tests/golden/graph_plan.json was recorded (tests/test_graph_plan_host.py: --record).
#ifndef GRAPH_PLAN_PARENT
#include "graph_plan.h"
using namespace padel;
#endif

#include "graph_desc_read.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

int main() {
    pa_model_desc d{};
    std::vector<pa_buf_desc> bufs;
    std::vector<pa_op_desc> ops;
    long long n_floats = 0;
    char cmd[32];
    std::string err;
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "graph")) {
            if (!read_graph(d, bufs, ops, n_floats)) return 2;
        } else if (!strcmp(cmd, "validate")) {
            if (validate_desc(&d, (size_t)n_floats, err)) printf("refused: %s\n", err.c_str());
            else printf("ok\n");
        } else if (!strcmp(cmd, "folds")) {
            std::vector<int> src, dst;
            find_upsample_folds(d, src, dst);
            printf("folds");
            for (size_t j = 0; j < dst.size(); ++j) if (dst[j] >= 0) printf(" %zu:%d", j, dst[j]);
            printf("\n");
        } else if (!strcmp(cmd, "stem")) {
            printf("stem");
            for (size_t i = 0; i < ops.size(); ++i) if (stem_fusable(d, i)) printf(" %zu", i);
            printf("\n");
        } else if (!strcmp(cmd, "plan")) {
            int nh = 0, nw = 0, batch = 0, alias = 0;
            if (scanf("%d %d %d %d", &nh, &nw, &batch, &alias) != 4) return 2;
            std::vector<int> src, dst;
            find_upsample_folds(d, src, dst);
            BufferPlan bp;
            if (plan_activations(d, src, nh, nw, batch, alias != 0, bp, err)) { printf("refused: %s\n", err.c_str()); continue; }
            printf("plan %zu %zu", bp.arena_bytes, bp.logical_bytes);
            for (size_t i = 0; i < bufs.size(); ++i) printf(" %zu:%zu", bp.off[i], bp.bytes[i]);
            printf("\n");
        } else if (!strcmp(cmd, "geometry")) {
            int h0 = 0, w0 = 0, S = 0, pre = 0, au = 0;
            if (scanf("%d %d %d %d %d", &h0, &w0, &S, &pre, &au) != 5) return 2;
            YoloGeometry g;
            if (yolo_geometry(h0, w0, S, pre, au, g, err)) { printf("refused: %s\n", err.c_str()); continue; }
            printf("geometry %d %d %d %d %d %d %d", g.rw, g.rh, g.top, g.left, g.net_h, g.net_w, g.lb_mode);
            for (int l = 0; l < 3; ++l) printf(" %d %d", g.lv[l].H, g.lv[l].W);
            printf(" %d %d\n", g.A, g.P2);
        } else if (!strcmp(cmd, "cv2")) {
            int s = 0, t = 0;
            if (scanf("%d %d", &s, &t) != 2) return 2;
            std::vector<int32_t> tab;
            cv2_linear_table(s, t, tab);
            printf("cv2");
            for (int32_t v : tab) printf(" %d", v);
            printf("\n");
        } else if (!strcmp(cmd, "pil")) {
            int s = 0, t = 0, f = 0;
            if (scanf("%d %d %d", &s, &t, &f) != 3) return 2;
            std::vector<int32_t> b, k;
            printf("pil %d", pil_coeffs(s, t, b, k, f));
            for (int32_t v : b) printf(" %d", v);
            printf(" |");
            for (int32_t v : k) printf(" %d", v);
            printf("\n");
        } else {
            fprintf(stderr, "graph_plan_main: unknown command '%s'\n", cmd);
            return 2;
        }
    }
    return 0;
}
