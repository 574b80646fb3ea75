// Stand-alone harness over csrc/conv_select.cpp (tests/test_conv_select_host.py builds it with g++; no GPU, no HIP runtime).
//
// stdin, one conv layer per line:
//   path B H W Ho Wo cin cout npad k stride w_single copies in_cs up_c requested
//     path       tap | bx3 | h2 | f16
//     w_single   the op carries PA_CONV_W_SINGLE and the tuning allows the two-product kernels
//     copies     1: the engine has built its operand-order weight copies (ConvArgs::wr is set where conv_wants_operand_copy says)
//     up_c       > 0: an nn.Upsample(2) of up_c channels in front of this conv is a candidate for absorption (ConvArgs::in2)
//     requested  forced tile id, or -1: the chooser's
// stdout, one line per layer:
//   chosen resolved family bm bn copy absorbed
//     chosen     the chooser's tile (always computed, without in2 — as the engine does)
//     resolved   the tile that runs after every fall-through, -1: not supported;  family: its tag, "-": none
//     bm bn      conv_tile_shape of the REQUESTED tile (0 0: not a tile of the path)
//     copy       conv_wants_operand_copy;  absorbed: the upsample is read through in2 (request_conv, the function the engine's step builder uses)
//
// -DCONV_SELECT_PARENT: the same main against a commit that predates conv_select.cpp (its conv .hip objects + libamdhip64): only
// the four choosers exist there, `copy` is that commit's own condition (its engine.cpp: ensure_operand_copies; the engine has since been split, csrc/engine_internal.h), the other columns print
// as "-".  This is how tests/golden/conv_tile_choices.json was recorded.
#include "kernels.h"
#ifndef CONV_SELECT_PARENT
#include "launch_plan.h"
#endif

#include <cstdio>
#include <cstring>

using namespace padel;

int main() {
    static float dummy[64];
    static unsigned flag;
    char path[16];
    int B, H, W, Ho, Wo, cin, cout, npad, k, stride, ws, copies, in_cs, up_c, req;
    while (scanf("%15s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", path, &B, &H, &W, &Ho, &Wo, &cin, &cout, &npad, &k, &stride, &ws, &copies,
                 &in_cs, &up_c, &req) == 16) {
        const bool h2 = !strcmp(path, "h2"), bx3 = !strcmp(path, "bx3"), f16 = !strcmp(path, "f16");
        ConvArgs a{};
        a.in = a.w = a.bias = a.zeros = dummy;
        a.out = dummy;
        a.in_cs = in_cs; a.out_cs = npad;
        a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
        a.cin = cin; a.cout = cout; a.n16 = npad / 16; a.ksize = k; a.stride = stride;
        a.M = B * Ho * Wo;
        a.w3 = bx3 ? (const void*)dummy : nullptr;
#ifdef CONV_SELECT_PARENT
        const bool few = cin == 16 || cin == 32 || cin == 48, whole = stride == 1 && (cin & 31) == 0 && cin >= 64;
        const bool s2 = k == 3 && stride == 2 && (cin & 31) == 0 && cin >= 32 && ws;
        const bool copy = (k == 3 && (whole || few)) || s2 || (k == 1 && whole && ws);
#else
        const bool copy = conv_wants_operand_copy(k, stride, cin, ws != 0);
#endif
        if (h2) {
            a.oscale = dummy; a.ovf_flag = &flag; a.w_single = ws;
            a.wr = (copies && copy) ? (const void*)dummy : nullptr;
        }
        const int chosen = h2 ? choose_conv_h2_variant(a) : f16 ? choose_conv_tap16_variant(a) : bx3 ? choose_conv_bx3_variant(a) : choose_conv_tap_variant(a.M, a.n16);
#ifdef CONV_SELECT_PARENT
        printf("%d - - - - %d -\n", chosen, (int)copy);
#else
        const int p = h2 ? CONV_PATH_H2 : f16 ? CONV_PATH_F16 : bx3 ? CONV_PATH_BX3 : CONV_PATH_TAP;
        const ConvUp up{dummy, up_c, 0, up_c};
        const ConvRequest r = request_conv(p, a, req, (up_c > 0 && (h2 || bx3)) ? &up : nullptr);          // the engine's own rule (launch_plan.cpp)
        int bm = 0, bn = 0;
        conv_tile_shape(p, r.tile, &bm, &bn);
        printf("%d %d %s %d %d %d %d\n", chosen, r.ran.tile, r.resolved ? r.ran.family : "-", bm, bn, (int)copy, a.in2 ? 1 : 0);
#endif
    }
    return 0;
}
