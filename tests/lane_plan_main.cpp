// csrc/lane_plan.h on the CPU (tests/test_lane_plan_host.py): one answer line per command read from stdin.
//   pick <second_ok> <busy0> <last0> <busy1> <last1>     -> "pick <lane>"
//   wanted <lanes> <conv_flops> <gate_flops>              -> "wanted <0|1>"
//   fits <free_bytes> <lane_bytes> <arena_bytes>          -> "fits <0|1>"
//   gate                                                  -> "gate <kLaneGateFlops>"
#include "lane_plan.h"

#include <cstdio>
#include <iostream>
#include <string>

using namespace padel;

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "pick") {
            int ok = 0, b0 = 0, b1 = 0;
            LaneState ln[kMaxLanes];
            std::cin >> ok >> b0 >> ln[0].last_ticket >> b1 >> ln[1].last_ticket;
            ln[0].busy = b0 != 0; ln[1].busy = b1 != 0;
            printf("pick %d\n", pick_lane(ln, ok != 0));
        } else if (cmd == "wanted") {
            int lanes = 0;
            double flops = 0, gate = 0;
            std::cin >> lanes >> flops >> gate;
            printf("wanted %d\n", second_lane_wanted(lanes, flops, gate) ? 1 : 0);
        } else if (cmd == "fits") {
            unsigned long long fr = 0, lane = 0, arena = 0;
            std::cin >> fr >> lane >> arena;
            printf("fits %d\n", second_lane_fits((size_t)fr, (size_t)lane, (size_t)arena) ? 1 : 0);
        } else if (cmd == "gate") {
            printf("gate %.17g\n", kLaneGateFlops);
        } else {
            printf("unknown %s\n", cmd.c_str());
            return 1;
        }
    }
    return 0;
}
