// Lanes: which of a YOLO model's (at most two) sets of per-batch device memory the next pa_yolo_submit runs on, and whether the
// model may have the second set at all.  Host code only, no HIP call, pure functions of what the engine knows on the host;
// tested on the CPU through tests/lane_plan_main.cpp.  What a lane owns and what the lanes share: engine_internal.h (struct Lane).
#pragma once
#include <cstddef>

namespace padel {

constexpr int kMaxLanes = 2;

// second_lane_wanted's gate as the engine applies it (conv FLOPs of one replay at max_batch); 0: no gate.  profiles/lanes_ab.txt
constexpr double kLaneGateFlops = 0;

// what the host knows of a lane when a ticket is about to be placed
struct LaneState {
    bool busy = false;            // the last ticket placed on it has not been waited for
    long long last_ticket = -1;   // that ticket (-1: the lane never ran one)
};

// The lane of the next ticket: an idle lane if there is one (lane 0 first), else the lane whose last ticket is older (it
// finishes first: tickets of one lane run in order).  second_ok: lane 1 exists or may be allocated now (second_lane_wanted and
// second_lane_fits); without it everything runs on lane 0, as before lanes existed.
inline int pick_lane(const LaneState ln[kMaxLanes], bool second_ok) {
    if (!second_ok || !ln[0].busy) return 0;
    if (!ln[1].busy) return 1;
    return ln[1].last_ticket < ln[0].last_ticket ? 1 : 0;
}

// May this model use a second lane?  lanes: the tuning knob (1 | 2).  conv_flops: conv FLOPs of one replay at max_batch;
// gate_flops: graphs above it stay on one lane (their kernels fill the chip alone and only pay for sharing it), <= 0: no gate.
inline bool second_lane_wanted(int lanes, double conv_flops, double gate_flops) {
    if (lanes < 2) return false;
    return gate_flops <= 0 || conv_flops <= gate_flops;
}

// The second lane is allocated only if it fits and leaves at least one more arena's worth of memory free (frame buffers,
// the other models' plans and the render path allocate after the first submit).
inline bool second_lane_fits(size_t free_bytes, size_t lane_bytes, size_t arena_bytes) {
    return free_bytes >= lane_bytes && free_bytes - lane_bytes >= arena_bytes;
}

}  // namespace padel
