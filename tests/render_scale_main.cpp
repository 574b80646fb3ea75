// Stand-alone program over csrc/render_scale.h (g++, no HIP): for scale s = 2, 3, 4 prints one line "s sum quotient" for every sum
// of s x s channel values (0 .. 255 s^2), the quotient being what pa_render_scaled stores (scale_round).
// tests/test_render_scale_host.py compares the lines with the plain integer division.
#include <cstdio>

#include "render_scale.h"

template <int S>
static void table() {
    for (unsigned sum = 0; sum <= 255u * S * S; ++sum) printf("%d %u %u\n", S, sum, padel::scale_round<S>(sum));
}

int main() {
    table<2>();
    table<3>();
    table<4>();
    return 0;
}
