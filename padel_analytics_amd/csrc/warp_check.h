// Host-only half of pa_warp_perspective (warp_check.cpp): what the call refuses.
#pragma once
#include "../../include/padel_hip.h"

#include <string>

namespace padel {

// every refusal of pa_warp_perspective.  src, dst: the addresses alone are looked at (NULL, overlap), nothing is read through them
int warp_validate(int n, int h, int w, int oh, int ow, const double* m, const int32_t* valid, const void* src, const void* dst,
                  std::string& err);

}  // namespace padel
