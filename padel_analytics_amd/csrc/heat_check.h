// Host-only half of pa_heat_accumulate (heat_check.cpp): what the call refuses.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

namespace padel {

// every refusal of pa_heat_accumulate.  canvas, state: the addresses alone are looked at (NULL, overlap), nothing is read through them;
// pts may be NULL when first[] announces no point
int heat_validate(int n, int oh, int ow, int planes, const int32_t* pts, const int32_t* first, const int32_t* valid, int r, uint32_t full,
                  int alpha, int show_mask, const uint8_t* lut, const void* canvas, const void* state, std::string& err);

}  // namespace padel
