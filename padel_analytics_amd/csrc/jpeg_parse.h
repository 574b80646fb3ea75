// Host-only half of the Motion-JPEG reader (jpeg_parse.cpp): the markers of one baseline JPEG -> its description (geometry,
// quantisers, Huffman tables) and its restart-interval table.  No HIP: built by g++ into the library (pa_jpeg_parse) and into
// tests/jpeg_decode_main.cpp's program.  What is accepted and refused is specified in include/padel_hip.h (pa_jpeg_decode).
#pragma once
#include "../../include/padel_hip.h"

#include <cstddef>
#include <string>
#include <vector>

namespace padel {

// 0: *info and ivls describe the frame; 1: refused, the reason in err
int jpeg_parse_frame(const uint8_t* p, size_t len, pa_jpeg_frame_info* info, std::vector<pa_jpeg_interval>& ivls, std::string& err);

}  // namespace padel
