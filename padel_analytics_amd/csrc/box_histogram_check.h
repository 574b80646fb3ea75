// Host-only half of the box histograms (box_histogram_check.cpp): the refusals of pa_box_histograms.
#pragma once
#include <cstdint>
#include <string>

namespace padel {

constexpr int kBoxHistBins = 512;
// rectangles of one call at most: their rows of 512 counters then take 32 MiB of the engine's staging buffer
constexpr int kBoxHistMaxRects = 16384;
// what pa_box_histograms and the check say about a NULL pointer
constexpr const char* kBoxHistNull = "pa_box_histograms: frames, rects or out is NULL";

// every refusal of pa_box_histograms that needs no pointer but rects (k x 5: frame, x0, y0, x1, y1).  0, or 1 with the reason in err
int box_hist_validate(int n, int h, int w, const int32_t* rects, int k, std::string& err);

}  // namespace padel
