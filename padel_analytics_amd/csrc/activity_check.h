// Host-only half of the frame statistics (activity_check.cpp): the refusals of pa_frame_activity and how a launch is cut into bands.
#pragma once
#include <cstdint>
#include <string>

namespace padel {

constexpr int kActivityMaxSide = 16384, kActivityMaxFrames = 65535;
// pixels of the roi one workgroup takes at most (whole rows; a row longer than this is a band of its own): 255 * 16384 < 2^23, so a
// workgroup's 32-bit partial sums cannot wrap
constexpr int kActivityBandPixels = 16384;

// every refusal of pa_frame_activity that needs no pointer but roi's.  0, or 1 with the reason in err
int activity_validate(int n, int h, int w, const int32_t* roi, int tau, std::string& err);
// rows of the roi per workgroup for a roi of roi_w x roi_h pixels (>= 1), and the bands that makes
int activity_band_rows(int roi_w, int roi_h);
inline int activity_bands(int roi_h, int band_rows) { return (roi_h + band_rows - 1) / band_rows; }

}  // namespace padel
