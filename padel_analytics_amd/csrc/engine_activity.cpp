// pa_frame_activity: frame statistics of BGR frames in HBM against a reference image and the previous frame (frame_activity.hip);
// pa_frames_median: the median kernel of the ball session without one; pa_box_histograms: colour histograms of rectangles of such
// frames (box_histogram.hip).  What is refused is host-only code in activity_check.cpp and box_histogram_check.cpp.
#include "engine_internal.h"
#include "activity_check.h"
#include "box_histogram_check.h"

int pa_frame_activity(pa_engine* e, const uint8_t* frames, int n, int h, int w, const uint8_t* ref, const uint8_t* prev, const int32_t* roi,
                      int tau, uint64_t* out) {
    if (!e) return 1;
    if (!frames || !ref || !out) PA_FAIL(e, "pa_frame_activity: frames, ref or out is NULL");
    std::string why;
    if (activity_validate(n, h, w, roi, tau, why)) PA_FAIL(e, "%s", why.c_str());
    PA_HIP(e, hipSetDevice(e->dev));
    ActivityArgs a{};
    a.frames = frames; a.ref = ref; a.prev = prev; a.n = n; a.h = h; a.w = w; a.tau = tau;
    a.x0 = roi ? roi[0] : 0; a.y0 = roi ? roi[1] : 0; a.x1 = roi ? roi[2] : w; a.y1 = roi ? roi[3] : h;
    a.band_rows = activity_band_rows(a.x1 - a.x0, a.y1 - a.y0);
    a.bands = activity_bands(a.y1 - a.y0, a.band_rows);
    // [n x 3 uint64 results | n x bands x 3 uint32 partial sums] in one engine-owned block; the call is synchronous, so a block
    // about to be replaced is idle
    const size_t out_bytes = (size_t)n * 3 * sizeof(uint64_t), bytes = out_bytes + (size_t)n * a.bands * 3 * sizeof(uint32_t);
    PA_HIP(e, e->activity_stage.fit(bytes, std::max(bytes * 2, (size_t)65536)));
    a.out = reinterpret_cast<unsigned long long*>(e->activity_stage.get());
    a.slab = reinterpret_cast<uint32_t*>(e->activity_stage.get() + out_bytes);
    hipStream_t s = e->main_stream();
    hipError_t r = launch_frame_activity(a, s);
    if (r != hipSuccess) PA_FAIL(e, "frame activity launch failed: %s", hipGetErrorString(r));
    PA_HIP(e, hipMemcpyAsync(out, a.out, out_bytes, hipMemcpyDeviceToHost, s));
    PA_HIP(e, hipStreamSynchronize(s));
    return 0;
}

int pa_frames_median(pa_engine* e, const uint8_t* frames, int n, int h, int w, uint8_t* out) {
    if (!e) return 1;
    if (!frames || !out) PA_FAIL(e, "pa_frames_median: frames or out is NULL");
    if (n < 1 || n > kActivityMaxFrames) PA_FAIL(e, "pa_frames_median: n = %d frames outside [1, %d]", n, kActivityMaxFrames);
    if (w < 1 || h < 1 || w > kActivityMaxSide || h > kActivityMaxSide)
        PA_FAIL(e, "pa_frames_median: %d x %d frames: width and height must lie in [1, %d]", w, h, kActivityMaxSide);
    const long long fb = (long long)h * w * 3;
    if (out < frames + (long long)n * fb && frames < out + fb) PA_FAIL(e, "pa_frames_median: out overlaps the frames");
    PA_HIP(e, hipSetDevice(e->dev));
    hipStream_t s = e->main_stream();
    const hipError_t r = launch_median(frames, n, fb, out, s, /*keep_bgr=*/true);
    if (r != hipSuccess) PA_FAIL(e, "median launch failed: %s", hipGetErrorString(r));
    PA_HIP(e, hipStreamSynchronize(s));
    return 0;
}

int pa_box_histograms(pa_engine* e, const uint8_t* frames, int n, int h, int w, const int32_t* rects, int k, uint32_t* out) {
    if (!e) return 1;
    if (!frames || !out) PA_FAIL(e, "%s", kBoxHistNull);
    std::string why;
    if (box_hist_validate(n, h, w, rects, k, why)) PA_FAIL(e, "%s", why.c_str());
    if (k == 0) return 0;
    PA_HIP(e, hipSetDevice(e->dev));
    // [k x 512 uint32 results | k x 5 int32 rectangles] in one engine-owned block; the call is synchronous, so a block about to be
    // replaced is idle.  The list is pageable memory: the runtime has consumed it when hipMemcpyAsync returns
    const size_t out_bytes = (size_t)k * kBoxHistBins * sizeof(uint32_t), rect_bytes = (size_t)k * 5 * sizeof(int32_t);
    PA_HIP(e, e->box_stage.fit(out_bytes + rect_bytes, std::max((out_bytes + rect_bytes) * 2, (size_t)65536)));
    BoxHistArgs a{};
    a.frames = frames; a.h = h; a.w = w; a.k = k;
    a.out = reinterpret_cast<uint32_t*>(e->box_stage.get());
    int32_t* const d_rects = reinterpret_cast<int32_t*>(e->box_stage.get() + out_bytes);
    a.rects = d_rects;
    hipStream_t s = e->main_stream();
    PA_HIP(e, hipMemcpyAsync(d_rects, rects, rect_bytes, hipMemcpyHostToDevice, s));
    hipError_t r = launch_box_histograms(a, s);
    if (r != hipSuccess) PA_FAIL(e, "box histogram launch failed: %s", hipGetErrorString(r));
    PA_HIP(e, hipMemcpyAsync(out, a.out, out_bytes, hipMemcpyDeviceToHost, s));
    PA_HIP(e, hipStreamSynchronize(s));
    return 0;
}
