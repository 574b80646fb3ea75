// pa_warp_perspective: packed BGR frames in HBM through one 3 x 3 matrix each -> packed BGR frames of another size (warp.hip).
// What is refused is host-only code in warp_check.cpp.
#include "engine_internal.h"
#include "warp_check.h"

int pa_warp_perspective(pa_engine* e, const uint8_t* src, int n, int h, int w, const double* m, const int32_t* valid, uint32_t fill,
                        uint8_t* dst, int oh, int ow) {
    if (!e) return 1;
    std::string why;
    if (warp_validate(n, h, w, oh, ow, m, valid, src, dst, why)) PA_FAIL(e, "%s", why.c_str());
    PA_HIP(e, hipSetDevice(e->dev));
    // staging: [n x 9 doubles | n valid words] in one host block, one copy on the compute stream.  The block is pageable memory:
    // the runtime has consumed it when hipMemcpyAsync returns
    const size_t valid_off = (size_t)n * 9 * sizeof(double), bytes = valid_off + (size_t)n * sizeof(int32_t);
    std::vector<double> host((bytes + sizeof(double) - 1) / sizeof(double));
    memcpy(host.data(), m, valid_off);
    memcpy(reinterpret_cast<char*>(host.data()) + valid_off, valid, (size_t)n * sizeof(int32_t));
    if (e->warp_stage.bytes() < bytes) {
        PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));              // a warp still queued reads the buffer about to go
        PA_HIP(e, e->warp_stage.fit(bytes, std::max(bytes * 2, (size_t)4096)));
    }
    uint8_t* const stage = e->warp_stage.get();
    PA_HIP(e, hipMemcpyAsync(stage, host.data(), bytes, hipMemcpyHostToDevice, e->main_stream()));
    WarpArgs a{};
    a.src = src; a.dst = dst;
    a.m = reinterpret_cast<const double*>(stage);
    a.valid = reinterpret_cast<const int32_t*>(stage + valid_off);
    a.n = n; a.h = h; a.w = w; a.oh = oh; a.ow = ow; a.fill = fill & 0xffffffu;
    int vec = 0;
    const hipError_t r = launch_warp(a, e->main_stream(), &vec);
    if (r != hipSuccess) PA_FAIL(e, "warp launch failed: %s", hipGetErrorString(r));
    e->warp_last_path = vec ? 1 : 2;
    return 0;
}

int pa_warp_last_path(pa_engine* e) { return e ? e->warp_last_path : 0; }
