// pa_heat_accumulate: the players' density maps, added to and blended into the top-down canvases in HBM, in place (heat.hip).
// What is refused is host-only code in heat_check.cpp.
#include "engine_internal.h"
#include "heat_check.h"
#include "heat_math.h"

int pa_heat_accumulate(pa_engine* e, uint8_t* canvas, int n, int oh, int ow, uint32_t* state, int planes, const int32_t* pts,
                       const int32_t* first, const int32_t* valid, int r, uint32_t full, int alpha, int show_mask, const uint8_t* lut) {
    if (!e) return 1;
    std::string why;
    if (heat_validate(n, oh, ow, planes, pts, first, valid, r, full, alpha, show_mask, lut, canvas, state, why)) PA_FAIL(e, "%s", why.c_str());
    PA_HIP(e, hipSetDevice(e->dev));
    // staging: [256 lut words | n + 1 first | n valid | n boxes of 4 | 3 words per point] in one host block, one copy on the compute
    // stream.  The block is pageable memory: the runtime has consumed it when hipMemcpyAsync returns
    const size_t total = (size_t)first[n];
    const size_t first_off = 256, valid_off = first_off + n + 1, box_off = valid_off + n, pts_off = box_off + 4 * (size_t)n;
    std::vector<int32_t> host(pts_off + 3 * total);
    for (int k = 0; k < 256; ++k) host[k] = (int32_t)((uint32_t)lut[3 * k] | (uint32_t)lut[3 * k + 1] << 8 | (uint32_t)lut[3 * k + 2] << 16);
    memcpy(&host[first_off], first, ((size_t)n + 1) * sizeof(int32_t));
    memcpy(&host[valid_off], valid, (size_t)n * sizeof(int32_t));
    for (int i = 0; i < n; ++i) {
        // the pixels frame i's discs can reach: a point (x, y) adds to |u - x| < r, |v - y| < r at most
        int32_t x0 = 1, y0 = 1, x1 = 0, y1 = 0;
        for (int k = first[i]; k < first[i + 1]; ++k) {
            const int32_t x = pts[3 * (size_t)k], y = pts[3 * (size_t)k + 1];
            if (x0 > x1) { x0 = x - r + 1; x1 = x + r - 1; y0 = y - r + 1; y1 = y + r - 1; }
            else { x0 = std::min(x0, x - r + 1); x1 = std::max(x1, x + r - 1); y0 = std::min(y0, y - r + 1); y1 = std::max(y1, y + r - 1); }
        }
        int32_t* const b = &host[box_off + 4 * (size_t)i];
        b[0] = x0; b[1] = y0; b[2] = x1; b[3] = y1;
    }
    if (total) memcpy(&host[pts_off], pts, 3 * total * sizeof(int32_t));
    const size_t bytes = host.size() * sizeof(int32_t);
    if (e->heat_stage.bytes() < bytes) {
        PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));              // a call still queued reads the buffer about to go
        PA_HIP(e, e->heat_stage.fit(bytes, std::max(bytes * 2, (size_t)4096)));
    }
    const int32_t* const stage = reinterpret_cast<const int32_t*>(e->heat_stage.get());
    PA_HIP(e, hipMemcpyAsync(e->heat_stage.get(), host.data(), bytes, hipMemcpyHostToDevice, e->main_stream()));
    HeatArgs a{};
    a.canvas = canvas; a.state = state;
    a.lut = reinterpret_cast<const uint32_t*>(stage);
    a.first = stage + first_off; a.valid = stage + valid_off; a.box = stage + box_off; a.pts = stage + pts_off;
    a.n = n; a.oh = oh; a.ow = ow; a.planes = planes; a.r = r; a.alpha = alpha; a.show_mask = show_mask; a.full = full;
    int vec = 0;
    const hipError_t rc = launch_heat(a, e->main_stream(), &vec);
    if (rc != hipSuccess) PA_FAIL(e, "heat launch failed: %s", hipGetErrorString(rc));
    e->heat_last_path = vec ? 1 : 2;
    return 0;
}

int pa_heat_last_path(pa_engine* e) { return e ? e->heat_last_path : 0; }
