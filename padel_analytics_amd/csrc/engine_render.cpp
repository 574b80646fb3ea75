// pa_render / pa_render_scaled: marks on BGR frames in HBM -> BGR or YUV 4:2:0, at the source's size or at 1/2, 1/3, 1/4 of it
// (render.hip).  What is refused, and the font, are host-only code in render_check.cpp.
#include "engine_internal.h"
#include "render_check.h"

// pa_render (scale 1) and pa_render_scaled: one body, the launch apart
static int render_run(pa_engine* e, const uint8_t* src, int n, int h, int w, const pa_mark* marks, const int32_t* first, int scale, int out,
                      const pa_yuv_desc* geom, const pa_yuv_enc* enc, uint8_t* dst) {
    if (!e) return 1;
    if (!src || !dst) PA_FAIL(e, "pa_render: src or dst is NULL");
    size_t span = 0;
    std::string why;
    if (render_scaled_validate(n, h, w, marks, first, scale, out, geom, enc, dst == src ? 1 : 0, &span, why)) PA_FAIL(e, "%s", why.c_str());
    const size_t src_bytes = (size_t)n * h * w * 3;
    const bool same = dst == src;
    if (!(same && out == PA_RENDER_BGR) && src < dst + span && dst < src + src_bytes)
        PA_FAIL(e, "pa_render: dst overlaps src (only BGR output with dst == src renders in place)");
    PA_HIP(e, hipSetDevice(e->dev));
    // staging: [resolved marks | their boxes, 4 x int16 each | first[n + 1]] in one host block, one copy on the compute stream.  The
    // block is pageable memory: the runtime has consumed it when hipMemcpyAsync returns
    const size_t total = (size_t)first[n];
    const size_t box_off = total * sizeof(pa_mark), first_off = box_off + total * 8, bytes = first_off + (size_t)(n + 1) * sizeof(int32_t);
    std::vector<pa_mark> host((bytes + sizeof(pa_mark) - 1) / sizeof(pa_mark));
    render_resolve_marks(marks, host.data(), total);
    int16_t* hb = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(host.data()) + box_off);
    for (size_t k = 0; k < total; ++k) {                         // (coordinates within +-8192 and sizes up to 255: every edge fits int16)
        const MarkBox b = mark_bbox(host[k]);
        hb[4 * k] = (int16_t)b.x0; hb[4 * k + 1] = (int16_t)b.y0; hb[4 * k + 2] = (int16_t)b.x1; hb[4 * k + 3] = (int16_t)b.y1;
    }
    memcpy(reinterpret_cast<char*>(host.data()) + first_off, first, (size_t)(n + 1) * sizeof(int32_t));
    if (e->render_stage.bytes() < bytes) {
        PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));              // a render still queued reads the buffer about to go
        PA_HIP(e, e->render_stage.fit(bytes, std::max(bytes * 2, (size_t)65536)));
    }
    uint8_t* const stage = e->render_stage.get();
    PA_HIP(e, hipMemcpyAsync(stage, host.data(), bytes, hipMemcpyHostToDevice, e->main_stream()));
    RenderArgs a{};
    a.src = src; a.dst = dst; a.marks = stage; a.boxes = stage + box_off;
    a.first = reinterpret_cast<const int32_t*>(stage + first_off);
    a.n = n; a.h = h; a.w = w; a.in_place = same ? 1 : 0;
    if (out == PA_RENDER_YUV420) {
        a.out = geom->layout == PA_YUV_NV12 ? 1 : 2;
        a.pitch_y = geom->pitch_y; a.pitch_c = geom->pitch_c; a.off_u = geom->off_u; a.off_v = geom->off_v; a.frame_stride = geom->frame_stride;
        a.y_off = enc->y_off; a.yr = enc->yr; a.yg = enc->yg; a.yb = enc->yb;
        a.ur = enc->ur; a.ug = enc->ug; a.ub = enc->ub; a.vr = enc->vr; a.vg = enc->vg; a.vb = enc->vb;
    }
#ifdef PADEL_RENDER_PROBE
    static unsigned long long* d_probe = nullptr;                // tools build only (build.sh, PADEL_EXTRA_FLAGS): see the report below
    if (!d_probe) PA_HIP(e, hipMalloc((void**)&d_probe, 4 * sizeof(unsigned long long)));
    PA_HIP(e, hipMemsetAsync(d_probe, 0, 4 * sizeof(unsigned long long), e->main_stream()));
    a.probe = d_probe;
#endif
    int vec = 0;
    const hipError_t r = scale == 1 ? launch_render(a, e->main_stream(), &vec) : launch_render_scaled(a, scale, e->main_stream(), &vec);
    if (r != hipSuccess) PA_FAIL(e, "render launch failed: %s", hipGetErrorString(r));
#ifdef PADEL_RENDER_PROBE
    unsigned long long p[4] = {};
    PA_HIP(e, hipMemcpyAsync(p, d_probe, sizeof(p), hipMemcpyDeviceToHost, e->main_stream()));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    if (p[3]) fprintf(stderr, "render probe: %llu marks, %llu workgroups, shader-clock cycles per workgroup up to its stores %.0f, of which cull %.0f, apply %.0f\n",
                      (unsigned long long)total, p[3], (double)p[2] / p[3], (double)p[0] / p[3], (double)p[1] / p[3]);
#endif
    e->render_last_path = vec ? 1 : 2;
    return 0;
}

int pa_render(pa_engine* e, const uint8_t* src, int n, int h, int w, const pa_mark* marks, const int32_t* first, int out,
              const pa_yuv_desc* geom, const pa_yuv_enc* enc, uint8_t* dst) {
    return render_run(e, src, n, h, w, marks, first, 1, out, geom, enc, dst);
}

int pa_render_scaled(pa_engine* e, const uint8_t* src, int n, int h, int w, const pa_mark* marks, const int32_t* first, int scale, int out,
                     const pa_yuv_desc* geom, const pa_yuv_enc* enc, uint8_t* dst) {
    return render_run(e, src, n, h, w, marks, first, scale, out, geom, enc, dst);
}

int pa_render_last_path(pa_engine* e) { return e ? e->render_last_path : 0; }
