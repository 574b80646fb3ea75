// Preprocessing shared by the model families: staging host frames in HBM, the two-pass Pillow resample (tables, temporary,
// launches) and YUV 4:2:0 -> BGR.  The arithmetic of the tables is host-only code in graph_plan.cpp.
#include "engine_internal.h"

hipError_t upload_table(pa_engine* e, DevMem<int32_t>& d, const std::vector<int32_t>& v) {
    hipError_t r = (hipError_t)d.alloc(v.size() * sizeof(int32_t));
    if (r != hipSuccess) return r;
    r = hipMemcpyAsync(d.get(), v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->main_stream());
    if (r != hipSuccess) return r;
    return hipStreamSynchronize(e->main_stream_wait_only());
}

int stage_frames(pa_model* m, const uint8_t** src, int nb, size_t frame_bytes, hipStream_t s) {
    pa_engine* e = m->e;
    PA_HIP(e, m->d_frames.fit((size_t)nb * frame_bytes, (size_t)m->max_batch * frame_bytes));
    PA_HIP(e, hipMemcpyAsync(m->d_frames.get(), *src, (size_t)nb * frame_bytes, hipMemcpyHostToDevice, s));
    *src = m->d_frames.get();
    return 0;
}

int resample_plan(pa_engine* e, ResamplePlan* rs, int sh, int sw, int dh, int dw, int filter, int max_batch, bool identity_pass) {
    rs->sh = sh; rs->sw = sw; rs->dh = dh; rs->dw = dw;
    std::vector<int32_t> b, k;
    if (sw != dw) { rs->hks = pil_coeffs(sw, dw, b, k, filter); PA_HIP(e, upload_table(e, rs->d_hb, b)); PA_HIP(e, upload_table(e, rs->d_hk, k)); }
    if (sh != dh) { rs->vks = pil_coeffs(sh, dh, b, k, filter); PA_HIP(e, upload_table(e, rs->d_vb, b)); PA_HIP(e, upload_table(e, rs->d_vk, k)); }
    if (sw != dw && sh != dh) PA_HIP(e, rs->d_tmp.alloc((size_t)max_batch * sh * dw * 3));
    if (identity_pass && sh == dh && sw == dw) {
        // identity "resample": one tap of weight 1.0 (1 << 22) per output row
        rs->vks = 1;
        b.assign((size_t)dh * 2, 0);
        k.assign((size_t)dh, 1 << 22);
        for (int y = 0; y < dh; ++y) { b[2 * y] = y; b[2 * y + 1] = 1; }
        PA_HIP(e, upload_table(e, rs->d_vb, b)); PA_HIP(e, upload_table(e, rs->d_vk, k));
    }
    return 0;
}

hipError_t resample_enqueue(const ResamplePlan& rs, const uint8_t* src, uint8_t* dst, int n, int out_c, int reverse, hipStream_t s, uint8_t* tmp) {
    // a source of the target size has no pass to run unless the plan built the 1-tap one (the ball session's): the YOLO and ResNet
    // paths copy such frames with the letterbox kernel and never get here; launching nothing would leave dst as it was
    if (rs.sw == rs.dw && rs.sh == rs.dh && !rs.d_vb) return hipErrorInvalidValue;
    if (!tmp) tmp = rs.d_tmp.get();
    const uint8_t* cur = src;
    int cw = rs.sw;
    hipError_t r = hipSuccess;
    if (rs.sw != rs.dw) {
        ResamplePassArgs a{};
        const bool last = (rs.sh == rs.dh);
        a.in = cur; a.out = last ? dst : tmp; a.B = n; a.in_h = rs.sh; a.in_w = rs.sw; a.in_c = 3;
        a.out_h = rs.sh; a.out_w = rs.dw; a.out_c = last ? out_c : 3; a.vertical = 0; a.bounds = rs.d_hb.get(); a.coefs = rs.d_hk.get();
        a.ksize = rs.hks; a.reverse = last ? reverse : 0;
        r = launch_resample_pass(a, s);
        cur = tmp; cw = rs.dw;
    }
    // (a source that already has the target size runs the 1-tap pass where the plan built one: only the channel order
    // may change; the letterbox kernel in copy mode writes 4-byte pixels)
    if (r == hipSuccess && (rs.sh != rs.dh || (rs.sw == rs.dw && rs.d_vb))) {
        ResamplePassArgs a{};
        a.in = cur; a.out = dst; a.B = n; a.in_h = rs.sh; a.in_w = cw; a.in_c = 3;
        a.out_h = rs.dh; a.out_w = cw; a.out_c = out_c; a.vertical = 1; a.bounds = rs.d_vb.get(); a.coefs = rs.d_vk.get();
        a.ksize = rs.vks; a.reverse = reverse;
        r = launch_resample_pass(a, s);
    }
    return r;
}

// ------------------------------------------------------------------------------- YUV 4:2:0 -> BGR

int pa_yuv420_to_bgr(pa_engine* e, const uint8_t* src, int src_on_device, int n, int h, int w, const pa_yuv_desc* d, uint8_t* dst) {
    if (!e) return 1;
    if (!src || !dst) PA_FAIL(e, "pa_yuv420_to_bgr: src or dst is NULL");
    size_t span = 0;
    std::string why;
    if (yuv_validate(n, h, w, d, &span, why)) PA_FAIL(e, "%s", why.c_str());
    PA_HIP(e, hipSetDevice(e->dev));
    if (!src_on_device) {
        if (e->yuv_stage.bytes() < span) {
            PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));          // a conversion still queued reads the buffer about to go
            PA_HIP(e, e->yuv_stage.fit(span, span));
        }
        PA_HIP(e, hipMemcpyAsync(e->yuv_stage.get(), src, span, hipMemcpyHostToDevice, e->main_stream()));
        src = e->yuv_stage.get();
    }
    YuvArgs a{};
    a.src = src; a.dst = dst; a.n = n; a.h = h; a.w = w; a.nv12 = d->layout == PA_YUV_NV12;
    a.pitch_y = d->pitch_y; a.pitch_c = d->pitch_c; a.off_u = d->off_u; a.off_v = d->off_v; a.frame_stride = d->frame_stride;
    a.y_off = d->y_off; a.cy = d->cy; a.cvr = d->cvr; a.cug = d->cug; a.cvg = d->cvg; a.cub = d->cub;
    int vec = 0;
    const hipError_t r = launch_yuv420_to_bgr(a, e->main_stream(), &vec);
    if (r != hipSuccess) PA_FAIL(e, "yuv420_to_bgr launch failed: %s", hipGetErrorString(r));
    e->yuv_last_path = vec ? 1 : 2;
    return 0;
}

int pa_yuv_last_path(pa_engine* e) { return e ? e->yuv_last_path : 0; }

int pa_pil_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* coefs, int coefs_cap, int* ksize) {
    if (in_size < 1 || out_size < 1 || (filter != PIL_BICUBIC && filter != PIL_BILINEAR) || !ksize) return 1;
    std::vector<int32_t> b, k;
    *ksize = pil_coeffs(in_size, out_size, b, k, filter);
    if (!bounds || !coefs) return 0;                       // size query
    if ((size_t)coefs_cap < k.size()) return 1;
    memcpy(bounds, b.data(), b.size() * sizeof(int32_t));
    memcpy(coefs, k.data(), k.size() * sizeof(int32_t));
    return 0;
}
