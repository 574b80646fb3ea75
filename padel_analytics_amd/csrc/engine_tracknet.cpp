// Generic op-list graphs run through pa_tracknet_infer (TrackNet, InpaintNet, conv unit tests) and the ball session.
#include "engine_internal.h"

// (re)plan a generic graph when the network input size or the batch changed
static int ensure_tracknet_plan(pa_model* m, int h, int w) {
    pa_engine* e = m->e;
    if (m->planned && m->net_h == h && m->net_w == w && m->p_batch == m->max_batch) return 0;
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    free_plan(m);
    m->net_h = h; m->net_w = w;
    if (plan_buffers(m, m->ln[0], m->max_batch, e->main_stream())) return 1;
    m->planned = true;
    return 0;
}

int pa_tracknet_infer(pa_model* m, const float* x, int n, int h, int w, int x_on_device, float* out, int out_on_device) {
    if (!m) return 1;
    pa_engine* e = m->e;
    if (m->d.task != PA_TASK_TRACKNET) PA_FAIL(e, "pa_tracknet_infer on a non-TrackNet model");
    if (!x || !out || n <= 0) PA_FAIL(e, "pa_tracknet_infer: bad arguments");
    PA_HIP(e, hipSetDevice(e->dev));
    m->ovf_cached = false;               // this call's kernels may raise the flag: the host copy is stale
    if (ensure_tracknet_plan(m, h, w)) return 1;
    hipStream_t s = e->main_stream();
    const int cin = m->bufs[0].channels;
    const int ob = m->d.head_buf[0];
    const int cout = m->bufs[ob].channels;
    const size_t es_in = m->d.dtype == PA_DTYPE_F16 ? 2 : 4;     // fp16 graphs take their input as halves
    const bool h2 = m->d.dtype == PA_DTYPE_H2;                  // h2 graphs take fp32 and encode it on the device
    if (h2 && (cin & 15)) PA_FAIL(e, "pa_tracknet_infer: h2 input buffer has %d channels", cin);
    size_t pi = 0;
    for (int c0 = 0; c0 < n; c0 += m->max_batch) {
        const int nb = std::min(m->max_batch, n - c0);
        const size_t in_bytes = (size_t)nb * h * w * cin * es_in;
        const char* xs = reinterpret_cast<const char*>(x) + (size_t)c0 * h * w * cin * es_in;
        if (h2) {
            const float* src = reinterpret_cast<const float*>(xs);
            if (!x_on_device) {
                PA_HIP(e, m->ln[0].d_stage.fit(in_bytes, (size_t)m->max_batch * h * w * cin * 4));
                PA_HIP(e, hipMemcpyAsync(m->ln[0].d_stage.get(), xs, in_bytes, hipMemcpyHostToDevice, s));
                src = m->ln[0].d_stage.get();
            }
            const hipError_t er = launch_h2_encode(src, m->ln[0].bptr[0], (long long)(in_bytes / 4), m->d_ovf.get(), s);
            if (er != hipSuccess) PA_FAIL(e, "h2 encode launch failed: %s", hipGetErrorString(er));
        } else
        PA_HIP(e, hipMemcpyAsync(m->ln[0].bptr[0], xs, in_bytes,
                                 x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        if (run_graph(m, m->ln[0], s, nb, &pi, false)) return 1;
        const size_t ohw = (size_t)(h >> m->bufs[ob].level) * (w >> m->bufs[ob].level);
        const size_t out_bytes = (size_t)nb * ohw * cout * sizeof(float);
        PA_HIP(e, hipMemcpyAsync(out + (size_t)c0 * ohw * cout, m->ln[0].bptr[ob], out_bytes,
                                 out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        PA_HIP(e, hipStreamSynchronize(s));
    }
    finish_profile(m, pi);
    return 0;
}

// ------------------------------------------------------------------------------- ball session
struct pa_ball {
    pa_model* m = nullptr;
    int h = 0, w = 0;            // source frame size
    int B = 0;                   // max frames per feed == model max_batch
    int ring = 0;                // resized-frame ring slots (B + 7)
    long long fed = 0;           // frames fed since the last set_background
    bool have_bg = false;
    DevMem<uint8_t> d_src, d_small, d_med_src, d_med, d_mask; DevMem<float> d_heat;
    DevMem<float> d_Y;           // [7 + B + 7][288][512][cs] window outputs (7 carry rows first)
    DevMem<float> d_lut;
    ResamplePlan rs;             // Pillow bicubic, source size -> 288 x 512
    DevMem<int32_t> d_row0, d_mode; DevMem<float> d_div;
    DevMem<int32_t> d_label, d_bbox, d_rect;
    int cs = 0;
};

static const int BALL_H = 288, BALL_W = 512;

void pa_ball_destroy(pa_ball* b);

int pa_ball_create(pa_model* m, int src_h, int src_w, pa_ball** out) {
    if (!m || !out) return 1;
    pa_engine* e = m->e;
    if (m->d.task != PA_TASK_TRACKNET) PA_FAIL(e, "pa_ball_create: not a TrackNet model");
    if (m->bufs[0].channels != 32) PA_FAIL(e, "pa_ball_create: TrackNet input buffer must have 32 channels (27 + pad)");
    PA_HIP(e, hipSetDevice(e->dev));
    if (src_h <= 0 || src_w <= 0) PA_FAIL(e, "pa_ball_create: unsupported source size %dx%d", src_w, src_h);
    if (m->bufs[m->d.head_buf[0]].channels < 8)
        PA_FAIL(e, "pa_ball_create: TrackNet output has %d channels (< 8)", m->bufs[m->d.head_buf[0]].channels);
    std::unique_ptr<pa_ball, void (*)(pa_ball*)> owner(new pa_ball(), pa_ball_destroy);      // a failure below: wait, then release
    pa_ball* b = owner.get();
    b->m = m; b->h = src_h; b->w = src_w; b->B = m->max_batch; b->ring = b->B + 7;
    b->cs = m->bufs[m->d.head_buf[0]].channels;
    const size_t HW = (size_t)BALL_H * BALL_W;
    PA_HIP(e, b->d_src.alloc((size_t)b->B * src_h * src_w * 3));
    PA_HIP(e, b->d_small.alloc((size_t)b->ring * HW * 3));
    PA_HIP(e, b->d_med_src.alloc((size_t)src_h * src_w * 3));
    PA_HIP(e, b->d_med.alloc(HW * 3));
    PA_HIP(e, b->d_mask.alloc((size_t)(b->B + 7) * HW));
    PA_HIP(e, b->d_heat.alloc((size_t)(b->B + 7) * HW * sizeof(float)));
    PA_HIP(e, b->d_Y.alloc((size_t)(b->B + 14) * HW * b->cs * sizeof(float)));
    PA_HIP(e, b->d_row0.alloc((b->B + 7) * sizeof(int32_t)));
    PA_HIP(e, b->d_mode.alloc((b->B + 7) * sizeof(int32_t)));
    PA_HIP(e, b->d_div.alloc((b->B + 7) * sizeof(float)));
    PA_HIP(e, b->d_label.alloc((size_t)(b->B + 7) * HW * sizeof(int32_t)));
    PA_HIP(e, b->d_bbox.alloc((size_t)(b->B + 7) * 4 * HW * sizeof(int32_t)));
    PA_HIP(e, b->d_rect.alloc((size_t)(b->B + 7) * 4 * sizeof(int32_t)));
    std::vector<float> lut(256);
    for (int i = 0; i < 256; ++i) lut[i] = (float)((double)i / 255.0);     // float64 division, then .float()
    PA_HIP(e, b->d_lut.alloc(256 * sizeof(float)));
    PA_HIP(e, hipMemcpyAsync(b->d_lut.get(), lut.data(), 256 * sizeof(float), hipMemcpyHostToDevice, e->main_stream()));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    if (resample_plan(e, &b->rs, src_h, src_w, BALL_H, BALL_W, PIL_BICUBIC, b->B, true)) return 1;
    *out = owner.release();
    return 0;
}

void pa_ball_destroy(pa_ball* b) {
    if (!b) return;
    hipSetDevice(b->m->e->dev);
    hipStreamSynchronize(b->m->e->main_stream_wait_only());
    delete b;
}

// Pillow bicubic resize of n u8 HWC images (h x w x 3) to 288 x 512 x 3, optional channel reversal
static int ball_resize(pa_ball* b, const uint8_t* src, int n, uint8_t* dst, int reverse) {
    pa_engine* e = b->m->e;
    const hipError_t r = resample_enqueue(b->rs, src, dst, n, 3, reverse, e->main_stream());
    if (r != hipSuccess) PA_FAIL(e, "ball resize launch failed: %s", hipGetErrorString(r));
    return 0;
}

static int ball_finish_background(pa_ball* b);

int pa_ball_set_background(pa_ball* b, const uint8_t* median_rgb) {
    if (!b || !median_rgb) return 1;
    pa_engine* e = b->m->e;
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipMemcpyAsync(b->d_med_src.get(), median_rgb, (size_t)b->h * b->w * 3, hipMemcpyHostToDevice, e->main_stream()));
    return ball_finish_background(b);
}

static int ball_finish_background(pa_ball* b) {
    pa_engine* e = b->m->e;
    if (ball_resize(b, b->d_med_src.get(), 1, b->d_med.get(), 0)) return 1;
    PA_HIP(e, hipMemsetAsync(b->d_Y.get(), 0, (size_t)(b->B + 14) * BALL_H * BALL_W * b->cs * sizeof(float), e->main_stream()));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    b->fed = 0;
    b->have_bg = true;
    return 0;
}

int pa_ball_background_from_frames(pa_ball* b, const uint8_t* frames_bgr, int n, int on_device, uint8_t* out_median_rgb) {
    if (!b || !frames_bgr) return 1;
    pa_engine* e = b->m->e;
    if (n < 1 || n > 65535) PA_FAIL(e, "pa_ball_background_from_frames: n = %d", n);
    PA_HIP(e, hipSetDevice(e->dev));
    hipStream_t s = e->main_stream();
    const long long fb = (long long)b->h * b->w * 3;
    const uint8_t* src = frames_bgr;
    DevMem<uint8_t> tmp;         // host frames: their copy on the device, for this call
    if (!on_device) {
        PA_HIP(e, tmp.alloc((size_t)n * fb));
        hipError_t r = hipMemcpyAsync(tmp.get(), frames_bgr, (size_t)n * fb, hipMemcpyHostToDevice, s);
        if (r != hipSuccess) PA_FAIL(e, "median upload: %s", hipGetErrorString(r));
        src = tmp.get();
    }
    hipError_t r = launch_median(src, n, fb, b->d_med_src.get(), s);
    if (r == hipSuccess && out_median_rgb) r = hipMemcpyAsync(out_median_rgb, b->d_med_src.get(), (size_t)fb, hipMemcpyDeviceToHost, s);
    if (r == hipSuccess) r = hipStreamSynchronize(s);
    tmp.reset();
    if (r != hipSuccess) PA_FAIL(e, "median kernel: %s", hipGetErrorString(r));
    return ball_finish_background(b);
}

int pa_ball_feed(pa_ball* b, const uint8_t* frames, int n, int on_device, int flush, uint8_t* out_masks,
                 float* out_heat, int32_t* out_rects, int* out_count) {
    if (!b || (!out_masks && !out_rects) || !out_count) return 1;
    pa_model* m = b->m;
    pa_engine* e = m->e;
    if (!b->have_bg) PA_FAIL(e, "pa_ball_feed: set the background first");
    if (b->B != m->max_batch)
        PA_FAIL(e, "pa_ball_feed: the model's max_batch changed (%d -> %d) after the session was created; create a new session",
                b->B, m->max_batch);
    if (n < 0 || n > b->B || (n > 0 && !frames)) PA_FAIL(e, "pa_ball_feed: n = %d (max %d)", n, b->B);
    PA_HIP(e, hipSetDevice(e->dev));
    m->ovf_cached = false;               // this call's kernels may raise the flag: the host copy is stale
    hipStream_t s = e->main_stream();
    const size_t HW = (size_t)BALL_H * BALL_W;
    if (ensure_tracknet_plan(m, BALL_H, BALL_W)) return 1;
    int nout = 0;
    std::vector<int32_t> row0, mode;
    std::vector<float> div;
    int nw = 0;
    size_t prof_n = 0;
    if (n > 0) {
        // 1. resize the new frames (BGR -> RGB) into the ring; a feed never wraps more than once
        const uint8_t* src = frames;
        if (!on_device) {
            PA_HIP(e, hipMemcpyAsync(b->d_src.get(), frames, (size_t)n * b->h * b->w * 3, hipMemcpyHostToDevice, s));
            src = b->d_src.get();
        }
        const int slot0 = (int)(b->fed % b->ring);
        const int first = std::min(n, b->ring - slot0);
        if (ball_resize(b, src, first, b->d_small.get() + (size_t)slot0 * HW * 3, 1)) return 1;
        if (first < n && ball_resize(b, src + (size_t)first * b->h * b->w * 3, n - first, b->d_small.get(), 1)) return 1;
        const long long f_old = b->fed, f_new = b->fed + n;
        // 2. new complete windows g in [g_lo, g_hi]
        const long long g_lo = std::max(0ll, f_old - 7), g_hi = f_new - 8;
        nw = g_hi >= g_lo ? (int)(g_hi - g_lo + 1) : 0;
        if (nw > 0) {
            BallAssembleArgs aa{};
            aa.median = b->d_med.get(); aa.frames = b->d_small.get(); aa.lut = b->d_lut.get(); aa.out = m->ln[0].bptr[0];
            aa.B = nw; aa.H = BALL_H; aa.W = BALL_W; aa.ring = b->ring; aa.first_slot = (int)(g_lo % b->ring);
            aa.out_f16 = m->d.dtype == PA_DTYPE_F16 ? 1 : m->d.dtype == PA_DTYPE_H2 ? 2 : 0;
            hipError_t r = launch_ball_assemble(aa, s);
            if (r != hipSuccess) PA_FAIL(e, "ball assemble launch failed: %s", hipGetErrorString(r));
            if (run_graph(m, m->ln[0], s, nw, &prof_n, false)) return 1;
            PA_HIP(e, hipMemcpyAsync(b->d_Y.get() + (size_t)7 * HW * b->cs, m->ln[0].bptr[m->d.head_buf[0]],
                                     (size_t)nw * HW * b->cs * sizeof(float), hipMemcpyDeviceToDevice, s));
            for (int i = 0; i < nw; ++i) {             // frame g = g_lo + i: rows i .. i+7 (row r <-> window g_lo - 7 + r)
                const long long g = g_lo + i;
                row0.push_back(i);
                mode.push_back(g < 7 ? 1 : 0);
                div.push_back((float)(g + 1));
            }
        }
        b->fed = f_new;
    }
    if (flush && b->fed >= 8) {
        // tail: rows after the last window are zero (ball_tracker.py:486-509)
        PA_HIP(e, hipMemsetAsync(b->d_Y.get() + (size_t)(7 + nw) * HW * b->cs, 0, (size_t)7 * HW * b->cs * sizeof(float), s));
        for (int fi = 1; fi < 8; ++fi) {
            row0.push_back(nw - 1 + fi);               // window index of the last sample is row (nw - 1) + 7
            mode.push_back(1);
            div.push_back((float)(8 - fi));
        }
    }
    nout = (int)row0.size();
    if (nout > 0) {
        PA_HIP(e, hipMemcpyAsync(b->d_row0.get(), row0.data(), nout * sizeof(int32_t), hipMemcpyHostToDevice, s));
        PA_HIP(e, hipMemcpyAsync(b->d_mode.get(), mode.data(), nout * sizeof(int32_t), hipMemcpyHostToDevice, s));
        PA_HIP(e, hipMemcpyAsync(b->d_div.get(), div.data(), nout * sizeof(float), hipMemcpyHostToDevice, s));
        BallEnsembleArgs ea{};
        ea.Y = b->d_Y.get(); ea.cs = b->cs; ea.H = BALL_H; ea.W = BALL_W; ea.row0 = b->d_row0.get(); ea.mode = b->d_mode.get(); ea.div = b->d_div.get();
        static const float w8[8] = {1.f, 2.f, 3.f, 4.f, 4.f, 3.f, 2.f, 1.f};
        for (int k = 0; k < 8; ++k) ea.w[k] = w8[k] / 20.0f;
        ea.threshold = 0.5f; ea.heat = out_heat ? b->d_heat.get() : nullptr; ea.mask = b->d_mask.get();
        hipError_t r = launch_ball_ensemble(ea, nout, s);
        if (r != hipSuccess) PA_FAIL(e, "ball ensemble launch failed: %s", hipGetErrorString(r));
        if (out_rects) {
            BallLocateArgs la{};
            la.mask = b->d_mask.get(); la.label = b->d_label.get(); la.bbox = b->d_bbox.get(); la.rect = b->d_rect.get(); la.H = BALL_H; la.W = BALL_W;
            r = launch_ball_locate(la, nout, s);
            if (r != hipSuccess) PA_FAIL(e, "ball locate launch failed: %s", hipGetErrorString(r));
            PA_HIP(e, hipMemcpyAsync(out_rects, b->d_rect.get(), (size_t)nout * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        if (out_masks) PA_HIP(e, hipMemcpyAsync(out_masks, b->d_mask.get(), (size_t)nout * HW, hipMemcpyDeviceToHost, s));
        if (out_heat) PA_HIP(e, hipMemcpyAsync(out_heat, b->d_heat.get(), (size_t)nout * HW * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    // 3. carry the last 7 window rows to the front for the next feed: rows [nw, nw+7) -> [0, 7).  The ranges
    // overlap when nw < 7; copying row by row in ascending order is safe because dst row < src row.
    if (nw > 0) {
        for (int r7 = 0; r7 < 7; ++r7)
            PA_HIP(e, hipMemcpyAsync(b->d_Y.get() + (size_t)r7 * HW * b->cs, b->d_Y.get() + (size_t)(nw + r7) * HW * b->cs,
                                     HW * b->cs * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    PA_HIP(e, hipStreamSynchronize(s));
    finish_profile(m, prof_n);
    *out_count = nout;
    return 0;
}

int pa_ball_read_resized(pa_ball* b, long long frame, uint8_t* out) {
    if (!b || !out) return 1;
    pa_engine* e = b->m->e;
    if (!b->have_bg) PA_FAIL(e, "pa_ball_read_resized: no background set");
    if (frame >= b->fed || (frame >= 0 && frame + b->ring < b->fed))
        PA_FAIL(e, "pa_ball_read_resized: frame %lld is not among the last %d of %lld fed", frame, b->ring, b->fed);
    PA_HIP(e, hipSetDevice(e->dev));
    const size_t bytes = (size_t)BALL_H * BALL_W * 3;
    const uint8_t* src = frame < 0 ? b->d_med.get() : b->d_small.get() + (size_t)(frame % b->ring) * bytes;
    PA_HIP(e, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, e->main_stream()));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    return 0;
}

int pa_ball_locate(pa_ball* b, const uint8_t* masks, int n, int32_t* out_rects) {
    if (!b || !masks || !out_rects) return 1;
    pa_engine* e = b->m->e;
    if (n < 1 || n > b->B + 7) PA_FAIL(e, "pa_ball_locate: n = %d (max %d)", n, b->B + 7);
    PA_HIP(e, hipSetDevice(e->dev));
    hipStream_t s = e->main_stream();
    const size_t HW = (size_t)BALL_H * BALL_W;
    PA_HIP(e, hipMemcpyAsync(b->d_mask.get(), masks, (size_t)n * HW, hipMemcpyHostToDevice, s));
    BallLocateArgs la{};
    la.mask = b->d_mask.get(); la.label = b->d_label.get(); la.bbox = b->d_bbox.get(); la.rect = b->d_rect.get(); la.H = BALL_H; la.W = BALL_W;
    hipError_t r = launch_ball_locate(la, n, s);
    if (r != hipSuccess) PA_FAIL(e, "ball locate launch failed: %s", hipGetErrorString(r));
    PA_HIP(e, hipMemcpyAsync(out_rects, b->d_rect.get(), (size_t)n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PA_HIP(e, hipStreamSynchronize(s));
    return 0;
}
