#include "engine_internal.h"

// ---- court keypoints: the ResNet-50 regressor of trackers/keypoints_tracker (keypoints_tracker.py:264-312, iterable.py:10-39) ----
// transforms.Resize((224, 224)) on a PIL image is Image.resize(..., BILINEAR): the separable 22-bit fixed-point passes of the
// pose path with the triangle filter, horizontal first; ToTensor + Normalize happen inside the stem (its 3 x 256 table).
static const int RESNET_S = 224;

static int plan_resnet(pa_model* m, int h0, int w0) {
    pa_engine* e = m->e;
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    free_plan(m);
    const int S = RESNET_S;
    m->net_h = m->net_w = S;
    m->rw = m->rh = S; m->top = m->left = 0; m->lb_mode = 0;
    if (resample_plan(e, &m->rs, h0, w0, S, S, PIL_BILINEAR, m->max_batch)) return 1;
    PA_HIP(e, m->ln[0].d_netin.alloc((size_t)m->max_batch * S * S * 4));
    if (plan_buffers(m, m->ln[0], m->max_batch, e->main_stream())) return 1;
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    m->p_h0 = h0; m->p_w0 = w0; m->p_imgsz = S; m->p_pre = PA_PRE_PIL_STRETCH; m->p_auto = 0;
    m->planned = true;
    return 0;
}

int pa_resnet_infer(pa_model* m, const uint8_t* frames, int n, int h, int w, int frames_on_device, float* out_xy, float* out_logits) {
    if (!m) return 1;
    pa_engine* e = m->e;
    if (m->d.task != PA_TASK_RESNET) PA_FAIL(e, "pa_resnet_infer on a model of another task");
    if (!frames || n <= 0 || h <= 0 || w <= 0) PA_FAIL(e, "pa_resnet_infer: bad arguments");
    PA_HIP(e, hipSetDevice(e->dev));
    if (m->n_inflight) PA_FAIL(e, "pa_resnet_infer: tickets in flight");
    if (!m->planned || m->p_h0 != h || m->p_w0 != w || m->p_batch != m->max_batch)
        if (plan_resnet(m, h, w)) return 1;
    if (m->fc_nout && !out_xy) PA_FAIL(e, "pa_resnet_infer: out_xy is NULL");
    hipStream_t s = e->main_stream();
    const int S = RESNET_S;
    const size_t frame_bytes = (size_t)h * w * 3;
    m->ovf_cached = false;               // this call's kernels may raise the flag: the host copy is stale
    size_t pi = 0;
    for (int c0 = 0; c0 < n; c0 += m->max_batch) {
        const int nb = std::min(m->max_batch, n - c0);
        const uint8_t* src = frames + (size_t)c0 * frame_bytes;
        if (!frames_on_device && stage_frames(m, &src, nb, frame_bytes, s)) return 1;
        // ---- BGR frames -> RGB, Pillow bilinear to 224 x 224 (horizontal pass, then vertical), u8 NHWC4
        ProfRec* pr = prof_begin(m, s, pi++, PROF_PRE, 0, 0.0);
        hipError_t r = hipSuccess;
        if (h == S && w == S) {
            LetterboxArgs a{};
            a.src = src; a.dst = m->ln[0].d_netin.get(); a.B = nb; a.h0 = h; a.w0 = w; a.rw = S; a.rh = S; a.nh = S; a.nw = S; a.mode = 0; a.reverse = 1;
            r = launch_letterbox(a, s);
        } else {
            r = resample_enqueue(m->rs, src, m->ln[0].d_netin.get(), nb, 4, 1, s);
        }
        prof_end(s, pr);
        if (r != hipSuccess) PA_FAIL(e, "preprocess launch failed: %s", hipGetErrorString(r));
        if (run_graph(m, m->ln[0], s, nb, &pi, false)) return 1;
        if (m->fc_nout) {
            const size_t row = (size_t)m->fc_nout * sizeof(float);
            PA_HIP(e, hipMemcpyAsync(out_xy + (size_t)c0 * m->fc_nout, m->ln[0].d_fc.get() + (size_t)m->p_batch * kGapFcMaxOut, nb * row, hipMemcpyDeviceToHost, s));
            if (out_logits) PA_HIP(e, hipMemcpyAsync(out_logits + (size_t)c0 * m->fc_nout, m->ln[0].d_fc.get(), nb * row, hipMemcpyDeviceToHost, s));
        }
        PA_HIP(e, hipStreamSynchronize(s));
        m->last_n = nb;
    }
    finish_profile(m, pi);
    return 0;
}

int pa_resnet_read_netin(pa_model* m, int n, uint8_t* out) {
    if (!m) return 1;
    pa_engine* e = m->e;
    if (m->d.task != PA_TASK_RESNET || !m->planned || !m->ln[0].d_netin.get() || n < 1 || n > m->last_n || !out) PA_FAIL(e, "pa_resnet_read_netin: no plan / bad n");
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipMemcpyAsync(out, m->ln[0].d_netin.get(), (size_t)n * RESNET_S * RESNET_S * 4, hipMemcpyDeviceToHost, e->main_stream()));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    return 0;
}

int pa_resnet_read_fc(pa_model* m, int n, float* out_xy, float* out_logits) {
    if (!m) return 1;
    pa_engine* e = m->e;
    if (!m->planned || !m->fc_nout || !m->ln[0].d_fc.get() || n < 1 || n > m->p_batch) PA_FAIL(e, "pa_resnet_read_fc: no plan with a pooled linear head / bad n");
    PA_HIP(e, hipSetDevice(e->dev));
    const size_t bytes = (size_t)n * m->fc_nout * sizeof(float);
    if (out_xy) PA_HIP(e, hipMemcpyAsync(out_xy, m->ln[0].d_fc.get() + (size_t)m->p_batch * kGapFcMaxOut, bytes, hipMemcpyDeviceToHost, e->main_stream()));
    if (out_logits) PA_HIP(e, hipMemcpyAsync(out_logits, m->ln[0].d_fc.get(), bytes, hipMemcpyDeviceToHost, e->main_stream()));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    return 0;
}

int pa_resnet_read_head(pa_model* m, int n, float* out) {
    if (!m) return 1;
    pa_engine* e = m->e;
    const int b = m->d.head_buf[0];
    if (m->d.task != PA_TASK_RESNET || !m->planned || b < 0 || n < 1 || n > m->last_n || !out) PA_FAIL(e, "pa_resnet_read_head: no plan / no head buffer / bad n");
    PA_HIP(e, hipSetDevice(e->dev));
    const size_t hw = (size_t)(m->net_h >> m->bufs[b].level) * (m->net_w >> m->bufs[b].level);
    PA_HIP(e, hipMemcpyAsync(out, m->ln[0].bptr[b], (size_t)n * hw * m->bufs[b].channels * sizeof(float), hipMemcpyDeviceToHost, e->main_stream()));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    return 0;
}
