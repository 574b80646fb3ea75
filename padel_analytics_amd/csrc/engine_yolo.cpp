// YOLO detect / pose: plan for a (source size, imgsz, preprocessing, batch), preprocessing, network, decode + NMS, tickets
// (pa_yolo_submit / pa_yolo_wait) and the read-backs of the tests.
#include "engine_internal.h"

// What one lane of a YOLO plan owns (struct Lane): network input, activation arena, head-level pointers, post-processing buffers
// and, on a second lane of a two-pass Pillow plan, its own temporary between the passes.  The memsets go onto the lane's stream.
// Notes the bytes of one lane in m->lane_bytes: what the lane holds, and the plan's temporary where lane 0 borrows it.
static int plan_lane(pa_model* m, Lane& L, const YoloGeometry& g, bool own_tmp) {
    pa_engine* e = m->e;
    const size_t B = (size_t)m->max_batch;
    const size_t A = (size_t)g.A;
    PA_HIP(e, L.d_netin.alloc(B * m->net_h * m->net_w * 4));
    if (plan_buffers(m, L, (int)B, L.stream)) return 1;
    for (int l = 0; l < 3; ++l) L.lv[l] = HeadLevel{L.bptr[m->d.head_buf[l]], g.lv[l].H, g.lv[l].W, g.lv[l].stride, g.lv[l].anchor0};
    PA_HIP(e, L.d_cand.alloc(B * A * 6 * sizeof(float)));
    PA_HIP(e, L.d_cidx.alloc(B * A * sizeof(int32_t)));
    PA_HIP(e, L.d_ccnt.alloc(B * sizeof(int32_t)));
    PA_HIP(e, L.d_keys.alloc(B * g.P2 * sizeof(uint64_t)));
    PA_HIP(e, L.d_order.alloc(B * A * sizeof(int32_t)));
    PA_HIP(e, L.d_supp.alloc(B * A));
    PA_HIP(e, L.d_oboxes.alloc(B * 300 * 6 * sizeof(float)));
    PA_HIP(e, L.d_ocnt.alloc(B * sizeof(int32_t)));
    if (m->d.nk) PA_HIP(e, L.d_okpts.alloc(B * 300 * m->d.nk * sizeof(float)));
    if (own_tmp && m->rs.d_tmp) PA_HIP(e, L.d_rs_tmp.alloc(m->rs.d_tmp.bytes()));
    m->lane_bytes = L.device_bytes() + (own_tmp ? 0 : m->rs.d_tmp.bytes());
    return 0;
}

static int plan_yolo(pa_model* m, int h0, int w0, const pa_yolo_params* p) {
    pa_engine* e = m->e;
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    free_plan(m);
    const int S = p->imgsz;
    YoloGeometry g;
    std::string why;
    if (yolo_geometry(h0, w0, S, p->pre_mode, p->letterbox_auto, g, why)) PA_FAIL(e, "%s", why.c_str());
    m->rw = g.rw; m->rh = g.rh; m->top = g.top; m->left = g.left; m->lb_mode = g.lb_mode;
    m->net_h = g.net_h; m->net_w = g.net_w;
    if (m->lb_mode == 2) {
        std::vector<int32_t> xt, yt;
        cv2_linear_table(w0, m->rw, xt);
        cv2_linear_table(h0, m->rh, yt);
        PA_HIP(e, upload_table(e, m->d_xtab, xt));
        PA_HIP(e, upload_table(e, m->d_ytab, yt));
    }
    if (p->pre_mode == PA_PRE_PIL_STRETCH && resample_plan(e, &m->rs, h0, w0, S, S, PIL_BICUBIC, m->max_batch)) return 1;
    m->A = g.A;
    m->P2 = g.P2;
    m->geom = g;
    if (plan_lane(m, m->ln[0], g, false)) return 1;
    PA_HIP(e, hipStreamSynchronize(m->ln[0].stream));
    m->p_h0 = h0; m->p_w0 = w0; m->p_imgsz = S; m->p_pre = p->pre_mode; m->p_auto = p->letterbox_auto;
    m->planned = true;
    return 0;
}

// May the next ticket go to lane 1?  It exists, or it may be allocated now: the knob and the size gate (second_lane_wanted), and
// no earlier refusal for this plan.
static bool second_lane_ok(const pa_model* m) {
    if (!second_lane_wanted(m->e->t.lanes, m->conv_flops, kLaneGateFlops)) return false;
    return m->ln[1].allocated || !m->lane1_refused;
}

// Lane 1 of a planned model, at the first submit that wants it.  A lane that does not fit (second_lane_fits) or whose allocation
// fails is given up for this plan: the model stays on lane 0, silently and correctly.
static bool alloc_second_lane(pa_model* m) {
    pa_engine* e = m->e;
    Lane& L = m->ln[1];
    size_t free_b = 0, total_b = 0;
    bool ok = hipMemGetInfo(&free_b, &total_b) == hipSuccess && second_lane_fits(free_b, m->lane_bytes, m->arena_bytes);
    if (ok) {
        const std::string err = e->err;
        const size_t arena = m->arena_bytes, logical = m->logical_bytes, lane_bytes = m->lane_bytes;
        ok = plan_lane(m, L, m->geom, true) == 0;
        m->arena_bytes = arena; m->logical_bytes = logical; m->lane_bytes = lane_bytes;      // (pa_model_plan_bytes: one lane's plan)
        if (!ok) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(L.stream);
            free_lane(L);
            e->err = err;
        }
    }
    if (!ok) m->lane1_refused = true;
    return ok;
}

// decode + NMS + scale_boxes / scale_coords of the head maps in L.lv[] for nb images of a planned model, results copied to
// the caller's arrays (rows beyond max_det are never written on device).  oh x ow: the size upstream treats as the source
// (the PIL-resized image on the stretch path).  fused: the op list skipped the heads' last convs (head_fused): the fused head tail
// computes them and the candidate list in place of decode_kernel; the head maps then hold only the keypoint rows NMS reads.
static int run_post(pa_model* m, Lane& L, const pa_yolo_params* p, int nb, int oh, int ow, size_t* ppi, float* out_boxes, float* out_kpts,
                int32_t* out_counts, int ovf_slot, bool fused) {
    pa_engine* e = m->e;
    hipStream_t s = L.stream;
    size_t& pi = *ppi;
    ProfRec* pr = nullptr;
    hipError_t r = hipSuccess;
    const double gain = std::min((double)m->net_h / oh, (double)m->net_w / ow);
    const double kpx = (m->net_w - ow * gain) / 2, kpy = (m->net_h - oh * gain) / 2;
    // ---- decode + NMS
    DecodeArgs da{};
    for (int l = 0; l < 3; ++l) da.lv[l] = L.lv[l];
    da.cs = m->bufs[m->d.head_buf[0]].channels; da.nc = m->d.nc; da.nk = m->d.nk; da.kdim = m->d.kpt_dim;
    da.A = m->A; da.B = nb; da.conf = p->conf; da.classes = m->d_classes.get(); da.n_classes = p->n_classes;
    da.cand = L.d_cand.get(); da.cand_idx = L.d_cidx.get(); da.cand_cnt = L.d_ccnt.get();
    pr = prof_begin(m, s, pi++, PROF_DECODE, 0, 0.0);
    if (fused) {
        HeadTailArgs ha{};
        ha.d = da;
        head_tail_convs(m, L, ha);
        r = launch_head_tail_h2(ha, s);
    } else {
        r = launch_decode(da, s);
    }
    prof_end(s, pr);
    if (r != hipSuccess) PA_FAIL(e, "%s launch failed: %s", fused ? "fused head tail" : "decode", hipGetErrorString(r));
    m->last_post_path = fused ? 1 : 0;
    m->heads_stale = fused;
    NmsArgs na{};
    na.cand = L.d_cand.get(); na.cand_idx = L.d_cidx.get(); na.cand_cnt = L.d_ccnt.get(); na.keys = L.d_keys.get();
    na.order = L.d_order.get(); na.supp = L.d_supp.get();
    for (int l = 0; l < 3; ++l) na.lv[l] = L.lv[l];
    na.cs = da.cs; na.nc = m->d.nc; na.nk = m->d.nk; na.kdim = m->d.kpt_dim; na.A = m->A; na.B = nb; na.P2 = m->P2;
    na.iou = p->iou; na.max_det = p->max_det; na.max_nms = 30000;
    na.gain = (float)gain;
    na.pad_x = (float)std::nearbyint(kpx - 0.1); na.pad_y = (float)std::nearbyint(kpy - 0.1);
    na.kpad_x = (float)kpx; na.kpad_y = (float)kpy;
    na.w0 = (float)ow; na.h0 = (float)oh;
    na.out_boxes = L.d_oboxes.get(); na.out_kpts = L.d_okpts.get(); na.out_cnt = L.d_ocnt.get();
    pr = prof_begin(m, s, pi++, PROF_NMS, 0, 0.0);
    r = launch_nms(na, s);
    prof_end(s, pr);
    if (r != hipSuccess) PA_FAIL(e, "nms launch failed: %s", hipGetErrorString(r));
    // ---- results back to the caller's arrays (rows beyond max_det are never written on device)
    if (guards_range(m))      // the overflow flag travels with the results: pa_model_take_overflow needs no device round trip
        PA_HIP(e, hipMemcpyAsync(m->h_pin.get() + ovf_slot, m->d_ovf.get(), sizeof(unsigned), hipMemcpyDeviceToHost, s));
    PA_HIP(e, hipMemcpyAsync(out_counts, L.d_ocnt.get(), nb * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PA_HIP(e, hipMemcpyAsync(out_boxes, L.d_oboxes.get(),
                             (size_t)nb * p->max_det * 6 * sizeof(float), hipMemcpyDeviceToHost, s));
    if (m->d.nk)
        PA_HIP(e, hipMemcpyAsync(out_kpts, L.d_okpts.get(),
                                 (size_t)nb * p->max_det * m->d.nk * sizeof(float), hipMemcpyDeviceToHost, s));
    return 0;
}

// is the plan the one this call needs?
static bool yolo_plan_current(const pa_model* m, int h, int w, const pa_yolo_params* p) {
    return m->planned && m->p_h0 == h && m->p_w0 == w && m->p_imgsz == p->imgsz && m->p_pre == p->pre_mode &&
           m->p_auto == p->letterbox_auto && m->p_batch == m->max_batch;
}

// the class filter of a call in d_classes; uploaded only when the caller's list differs from the one the device holds
static int set_classes(pa_model* m, const pa_yolo_params* p) {
    pa_engine* e = m->e;
    if (p->n_classes <= 0) return 0;
    if ((int)m->classes_host.size() == p->n_classes && !memcmp(m->classes_host.data(), p->classes, p->n_classes * sizeof(int32_t))) return 0;
    // (the device list is read by queued decode kernels: replace it only once they are done)
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));        // (behind every ticket's join)
    PA_HIP(e, e->sync_lanes());
    const size_t bytes = p->n_classes * sizeof(int32_t);
    if (m->d_classes.bytes() < bytes) m->classes_host.clear();          // the device list is about to go
    PA_HIP(e, m->d_classes.fit(bytes, bytes));
    m->classes_host.assign(p->classes, p->classes + p->n_classes);
    PA_HIP(e, hipMemcpy(m->d_classes.get(), m->classes_host.data(), p->n_classes * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

// argument checks + plan of a pa_yolo_infer / pa_yolo_submit call, class filter upload
static int yolo_prepare(pa_model* m, const uint8_t* frames, int n, int h, int w, const pa_yolo_params* p, float* out_boxes,
                        float* out_kpts, int32_t* out_counts, const char* who) {
    pa_engine* e = m->e;
    if (m->d.task != PA_TASK_DETECT && m->d.task != PA_TASK_POSE) PA_FAIL(e, "%s on a non-YOLO model", who);
    if (!frames || n <= 0 || h <= 0 || w <= 0 || !out_boxes || !out_counts) PA_FAIL(e, "%s: bad arguments", who);
    if (m->d.nk && !out_kpts) PA_FAIL(e, "%s: out_kpts is NULL for a pose model", who);
    if (p->max_det < 1 || p->max_det > 300) PA_FAIL(e, "max_det %d outside [1,300]", p->max_det);
    PA_HIP(e, hipSetDevice(e->dev));
    if (!yolo_plan_current(m, h, w, p)) {
        if (m->n_inflight) PA_FAIL(e, "%s: the plan would change (source size / imgsz / batch) with %d ticket(s) in flight", who, m->n_inflight);
        if (plan_yolo(m, h, w, p)) return 1;
    }
    return set_classes(m, p);
}

// everything one batch of nb <= max_batch frames needs, enqueued on lane li's stream behind what the main stream held at the call
// (fork_lane): upload (host frames), preprocessing, network, decode, NMS, result copies (the overflow flag of h2 and fp16 models into
// h_pin[ovf_slot]).  Does not wait.
static int yolo_enqueue(pa_model* m, int li, const uint8_t* src, int nb, int h, int w, const pa_yolo_params* p, float* out_boxes,
                        float* out_kpts, int32_t* out_counts, int ovf_slot, size_t* ppi) {
    pa_engine* e = m->e;
    Lane& L = m->ln[li];
    hipStream_t s = L.stream;
    PA_HIP(e, e->fork_lane(li));
    m->last_lane = li;
    size_t& pi = *ppi;
    const size_t frame_bytes = (size_t)h * w * 3;
    const int S = p->imgsz;
    // scale_boxes / scale_coords parameters (upstream treats the PIL-resized image as the source)
    const int oh = p->pre_mode == PA_PRE_PIL_STRETCH ? S : h, ow = p->pre_mode == PA_PRE_PIL_STRETCH ? S : w;
    if (!p->frames_on_device && stage_frames(m, &src, nb, frame_bytes, s)) return 1;
    // ---- preprocessing -> u8 NHWC4 network input
    ProfRec* pr = prof_begin(m, s, pi++, PROF_PRE, 0, 0.0);
    hipError_t r = hipSuccess;
    if (p->pre_mode == PA_PRE_LETTERBOX || (h == S && w == S)) {
        LetterboxArgs a{};
        a.src = src; a.dst = L.d_netin.get(); a.B = nb; a.h0 = h; a.w0 = w; a.rw = m->rw; a.rh = m->rh;
        a.top = m->top; a.left = m->left; a.nh = m->net_h; a.nw = m->net_w; a.mode = m->lb_mode;
        a.reverse = p->channel_reverse; a.xtab = m->d_xtab.get(); a.ytab = m->d_ytab.get();
        r = launch_letterbox(a, s);
    } else {
        r = resample_enqueue(m->rs, src, L.d_netin.get(), nb, 4, p->channel_reverse, s, L.d_rs_tmp.get());
    }
    prof_end(s, pr);
    if (r != hipSuccess) PA_FAIL(e, "preprocess launch failed: %s", hipGetErrorString(r));
    // ---- network (without the heads' last convs when the fused head tail runs them: decided once, here)
    const bool fused = head_fused(m);
    if (run_graph(m, L, s, nb, &pi, fused)) return 1;
    // ---- decode + NMS + results back to the caller's arrays
    return run_post(m, L, p, nb, oh, ow, &pi, out_boxes, m->d.nk ? out_kpts : nullptr, out_counts, ovf_slot, fused);
}

int pa_yolo_infer(pa_model* m, const uint8_t* frames, int n, int h, int w, const pa_yolo_params* p,
                  float* out_boxes, float* out_kpts, int32_t* out_counts) {
    if (!m || !p) return 1;
    pa_engine* e = m->e;
    if (yolo_prepare(m, frames, n, h, w, p, out_boxes, out_kpts, out_counts, "pa_yolo_infer")) return 1;
    hipStream_t s = m->ln[0].stream;          // synchronous calls run on lane 0
    const size_t frame_bytes = (size_t)h * w * 3;
    size_t pi = 0;
    for (int c0 = 0; c0 < n; c0 += m->max_batch) {
        const int nb = std::min(m->max_batch, n - c0);
        if (yolo_enqueue(m, 0, frames + (size_t)c0 * frame_bytes, nb, h, w, p, out_boxes + (size_t)c0 * p->max_det * 6,
                         m->d.nk ? out_kpts + (size_t)c0 * p->max_det * m->d.nk : nullptr, out_counts + c0, PA_MAX_INFLIGHT, &pi))
            return 1;
        PA_HIP(e, hipStreamSynchronize(s));
        m->last_n = nb;
        if (guards_range(m)) { m->h_ovf |= m->h_pin.get()[PA_MAX_INFLIGHT]; m->ovf_cached = true; }
    }
    PA_HIP(e, e->sync_lanes());          // a synchronous call completes every ticket still in flight, on either lane: their waits return at once
    finish_profile(m, pi);
    return 0;
}

int pa_yolo_submit(pa_model* m, const uint8_t* frames, int n, int h, int w, const pa_yolo_params* p,
                   float* out_boxes, float* out_kpts, int32_t* out_counts, int* ticket) {
    if (!m || !p || !ticket) return 1;
    pa_engine* e = m->e;
    if (!p->frames_on_device) PA_FAIL(e, "pa_yolo_submit: frames must be in HBM (frames_on_device = 1)");
    if (n > m->max_batch) PA_FAIL(e, "pa_yolo_submit: n = %d > max_batch %d", n, m->max_batch);
    if (e->profiling || e->t.timeline) PA_FAIL(e, "pa_yolo_submit: not while profiling (use pa_yolo_infer)");
    const int slot = m->next_ticket % PA_MAX_INFLIGHT;
    if (m->tk_busy[slot]) PA_FAIL(e, "pa_yolo_submit: %d tickets in flight (PA_MAX_INFLIGHT)", PA_MAX_INFLIGHT);
    if (yolo_prepare(m, frames, n, h, w, p, out_boxes, out_kpts, out_counts, "pa_yolo_submit")) return 1;
    const LaneState st[kMaxLanes] = {m->ln[0].st, m->ln[1].st};
    int li = pick_lane(st, second_lane_ok(m));
    if (li == 1 && !m->ln[1].allocated && !alloc_second_lane(m)) li = 0;
    Lane& L = m->ln[li];
    size_t pi = 0;
    if (yolo_enqueue(m, li, frames, n, h, w, p, out_boxes, out_kpts, out_counts, slot, &pi)) {
        // part of the call may be queued already (preprocessing, some layers) and would write into the caller's arrays with
        // no ticket to wait on: drain before reporting the failure
        (void)hipStreamSynchronize(L.stream);
        return 1;
    }
    PA_HIP(e, hipEventRecord(m->tk_ev[slot], L.stream));
    // join: whatever goes onto the main stream from here on runs behind this ticket, as when the ticket itself ran there
    PA_HIP(e, e->join_lane(m->tk_ev[slot]));
    L.st.busy = true;
    L.st.last_ticket = m->next_ticket;
    m->tk_lane[slot] = li;
    m->tk_busy[slot] = true;
    ++m->n_inflight;
    m->last_n = n;
    m->n_prof = 0;
    m->ovf_cached = false;
    *ticket = m->next_ticket++;
    return 0;
}

int pa_yolo_wait(pa_model* m, int ticket, int* overflow) {
    if (!m) return 1;
    pa_engine* e = m->e;
    const int slot = ticket % PA_MAX_INFLIGHT;
    if (ticket < 0 || ticket >= m->next_ticket || ticket + PA_MAX_INFLIGHT < m->next_ticket || !m->tk_busy[slot])
        PA_FAIL(e, "pa_yolo_wait: ticket %d is not in flight", ticket);
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipEventSynchronize(m->tk_ev[slot]));
    m->tk_busy[slot] = false;
    --m->n_inflight;
    Lane& L = m->ln[m->tk_lane[slot]];
    if (L.st.last_ticket == ticket) L.st.busy = false;
    if (overflow) *overflow = (guards_range(m) && m->h_pin.get()[slot]) ? 1 : 0;
    return 0;
}

int pa_yolo_postprocess(pa_model* m, const float* const* heads, int n, int h, int w, const pa_yolo_params* p,
                        float* out_boxes, float* out_kpts, int32_t* out_counts) {
    if (!m || !p || !heads) return 1;
    pa_engine* e = m->e;
    if (m->d.task != PA_TASK_DETECT && m->d.task != PA_TASK_POSE) PA_FAIL(e, "pa_yolo_postprocess on a non-YOLO model");
    if (n <= 0 || n > m->max_batch || !out_boxes || !out_counts || (m->d.nk && !out_kpts)) PA_FAIL(e, "pa_yolo_postprocess: bad arguments");
    if (p->max_det < 1 || p->max_det > 300) PA_FAIL(e, "max_det %d outside [1,300]", p->max_det);
    PA_HIP(e, hipSetDevice(e->dev));
    if (!yolo_plan_current(m, h, w, p) && plan_yolo(m, h, w, p)) return 1;
    if (set_classes(m, p)) return 1;
    Lane& L = m->ln[0];
    hipStream_t s = L.stream;
    PA_HIP(e, e->fork_lane(0));
    m->last_lane = 0;
    const int cs = m->bufs[m->d.head_buf[0]].channels;
    for (int l = 0; l < 3; ++l) {
        if (!heads[l]) PA_FAIL(e, "pa_yolo_postprocess: heads[%d] is NULL", l);
        PA_HIP(e, hipMemcpyAsync(const_cast<float*>(L.lv[l].buf), heads[l], (size_t)n * L.lv[l].H * L.lv[l].W * cs * sizeof(float),
                                 hipMemcpyHostToDevice, s));
    }
    const int S = p->imgsz;
    const int oh = p->pre_mode == PA_PRE_PIL_STRETCH ? S : h, ow = p->pre_mode == PA_PRE_PIL_STRETCH ? S : w;
    size_t pi = 0;
    if (run_post(m, L, p, n, oh, ow, &pi, out_boxes, out_kpts, out_counts, PA_MAX_INFLIGHT, false)) return 1;
    PA_HIP(e, e->sync_lanes());
    m->last_n = n;
    finish_profile(m, pi);
    return 0;
}

int pa_yolo_head_shape(pa_model* m, int level, int* h, int* w, int* c) {
    if (!m->planned || level < 0 || level > 2) PA_FAIL(m->e, "pa_yolo_head_shape: no plan / bad level");
    *h = m->ln[0].lv[level].H; *w = m->ln[0].lv[level].W; *c = m->bufs[m->d.head_buf[0]].channels;
    return 0;
}

int pa_yolo_read_head(pa_model* m, int level, int n, float* out) {
    pa_engine* e = m->e;
    if (m->d.task != PA_TASK_DETECT && m->d.task != PA_TASK_POSE) PA_FAIL(e, "pa_yolo_read_head on a non-YOLO model");
    if (!m->planned || level < 0 || level > 2 || n > m->last_n) PA_FAIL(e, "pa_yolo_read_head: no plan / bad level / n");
    PA_HIP(e, hipSetDevice(e->dev));
    Lane& L = m->ln[m->last_lane];          // the lane of the model's last call
    hipStream_t s = L.stream;
    if (m->heads_stale) {          // the last call ran the fused head tail: the maps of its last_n images from the tail convs' inputs, once
        if (run_tail_ops(m, L, s, m->last_n)) return 1;
        m->heads_stale = false;
    }
    const size_t bytes = (size_t)n * L.lv[level].H * L.lv[level].W * m->bufs[m->d.head_buf[0]].channels * sizeof(float);
    PA_HIP(e, hipMemcpyAsync(out, L.lv[level].buf, bytes, hipMemcpyDeviceToHost, s));
    PA_HIP(e, hipStreamSynchronize(s));
    return 0;
}

int pa_yolo_resample_passes(pa_model* m) {
    if (!m || !m->planned) return 0;
    const ResamplePlan& r = m->rs;
    const int passes = (r.sw != r.dw ? 1 : 0) + (r.sh != r.dh ? 1 : 0);
    return passes == 2 && !r.d_tmp ? -1 : passes;          // (two passes always have their temporary)
}

int pa_yolo_last_post_path(pa_model* m) { return m ? m->last_post_path : 0; }

int pa_yolo_netin_shape(pa_model* m, int* h, int* w) {
    if (!m->planned || m->d.task == PA_TASK_TRACKNET) PA_FAIL(m->e, "pa_yolo_netin_shape: no YOLO plan");
    *h = m->net_h; *w = m->net_w;
    return 0;
}

int pa_yolo_read_netin(pa_model* m, int n, uint8_t* out) {
    pa_engine* e = m->e;
    if (!m->planned || !m->ln[0].d_netin || n < 1 || n > m->last_n || !out) PA_FAIL(e, "pa_yolo_read_netin: no plan / bad n");
    PA_HIP(e, hipSetDevice(e->dev));
    Lane& L = m->ln[m->last_lane];
    const hipStream_t s = L.stream ? L.stream : e->main_stream();          // (a ResNet plan has a network input too: it runs on the main stream)
    PA_HIP(e, hipMemcpyAsync(out, L.d_netin.get(), (size_t)n * m->net_h * m->net_w * 4, hipMemcpyDeviceToHost, s));
    PA_HIP(e, hipStreamSynchronize(s));
    return 0;
}
