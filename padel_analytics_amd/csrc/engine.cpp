// libpadel_hip.so — engine: owns the streams of one GPU (the main stream that orders its work, two lane streams for in-flight
// YOLO batches, a copy stream), the packed weights and every activation buffer in HBM, plans a graph for a (source size, imgsz, batch) and replays it per batch.
// C-ABI declared in include/padel_hip.h.  This file: engine and model lifecycle, tuning, memory and timer calls, the arena,
// the op-list replay (run_ops / run_graph: the step list of launch_plan.cpp, launched step by step) and the profile text;
// engine_internal.h names the other files.
#include "engine_internal.h"

#include <atomic>

thread_local std::string g_err;

// device_mem.h's hooks: every allocation a DevMem / PinMem of the engine owns is made and released here, and the device bytes
// they hold are counted for the whole process (pa_device_bytes_live: a release that was forgotten shows as a number)
static std::atomic<size_t> g_live_bytes{0};
int dev_alloc(void** p, size_t bytes) { const hipError_t r = hipMalloc(p, bytes); if (r == hipSuccess) g_live_bytes += bytes; return (int)r; }
void dev_free(void* p, size_t bytes) { (void)hipFree(p); g_live_bytes -= bytes; }
int pin_alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
void pin_free(void* p, size_t) { (void)hipHostFree(p); }
size_t pa_device_bytes_live(void) { return g_live_bytes.load(); }

// Every tuning knob but `impl` (whose environment value is a word): pa_engine_set_tuning key, environment variable read once at
// pa_engine_create (none: set_tuning only), field, and how a value is normalised on both ways in.  A flag is only ever tested
// for truth; fuse_stem / fuse_sppf keep the raw value (fuse_sppf 2..4 force a workgroup size, kernels_misc.hip).
static int knob_raw(int v) { return v; }
static int knob_tune(int v) { return v & kTuneMask; }      // launch_plan.h: no other bit selects anything
static int knob_flag(int v) { return v ? 1 : 0; }
static int knob_tap_pd(int v) { return v == 3 ? 3 : 2; }
static int knob_lanes(int v) { return v >= 2 ? 2 : 1; }
static const struct Knob { const char* key; const char* env; int Tuning::*field; int (*norm)(int); } kKnobs[] = {
    {"variant", "PADEL_CONV_VARIANT", &Tuning::variant, knob_raw},
    {"tune", "PADEL_CONV_TUNE", &Tuning::tune, knob_tune},
    {"tap_pd", "PADEL_CONV_TAP_PD", &Tuning::tap_pd, knob_tap_pd},
    {"graph", "PADEL_GRAPH", &Tuning::graph, knob_flag},
    {"timeline", nullptr, &Tuning::timeline, knob_flag},
    {"alias", "PADEL_ALIAS", &Tuning::alias, knob_flag},
    {"fold_up", "PADEL_FOLD_UP", &Tuning::fold_up, knob_flag},
    {"lanes", "PADEL_LANES", &Tuning::lanes, knob_lanes},
    {"fuse_stem", "PADEL_FUSE_STEM", &Tuning::fuse_stem, knob_raw},
    {"fuse_sppf", "PADEL_FUSE_SPPF", &Tuning::fuse_sppf, knob_raw},
    {"fuse_head", "PADEL_FUSE_HEAD", &Tuning::fuse_head, knob_flag},
    {"fuse_stem_cv1", "PADEL_FUSE_STEM_CV1", &Tuning::fuse_stem_cv1, knob_flag},
    {"w_single", nullptr, &Tuning::w_single, knob_flag},
};

int pa_abi_version(void) { return PA_ABI_VERSION; }

int pa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* pa_last_error(pa_engine* eng) { return eng ? eng->err.c_str() : g_err.c_str(); }

int pa_engine_create(int device_id, pa_engine** out) {
    if (!out) PA_FAIL((pa_engine*)nullptr, "pa_engine_create: out is NULL");
    int n = 0;
    PA_HIP((pa_engine*)nullptr, hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n) PA_FAIL((pa_engine*)nullptr, "pa_engine_create: device %d of %d", device_id, n);
    PA_HIP((pa_engine*)nullptr, hipSetDevice(device_id));
    pa_engine* e = new pa_engine();
    e->dev = device_id;
    hipError_t r = e->create_streams();
    if (r == hipSuccess) r = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking);
    if (r != hipSuccess) { pa_engine_destroy(e); PA_FAIL((pa_engine*)nullptr, "hipStreamCreate: %s", hipGetErrorString(r)); }
    r = (hipError_t)e->zeros.alloc(256);
    if (r == hipSuccess) r = hipMemset(e->zeros.get(), 0, 256);
    if (r != hipSuccess) { delete e; PA_FAIL((pa_engine*)nullptr, "zero page: %s", hipGetErrorString(r)); }
    r = padel::init_misc_kernels();
    if (r == hipSuccess) r = padel::init_head_tail_kernels();
    if (r != hipSuccess) { delete e; PA_FAIL((pa_engine*)nullptr, "kernel attributes: %s", hipGetErrorString(r)); }
    if (const char* v = getenv("PADEL_CONV_IMPL")) {       // tap | bx3 ("lds", the kernel retired in round 5, is refused — it used to select tap silently)
        if (v[0] == 'l') { delete e; PA_FAIL((pa_engine*)nullptr, "PADEL_CONV_IMPL=%s: the LDS kernel was retired in round 5; tap or bx3", v); }
        e->t.impl = (v[0] == 'b') ? 2 : 0;
    }
    for (const Knob& k : kKnobs)
        if (const char* v = k.env ? getenv(k.env) : nullptr) e->t.*k.field = k.norm(atoi(v));
    *out = e;
    return 0;
}

hipError_t pa_engine::create_streams() {
    hipError_t r = hipStreamCreateWithFlags(&main_, hipStreamNonBlocking);
    for (int i = 0; i < kMaxLanes && r == hipSuccess; ++i) {
        r = hipStreamCreateWithFlags(&lane_stream[i], hipStreamNonBlocking);
        if (r == hipSuccess) r = hipEventCreateWithFlags(&fork_ev_[i], hipEventDisableTiming);
    }
    return r;
}

void pa_engine::destroy_streams() {
    for (int i = 0; i < kMaxLanes; ++i) {
        if (lane_stream[i]) { hipStreamSynchronize(lane_stream[i]); hipStreamDestroy(lane_stream[i]); }
        if (fork_ev_[i]) hipEventDestroy(fork_ev_[i]);
        lane_stream[i] = nullptr; fork_ev_[i] = nullptr;
    }
    if (main_) hipStreamDestroy(main_);
    main_ = nullptr;
}

hipError_t pa_engine::fork_lane(int i) {
    if (forked_seq_[i] == main_seq_) return hipSuccess;      // only joins since: waiting would put this lane behind the other one's ticket
    hipError_t r = hipEventRecord(fork_ev_[i], main_);
    if (r == hipSuccess) r = hipStreamWaitEvent(lane_stream[i], fork_ev_[i], 0);
    if (r == hipSuccess) forked_seq_[i] = main_seq_;
    return r;
}

hipError_t pa_engine::sync_lanes() {
    for (hipStream_t s : lane_stream)
        if (s) { const hipError_t r = hipStreamSynchronize(s); if (r != hipSuccess) return r; }
    return hipSuccess;
}

int pa_engine_set_tuning(pa_engine* e, const char* key, int value) {
    if (!e || !key) return 1;
    if (!strcmp(key, "impl")) {                             // 0: fp32-input MFMA tap kernels, 2: bf16x3
        if (value != 0 && value != 2) PA_FAIL(e, "tuning impl = %d: 0 (fp32-input MFMA tap kernels) or 2 (bf16x3); 1 was the LDS kernel, retired in round 5 (tools/legacy_conv)", value);
        e->t.impl = value;
    } else {
        const Knob* k = std::find_if(std::begin(kKnobs), std::end(kKnobs), [&](const Knob& c) { return !strcmp(c.key, key); });
        if (k == std::end(kKnobs)) PA_FAIL(e, "pa_engine_set_tuning: unknown key '%s'", key);
        e->t.*k->field = k->norm(value);
    }
    e->tuning_epoch++;
    return 0;
}

int pa_engine_set_timeline_path(pa_engine* e, const char* path) {
    if (!e) return 1;
    e->timeline_path = path ? path : "";
    return 0;
}

void pa_engine_destroy(pa_engine* e) {
    if (!e) return;
    hipSetDevice(e->dev);
    pa_engine_comm_destroy(e);
    if (e->main_stream_wait_only()) hipStreamSynchronize(e->main_stream_wait_only());
    jpeg_scratch_free(e);
    jpeg_dec_scratch_free(e);
    for (hipEvent_t ev : e->timer_ev) if (ev) hipEventDestroy(ev);
    e->destroy_streams();
    if (e->copy_stream) hipStreamDestroy(e->copy_stream);
    delete e;          // zeros, yuv_stage, render_stage, warp_stage, heat_stage, activity_stage, box_stage: idle since the wait above
}

int pa_engine_synchronize(pa_engine* e) {
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    return 0;
}

int pa_engine_set_profiling(pa_engine* e, int enable) { e->profiling = enable != 0; return 0; }

int pa_device_malloc(pa_engine* e, size_t nbytes, void** out) {
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipMalloc(out, nbytes));
    return 0;
}
int pa_device_free(pa_engine* e, void* p) {
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipFree(p));
    return 0;
}
int pa_memcpy_h2d(pa_engine* e, void* dst, const void* src, size_t n) {
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, e->main_stream()));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    return 0;
}
int pa_upload(pa_engine* e, void* dst, const void* src, size_t n) {
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, e->copy_stream));
    PA_HIP(e, hipStreamSynchronize(e->copy_stream));
    return 0;
}
int pa_host_register(pa_engine* e, void* ptr, size_t nbytes) {
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipHostRegister(ptr, nbytes, hipHostRegisterDefault));
    return 0;
}
int pa_host_unregister(pa_engine* e, void* ptr) {
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipHostUnregister(ptr));
    return 0;
}
int pa_memcpy_d2h(pa_engine* e, void* dst, const void* src, size_t n) {
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, e->main_stream()));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    return 0;
}

int pa_engine_timer_start(pa_engine* e) {
    if (!e) return 1;
    PA_HIP(e, hipSetDevice(e->dev));
    for (hipEvent_t& ev : e->timer_ev) if (!ev) PA_HIP(e, hipEventCreate(&ev));
    PA_HIP(e, hipEventRecord(e->timer_ev[0], e->main_stream()));
    return 0;
}
int pa_engine_timer_stop(pa_engine* e, float* ms) {
    if (!e || !ms) return 1;
    if (!e->timer_ev[0] || !e->timer_ev[1]) PA_FAIL(e, "pa_engine_timer_stop without pa_engine_timer_start");
    PA_HIP(e, hipSetDevice(e->dev));
    PA_HIP(e, hipEventRecord(e->timer_ev[1], e->main_stream()));
    PA_HIP(e, hipEventSynchronize(e->timer_ev[1]));
    PA_HIP(e, hipEventElapsedTime(ms, e->timer_ev[0], e->timer_ev[1]));
    return 0;
}

// ------------------------------------------------------------------------------- model
int pa_model_create(pa_engine* e, const pa_model_desc* desc, const float* weights, size_t n_floats, pa_model** out) {
    // weights == NULL: the blob is allocated zero-filled and arrives through pa_engine_bcast_weights
    if (!e || !desc || !out) PA_FAIL(e, "pa_model_create: NULL argument");
    std::string why;
    if (validate_desc(desc, n_floats, why)) PA_FAIL(e, "%s", why.c_str());
    PA_HIP(e, hipSetDevice(e->dev));
    pa_model* m = new pa_model();
    m->e = e;
    m->d = *desc;
    m->bufs.assign(desc->bufs, desc->bufs + desc->n_bufs);
    m->ops.assign(desc->ops, desc->ops + desc->n_ops);
    m->d.bufs = m->bufs.data();
    m->d.ops = m->ops.data();
    std::vector<int> fold_dst;
    find_upsample_folds(m->d, m->fold_src, fold_dst);
    m->stem_fuse.resize(m->ops.size());
    for (size_t i = 0; i < m->ops.size(); ++i) m->stem_fuse[i] = stem_cv1_fusable(m->d, i) ? 2 : stem_fusable(m->d, i) ? 1 : 0;
    m->tail = find_head_tail(m->d, m->fold_src);
    m->n_w = n_floats;
    if (desc->task == PA_TASK_DETECT || desc->task == PA_TASK_POSE)
        for (int i = 0; i < kMaxLanes; ++i) m->ln[i].stream = e->lane_stream[i];
    hipError_t r = (hipError_t)m->d_w.alloc(n_floats * sizeof(float) + kConvReadSlack);
    if (r == hipSuccess)
        r = weights ? hipMemcpyAsync(m->d_w.get(), weights, n_floats * sizeof(float), hipMemcpyHostToDevice, e->main_stream())
                    : hipMemsetAsync(m->d_w.get(), 0, n_floats * sizeof(float), e->main_stream());
    if (r == hipSuccess) r = hipMemsetAsync(m->d_w.get() + n_floats, 0, kConvReadSlack, e->main_stream());
    if (r == hipSuccess) r = (hipError_t)m->d_ovf.alloc(256);
    if (r == hipSuccess) r = hipMemsetAsync(m->d_ovf.get(), 0, 256, e->main_stream());
    if (r == hipSuccess) r = (hipError_t)m->h_pin.alloc(64 * sizeof(unsigned));
    if (r == hipSuccess) memset(m->h_pin.get(), 0, 64 * sizeof(unsigned));
    for (int k = 0; k < PA_MAX_INFLIGHT && r == hipSuccess; ++k) r = hipEventCreateWithFlags(&m->tk_ev[k], hipEventDisableTiming);
    if (r == hipSuccess) r = hipStreamSynchronize(e->main_stream_wait_only());
    if (r != hipSuccess) { delete m; PA_FAIL(e, "weights upload: %s", hipGetErrorString(r)); }
    *out = m;
    return 0;
}

static void destroy_graphs(pa_model* m) {
    for (Lane& L : m->ln) {
        for (auto& g : L.graphs) hipGraphExecDestroy(g.second);
        L.graphs.clear();
    }
}

void free_lane(Lane& L) {
    for (auto& g : L.graphs) hipGraphExecDestroy(g.second);
    L.graphs.clear();
    const hipStream_t s = L.stream;
    L = Lane{};
    L.stream = s;
}

void free_plan(pa_model* m) {
    (void)m->e->sync_lanes();
    for (Lane& L : m->ln) free_lane(L);
    m->d_xtab.reset();
    m->d_ytab.reset();
    m->rs = ResamplePlan{};
    m->lane1_refused = false;
    m->last_lane = 0;
    m->planned = false;
    m->heads_stale = false;
}

void pa_model_destroy(pa_model* m) {
    if (!m) return;
    hipSetDevice(m->e->dev);
    hipStreamSynchronize(m->e->main_stream_wait_only());      // (behind every ticket's join; free_plan drains the lanes themselves)
    free_plan(m);
    for (auto& r : m->prof) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    for (int k = 0; k < PA_MAX_INFLIGHT; ++k) if (m->tk_ev[k]) hipEventDestroy(m->tk_ev[k]);
    delete m;          // weights, operand copies, flags, staging: idle since the wait above
}

int pa_model_take_overflow(pa_model* m, int* out) {
    if (!m || !out) return 1;
    pa_engine* e = m->e;
    *out = 0;
    if (!guards_range(m)) return 0;
    PA_HIP(e, hipSetDevice(e->dev));
    unsigned v = 0;
    if (m->ovf_cached) {                 // pa_yolo_infer read the flag back with its results (nothing has run on the model since)
        v = m->h_ovf;
    } else {
        PA_HIP(e, hipMemcpyAsync(&v, m->d_ovf.get(), sizeof(v), hipMemcpyDeviceToHost, e->main_stream()));
        PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    }
    m->ovf_cached = false;
    m->h_ovf = 0;
    if (v) {
        PA_HIP(e, hipMemsetAsync(m->d_ovf.get(), 0, sizeof(v), e->main_stream()));
        PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    }
    *out = v ? 1 : 0;
    return 0;
}

int pa_model_set_max_batch(pa_model* m, int max_batch) {
    if (max_batch < 1) PA_FAIL(m->e, "max_batch %d", max_batch);
    if (max_batch != m->max_batch) { hipSetDevice(m->e->dev); hipStreamSynchronize(m->e->main_stream_wait_only()); free_plan(m); m->max_batch = max_batch; }
    return 0;
}

// The activation arena of a model whose network input size is set: graph_plan.cpp decides which buffers share bytes
// (plan_activations), this allocates and zeroes what it asks for.
int plan_buffers(pa_model* m, Lane& L, int batch, hipStream_t s) {
    pa_engine* e = m->e;
    BufferPlan bp;
    std::string why;
    if (plan_activations(m->d, m->fold_src, m->net_h, m->net_w, batch, e->t.alias != 0, bp, why, &m->tail)) PA_FAIL(e, "%s", why.c_str());
    m->fc_nout = 0;
    m->conv_flops = 0;
    for (const auto& o : m->ops) {
        if (o.kind == PA_OP_GAP_FC) m->fc_nout = o.cout;
        if (o.kind == PA_OP_CONV) {
            const int lvl = m->bufs[o.out_buf].level;
            m->conv_flops += 2.0 * batch * (double)(m->net_h >> lvl) * (m->net_w >> lvl) * o.cout * o.cin * o.ksize * o.ksize;
        }
    }
    if (m->fc_nout) {
        PA_HIP(e, L.d_fc.alloc((size_t)batch * 2 * kGapFcMaxOut * sizeof(float)));
        PA_HIP(e, hipMemsetAsync(L.d_fc.get(), 0, (size_t)batch * 2 * kGapFcMaxOut * sizeof(float), s));
    }
    PA_HIP(e, L.arena.alloc(bp.arena_bytes + kConvReadSlack));
    PA_HIP(e, hipMemsetAsync(L.arena.get(), 0, bp.arena_bytes + kConvReadSlack, s));
    L.bptr.assign(m->bufs.size(), nullptr);
    for (size_t i = 0; i < m->bufs.size(); ++i) L.bptr[i] = reinterpret_cast<float*>(L.arena.get() + bp.off[i]);
    L.allocated = true;
    m->arena_bytes = bp.arena_bytes;
    m->logical_bytes = bp.logical_bytes;
    m->p_batch = batch;
    return 0;
}

ProfRec* prof_begin(pa_model* m, hipStream_t s, size_t idx, int kind, int ksize, double flops) {
    if (!m->e->profiling) return nullptr;
    if (m->prof.size() <= idx) {
        m->prof.resize(idx + 1);
        hipEventCreate(&m->prof[idx].e0);
        hipEventCreate(&m->prof[idx].e1);
    }
    ProfRec* r = &m->prof[idx];
    r->kind = kind; r->ksize = ksize; r->flops = flops; r->ms = 0.f;
    r->M = r->cout = r->cin = r->stride = r->mf = r->nf = r->res = 0;
    r->tile = -1; r->family = "";
    hipEventRecord(r->e0, s);
    return r;
}

// the base pointers of a replay on lane L (launch_plan.h; their lifetime: the audit at struct Lane)
static PlanPointers plan_pointers(const pa_model* m, const Lane& L) {
    return PlanPointers{L.bptr.data(), m->d_w.get(), m->d_wr.get(), m->wr_valid ? m->wr_off.data() : nullptr, m->e->zeros.get(), m->d_ovf.get(),
                        L.d_netin.get(), L.d_fc.get(), m->p_batch};
}

// the launches of one replay for n images into L.steps; a refusal leaves the list empty and nothing enqueued
static int plan_steps(pa_model* m, Lane& L, int n) {
    std::string why;
    if (build_steps(m->d, m->fold_src, m->stem_fuse, m->tail, m->e->t, plan_pointers(m, L), m->net_h, m->net_w, n, L.steps, why,
                    hipGetErrorString(hipErrorNotSupported)))
        PA_FAIL(m->e, "%s", why.c_str());
    return 0;
}

void head_tail_convs(const pa_model* m, const Lane& L, HeadTailArgs& a) {
    bool single = m->e->t.w_single != 0;
    for (int l = 0; l < 3; ++l)
        for (int c = 0; c < 3; ++c) {
            HeadTailConv& v = a.cv[l][c];
            v = HeadTailConv{};
            const int i = m->tail.op[l][c];
            if (i < 0) continue;
            const pa_op_desc& o = m->ops[i];
            v.in = L.bptr[o.in_buf]; v.in_cs = m->bufs[o.in_buf].channels; v.in_choff = o.in_choff;
            v.w = m->d_w.get() + o.w_off; v.bias = m->d_w.get() + o.b_off; v.oscale = m->d_w.get() + o.reserved;
            v.cin = o.cin; v.n16 = o.npad / 16;
            single = single && (o.flags & PA_CONV_W_SINGLE);
        }
    a.w_single = single ? 1 : 0;      // one form for the three convs: the three-product form is bitwise the two-product one on a zero m plane
}

bool head_fused(const pa_model* m) {
    const pa_engine* e = m->e;
    if (!e->t.fuse_head || m->d.dtype != PA_DTYPE_H2 || !m->tail.found || e->profiling || e->t.timeline || !m->planned) return false;
    HeadTailArgs a{};
    a.d.cs = m->bufs[m->d.head_buf[0]].channels; a.d.nc = m->d.nc; a.d.nk = m->d.nk;
    head_tail_convs(m, m->ln[0], a);          // (what it asks does not depend on the lane)
    return head_tail_h2_supported(a);
}

// the launcher of a step's kind with the step's arguments (a: its conv arguments, or the timeline's copy of them)
static hipError_t launch_step(const Step& st, const ConvArgs& a, hipStream_t s) {
    const SliceArgs& v = st.sl;
    switch (st.kind) {
        case PA_OP_CONV: return launch_conv_family(st.family, a, st.ran.tile, s);
        case PA_OP_STEM: return st.n_ops == 2 ? launch_stem_l1_h2(st.stem, a, nullptr, s) : launch_stem(st.stem, s);
        case PA_OP_SPPF_POOL: return launch_sppf_pool(v.in, v.in_cs, v.in_choff, v.c, v.B, v.H, v.W, s, v.fmt, v.fused);
        case PA_OP_UPSAMPLE2X: return launch_upsample2x(v.in, v.in_cs, v.in_choff, v.out, v.out_cs, v.out_choff, v.c, v.B, v.H, v.W, s, v.fmt);
        case PA_OP_MAXPOOL2: return launch_maxpool2(v.in, v.in_cs, v.in_choff, v.out, v.out_cs, v.out_choff, v.c, v.B, v.H, v.W, s, v.fmt);
        case PA_OP_MAXPOOL3S2: return launch_maxpool3s2(v.in, v.in_cs, v.in_choff, v.out, v.out_cs, v.out_choff, v.c, v.B, v.H, v.W, v.Ho, v.Wo, s, v.fmt);
        case PA_OP_STEM7: return launch_stem7(st.stem7, s);
        case PA_OP_GAP_FC: return launch_gap_fc(v.in, v.in_cs, v.in_choff, v.c, v.B, v.H, v.w, v.bias, v.nout, v.logits, v.probs, s, v.fmt);
        case PA_OP_DWCONV3: return launch_dwconv3(st.dw, s);
        case PA_OP_PSA_ATTN: return launch_psa_attn(st.attn, s);
    }
    return hipSuccess;
}

// tuning only ("timeline"): a conv step that runs the tile it asked for, with the s_memtime timeline of this launch collected into
// timeline_path.  The buffer is per launch: released where this returns, behind the wait
static hipError_t launch_conv_timeline(pa_model* m, const Step& st, hipStream_t s) {
    pa_engine* e = m->e;
    ConvArgs a = st.conv;
    const size_t patches = (size_t)(a.M / (a.Ho * a.Wo)) * ((a.Ho + 7) / 8) * ((a.Wo + 15) / 16);          // patch kernels: one record per workgroup of the 1-D grid
    const size_t records = st.path == CONV_PATH_H2 ? 8 * ((patches + 7) / 8) * (size_t)((a.n16 + 5) / 6)
                                                   : (size_t)((a.M + 63) / 64) * ((m->ops[st.op].npad + 95) / 96);
    const size_t dbg_bytes = records * conv_timeline_words(st.ran, a.ksize) * 8;          // 0: this kernel has no timeline instantiation
    DevMem<unsigned long long> dbg_dev;
    if (dbg_bytes && dbg_dev.alloc(dbg_bytes) == 0) (void)hipMemsetAsync(dbg_dev.get(), 0, dbg_bytes, s);
    a.dbg = dbg_dev.get();
    const hipError_t r = launch_step(st, a, s);
    if (dbg_dev) {
        (void)hipStreamSynchronize(s);
        std::vector<unsigned long long> host(dbg_bytes / 8);
        (void)hipMemcpy(host.data(), dbg_dev.get(), dbg_bytes, hipMemcpyDeviceToHost);
        if (FILE* f = fopen(e->timeline_path.c_str(), "wb")) { fwrite(host.data(), 1, dbg_bytes, f); fclose(f); }
    }
    return r;
}

// the tail convs alone, for the n images of the lane's last call: the same list, the steps marked `tail`
int run_tail_ops(pa_model* m, Lane& L, hipStream_t s, int n) {
    if (plan_steps(m, L, n)) return 1;
    for (const Step& st : L.steps) {
        if (!st.tail) continue;
        const hipError_t r = launch_step(st, st.conv, s);
        if (r != hipSuccess) PA_FAIL(m->e, "op %d (head tail) launch failed: %s", st.op, hipGetErrorString(r));
    }
    return 0;
}

// replay the op list for `n` images (prof records appended starting at *pi): decide every launch (launch_plan.cpp), then launch
static int run_ops(pa_model* m, Lane& L, hipStream_t s, int n, size_t* pi, bool skip_tail) {
    pa_engine* e = m->e;
    if (plan_steps(m, L, n)) return 1;
    // the 1x1 behind a fused stem + layer 1 inside that kernel (tuning fuse_stem_cv1, decided per step by build_steps): not while
    // profiling or collecting a timeline, which keep that conv's row
    const bool cv1_fused = !e->profiling && !e->t.timeline;
    m->last_stem_path = 0;
    for (const Step& st : L.steps) {
        if (skip_tail && st.tail) continue;          // the heads' last convs run inside the fused head tail (run_post)
        if (cv1_fused && st.stem_cv1) continue;      // ran inside the stem's kernel
        if (cv1_fused && st.kind == PA_OP_STEM && st.n_ops == 2 && st.has_cv1) {
            const hipError_t r = launch_stem_l1_h2(st.stem, st.conv, &st.cv1, s);
            if (r != hipSuccess) PA_FAIL(e, "fused stem + layer 1 + 1x1 launch failed: %s", hipGetErrorString(r));
            m->last_stem_path = 1;
            ++*pi;                                   // (its record stays unused: no profile is being taken)
            continue;
        }
        ProfRec* pr = prof_begin(m, s, (*pi)++, st.kind, st.ksize, st.flops);
        if (pr) {
            pr->M = st.M; pr->cout = st.cout; pr->cin = st.cin; pr->stride = st.stride; pr->mf = st.mf; pr->nf = st.nf; pr->res = st.res;
            pr->tile = st.ran.tile; pr->family = st.ran.family;
        }
        const bool timeline = st.kind == PA_OP_CONV && e->t.timeline && !e->timeline_path.empty() && st.ran.tile == st.requested;
        const hipError_t r = timeline ? launch_conv_timeline(m, st, s) : launch_step(st, st.conv, s);
        prof_end(s, pr);
        if (r != hipSuccess && st.n_ops == 2) PA_FAIL(e, "fused stem + layer 1 launch failed: %s", hipGetErrorString(r));
        if (r != hipSuccess) PA_FAIL(e, "op %d (kind %d) launch failed: %s", st.op, st.kind, hipGetErrorString(r));
    }
    return 0;
}

// the operand-order weight copies of conv_patch_h2r.hip and the stem operand block of stem_l1_h2.hip: allocated once, (re)built
// from the blob whenever it changed
static int ensure_operand_copies(pa_model* m) {
    if (m->wr_valid || m->d.dtype != PA_DTYPE_H2) return 0;
    pa_engine* e = m->e;
    // PA_CONV_W_SINGLE is the caller's promise that a conv's packed m plane is all zero; the two-product kernels skip the wm x ah
    // product on the strength of it.  Checked against the blob once per model (and again after a weight broadcast): a conv whose
    // promise does not hold fails the call instead of computing silently wrong results
    {
        bool any = false;
        PA_HIP(e, hipMemsetAsync(m->d_ovf.get() + 32, 0, sizeof(unsigned) * 8, e->main_stream()));        // scratch words of the 256-byte flag block
        for (size_t i = 0; i < m->ops.size(); ++i) {
            const pa_op_desc& o = m->ops[i];
            if (o.kind != PA_OP_CONV || !(o.flags & PA_CONV_W_SINGLE)) continue;
            PA_HIP(e, launch_h2_mplane_check(m->d_w.get() + o.w_off, (long long)o.npad * h2_ksteps(o.cin, o.ksize), m->d_ovf.get() + 32, e->main_stream()));
            any = true;
        }
        if (any) {
            unsigned bad = 0;
            PA_HIP(e, hipMemcpyAsync(&bad, m->d_ovf.get() + 32, sizeof(bad), hipMemcpyDeviceToHost, e->main_stream()));
            PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
            if (bad) PA_FAIL(e, "a conv flagged PA_CONV_W_SINGLE has a non-zero m plane in the weight blob (pack it without the flag, or with fp16-number weights)");
        }
    }
    if (m->wr_off.empty()) {
        std::vector<long long> off;
        const size_t total = operand_copy_offsets(m->d, m->stem_fuse, off);
        if (total) {
            PA_HIP(e, m->d_wr.fit(total + 8192, total + 8192));          // the last chunk's look-ahead reads run 4 KB past a fragment
            PA_HIP(e, hipMemsetAsync(m->d_wr.get() + total, 0, 8192, e->main_stream()));
        }
        m->wr_off = std::move(off);        // only once the allocation stands: a failed call leaves no offsets into a null d_wr
    }
    for (size_t i = 0; i < m->ops.size(); ++i) {
        if (m->wr_off[i] < 0) continue;
        const pa_op_desc& o = m->ops[i];
        if (o.kind == PA_OP_STEM) {
            PA_HIP(e, launch_stem_l1_operands(m->d_w.get() + o.w_off, o.cout, m->d_wr.get() + m->wr_off[i], e->main_stream()));
            continue;
        }
        PA_HIP(e, launch_h2r_repack(m->d_w.get() + o.w_off, m->d_wr.get() + m->wr_off[i], o.npad / 16, o.cin, o.ksize, e->main_stream()));
    }
    // (built on the main stream, read on the lanes: the lanes do not fork for it, the host waits once per model instead)
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    m->wr_valid = true;
    return 0;
}

// run_ops, or (tuning "graph", not while profiling) the replay of its capture for this batch size: the op list of
// an n-scale graph is ~100 launches of 10-40 us each, where per-launch host work shows.  A captured graph bakes the skip_tail of
// its capture.  That is sound: skip_tail is the caller's head_fused, which for a planned model changes only with tuning fuse_head
// (every pa_engine_set_tuning bumps the epoch, and the graphs of an older epoch are destroyed below) or with profiling / timeline,
// under which no graph is replayed.
int run_graph(pa_model* m, Lane& L, hipStream_t s, int n, size_t* pi, bool skip_tail) {
    pa_engine* e = m->e;
    if (ensure_operand_copies(m)) return 1;
    if (!e->t.graph || e->profiling || e->t.timeline) return run_ops(m, L, s, n, pi, skip_tail);
    if (m->graph_epoch != e->tuning_epoch) {            // kernel choice may have changed since the capture
        PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
        PA_HIP(e, e->sync_lanes());
        destroy_graphs(m);
        m->graph_epoch = e->tuning_epoch;
    }
    auto it = L.graphs.find(n);
    if (it == L.graphs.end()) {
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        PA_HIP(e, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        size_t dummy = 0;
        const int rc = run_ops(m, L, s, n, &dummy, skip_tail);
        const hipError_t r = hipStreamEndCapture(s, &g);
        if (rc) { if (g) hipGraphDestroy(g); return 1; }
        if (r != hipSuccess) PA_FAIL(e, "hipStreamEndCapture: %s", hipGetErrorString(r));
        const hipError_t ri = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (ri != hipSuccess) PA_FAIL(e, "hipGraphInstantiate: %s", hipGetErrorString(ri));
        it = L.graphs.emplace(n, ge).first;
        L.graph_stem_path[n] = m->last_stem_path;          // what the capture launched is what every replay of it launches
    }
    PA_HIP(e, hipGraphLaunch(it->second, s));
    m->last_stem_path = L.graph_stem_path[n];
    return 0;
}

int finish_profile(pa_model* m, size_t n_rec) {
    if (!m->e->profiling) { m->n_prof = 0; return 0; }
    for (size_t i = 0; i < n_rec && i < m->prof.size(); ++i)
        hipEventElapsedTime(&m->prof[i].ms, m->prof[i].e0, m->prof[i].e1);
    m->n_prof = n_rec;
    return 0;
}

int pa_model_plan_bytes(pa_model* m, size_t* arena_bytes, size_t* logical_bytes) {
    if (!m->planned) PA_FAIL(m->e, "pa_model_plan_bytes: no plan yet");
    if (arena_bytes) *arena_bytes = m->arena_bytes;
    if (logical_bytes) *logical_bytes = m->logical_bytes;
    return 0;
}

int pa_model_fill_arena(pa_model* m, int byte_value) {
    if (!m) return 1;
    pa_engine* e = m->e;
    if (!m->planned || !m->ln[0].arena) PA_FAIL(e, "pa_model_fill_arena: no plan yet");
    PA_HIP(e, hipSetDevice(e->dev));
    for (Lane& L : m->ln) {          // every lane the model has, each on the stream its batches run on
        if (!L.allocated) continue;
        const hipStream_t s = L.stream ? L.stream : e->main_stream();
        PA_HIP(e, hipMemsetAsync(L.arena.get(), byte_value & 0xFF, m->arena_bytes, s));
        // (the u8 network input as well: the preprocessing of the next call writes all four bytes of every pixel)
        if (L.d_netin) PA_HIP(e, hipMemsetAsync(L.d_netin.get(), byte_value & 0xFF, (size_t)m->p_batch * m->net_h * m->net_w * 4, s));
        PA_HIP(e, hipStreamSynchronize(s));
    }
    return 0;
}

int pa_model_lanes_allocated(pa_model* m) {
    int n = 0;
    if (m) for (const Lane& L : m->ln) n += L.allocated ? 1 : 0;
    return n;
}

int pa_model_last_lane(pa_model* m) { return m ? m->last_lane : 0; }

int pa_model_last_stem_path(pa_model* m) { return m ? m->last_stem_path : 0; }

int pa_model_profile_text(pa_model* m, char* buf, size_t cap) {
    size_t off = 0;
    for (size_t i = 0; i < m->n_prof && i < m->prof.size(); ++i) {
        const ProfRec& r = m->prof[i];
        int n = snprintf(buf + off, off < cap ? cap - off : 0, "%d,%d,%d,%d,%d,%d,%d,%d,%.5f,%.0f,%d,%d,%s\n", r.kind, r.ksize, r.M, r.cout,
                         r.cin, r.stride, r.mf, r.nf, r.ms, r.flops, r.res, r.tile, r.family ? r.family : "");
        if (n < 0 || off + n >= cap) break;
        off += n;
    }
    if (off < cap) buf[off] = 0;
    return (int)off;
}

int pa_model_last_profile(pa_model* m, int cap, int32_t* kinds, float* ms, double* flops, int32_t* ksizes) {
    int n = 0;
    for (size_t i = 0; i < m->n_prof && i < m->prof.size() && n < cap; ++i, ++n) {
        kinds[n] = m->prof[i].kind; ms[n] = m->prof[i].ms; flops[n] = m->prof[i].flops; ksizes[n] = m->prof[i].ksize;
    }
    return n;
}
