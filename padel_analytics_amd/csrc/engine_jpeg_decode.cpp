// pa_jpeg_decode: baseline JPEGs in host memory -> packed BGR frames in HBM (jpeg_decode.hip).  The markers are read by host-only
// code (jpeg_parse.cpp); what reaches the device is the compressed bytes as they are, one table block per frame and the interval table.
#include "engine_internal.h"
#include "jpeg_decode.h"
#include "jpeg_parse.h"

#include <chrono>

// Scratch of the call in flight, grown on demand, freed with the engine; filled and read on the compute stream only.
struct JpegDecScratch {
    DevMem<uint8_t> data;                                        // compressed bytes of a sub-batch
    DevMem<JpegDecFrame> frames;
    DevMem<JpegDecInterval> ivls;
    DevMem<int32_t> status;                                      // per interval one status word, then one word of rounds
    DevMem<int32_t> order;                                       // the intervals of the serial kernel, then those of the split kernel
    DevMem<int16_t> coef;
    DevMem<uint8_t> planes;
    hipEvent_t ev[5]{};                                          // profiling: in front of the upload, of (a), (b), (c), behind (c)
    double ms[5]{};                                              // of the last call while profiling: parse (host clock), upload, (a), (b), (c)
};

// coefficients and planes of one sub-batch stay under this many bytes (one frame's where a single frame needs more), and a sub-batch
// has at most this many frames
static const size_t kDecBudget = (size_t)256 << 20;
static const int kDecMaxSub = 64;

void jpeg_dec_scratch_free(pa_engine* e) {
    if (!e->jpeg_dec) return;
    if (e->main_stream_wait_only()) hipStreamSynchronize(e->main_stream_wait_only());
    for (hipEvent_t ev : e->jpeg_dec->ev) if (ev) hipEventDestroy(ev);
    delete e->jpeg_dec;
    e->jpeg_dec = nullptr;
}

int pa_jpeg_decode(pa_engine* e, const uint8_t* jpegs, const int64_t* offsets, int n, int h, int w, uint8_t* dst, int32_t* status_host) {
    if (!e) return 1;
    if (!jpegs || !offsets || !dst || !status_host) PA_FAIL(e, "pa_jpeg_decode: jpegs_host, offsets, dst_bgr_dev or status_host is NULL");
    if (n < 1) PA_FAIL(e, "pa_jpeg_decode: n = %d frames", n);
    if (w < 1 || h < 1 || w > PA_JPEG_DEC_MAX_DIM || h > PA_JPEG_DEC_MAX_DIM)
        PA_FAIL(e, "pa_jpeg_decode: %d x %d frames outside 1 .. %d pixels a side", w, h, PA_JPEG_DEC_MAX_DIM);
    for (int i = 0; i < n; ++i)
        if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) PA_FAIL(e, "pa_jpeg_decode: offsets[%d .. %d] = %lld, %lld do not ascend", i, i + 1, (long long)offsets[i], (long long)offsets[i + 1]);
    // every frame is parsed before anything is launched: a refusal leaves dst untouched
    std::vector<pa_jpeg_frame_info> infos((size_t)n);
    std::vector<std::vector<pa_jpeg_interval>> tables((size_t)n);
    std::string why;
    const auto parse_t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n; ++i) {
        if (jpeg_parse_frame(jpegs + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), &infos[(size_t)i], tables[(size_t)i], why))
            PA_FAIL(e, "pa_jpeg_decode: frame %d: %s", i, why.c_str());
        if (infos[(size_t)i].w != w || infos[(size_t)i].h != h)
            PA_FAIL(e, "pa_jpeg_decode: frame %d is %d x %d, the call says %d x %d: frame sizes differ within the clip", i, infos[(size_t)i].w, infos[(size_t)i].h, w, h);
    }
    const double parse_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - parse_t0).count();
    PA_HIP(e, hipSetDevice(e->dev));
    if (!e->jpeg_dec) e->jpeg_dec = new JpegDecScratch();
    JpegDecScratch* s = e->jpeg_dec;
    const bool timed = e->profiling;
    if (timed) {
        for (hipEvent_t& ev : s->ev)
            if (!ev) PA_HIP(e, hipEventCreate(&ev));
        for (double& v : s->ms) v = 0;
        s->ms[0] = parse_ms;
    }
    const int mcus_x = jpeg::mcus_per_row(w), mcus_y = jpeg::mcu_rows(h);
    const size_t mcus = (size_t)mcus_x * mcus_y;
    const size_t coef_frame = mcus * jpeg::kBlocksPerMcu * 64 * sizeof(int16_t), planes_frame = mcus * 384;
    const int sub = (int)std::max<size_t>(1, std::min<size_t>(std::min(n, kDecMaxSub), kDecBudget / (coef_frame + planes_frame)));

    std::vector<JpegDecFrame> frames;
    std::vector<JpegDecInterval> ivls;
    std::vector<int32_t> ivl_status, order, split;
    const long long split_min = e->jpeg_dec_split_min == 0 ? PA_JPEG_DEC_SPLIT_MIN_BYTES : e->jpeg_dec_split_min;      // < 0: never
    const int split_sub = e->jpeg_dec_split_sub == 0 ? PA_JPEG_DEC_SPLIT_SUB_BYTES : e->jpeg_dec_split_sub;
    long long last_split[4] = {0, 0, 0, 0};
    for (int f0 = 0; f0 < n; f0 += sub) {
        const int nf = std::min(sub, n - f0);
        const int64_t base = offsets[f0];
        const size_t bytes = (size_t)(offsets[f0 + nf] - base);
        frames.assign((size_t)nf, JpegDecFrame{});
        ivls.clear();
        for (int i = 0; i < nf; ++i) {
            const pa_jpeg_frame_info& in = infos[(size_t)(f0 + i)];
            JpegDecFrame& fr = frames[(size_t)i];
            for (int t = 0; t < 2; ++t) {
                jpeg::huff_dec_build(in.dc[t].bits, in.dc[t].vals, in.dc[t].nvals, &fr.dc[t]);
                jpeg::huff_dec_build(in.ac[t].bits, in.ac[t].vals, in.ac[t].nvals, &fr.ac[t]);
            }
            for (int c = 0; c < 3; ++c) {
                for (int k = 0; k < 64; ++k) fr.quant[c][k] = in.quant[c][k];
                fr.comp_dc[c] = in.comp_dc[c];
                fr.comp_ac[c] = in.comp_ac[c];
            }
            const int64_t at = offsets[f0 + i] - base;
            for (const pa_jpeg_interval& v : tables[(size_t)(f0 + i)])
                ivls.push_back({(long long)(at + v.begin), (long long)(at + v.end), i, v.first_mcu, v.mcus, 0});
        }
        const size_t need_f = frames.size() * sizeof(JpegDecFrame), need_i = ivls.size() * sizeof(JpegDecInterval);
        // which kernel decodes an interval: its length decides (an empty one has nothing to split)
        order.clear();
        split.clear();
        int most_sub = 1;
        for (size_t k = 0; k < ivls.size(); ++k) {
            const long long len = ivls[k].end - ivls[k].begin;
            if (split_min >= 0 && len > 0 && len >= split_min && ivls[k].mcus > 0) {
                split.push_back((int32_t)k);
                const uint32_t l = jpeg::split_len(ivls[k].begin, ivls[k].end);
                const int subs = jpeg::split_count(l, jpeg::split_sub_bytes(l, split_sub));
                most_sub = std::max(most_sub, subs);
                last_split[1] += subs;
            } else {
                order.push_back((int32_t)k);
            }
        }
        const int n_serial = (int)order.size(), n_split = (int)split.size();
        order.insert(order.end(), split.begin(), split.end());
        last_split[0] += n_split;
        last_split[3] += n_serial;
        const size_t need_s = 2 * ivls.size() * sizeof(int32_t), need_o = ivls.size() * sizeof(int32_t);
        if (s->data.bytes() < bytes + 16 || s->frames.bytes() < need_f || s->ivls.bytes() < need_i || s->status.bytes() < need_s ||
            s->order.bytes() < need_o || s->coef.bytes() < coef_frame * nf || s->planes.bytes() < planes_frame * nf) {
            PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));          // a decode still queued uses what is about to go
            const auto roomy = [](size_t need) { return need + need / 4; };       // what a buffer that has to grow is given
            PA_HIP(e, s->data.fit(bytes + 16, roomy(bytes + 16)));
            PA_HIP(e, s->frames.fit(need_f, roomy(need_f)));
            PA_HIP(e, s->ivls.fit(need_i, roomy(need_i)));
            PA_HIP(e, s->status.fit(need_s, roomy(need_s)));
            PA_HIP(e, s->order.fit(need_o, roomy(need_o)));
            PA_HIP(e, s->coef.fit(coef_frame * nf, roomy(coef_frame * nf)));
            PA_HIP(e, s->planes.fit(planes_frame * nf, roomy(planes_frame * nf)));
        }
        // (pageable sources: the runtime has consumed them when hipMemcpyAsync returns; an earlier sub-batch's kernels are ahead in the stream)
        if (timed) PA_HIP(e, hipEventRecord(s->ev[0], e->main_stream()));
        if (bytes) PA_HIP(e, hipMemcpyAsync(s->data.get(), jpegs + base, bytes, hipMemcpyHostToDevice, e->main_stream()));
        PA_HIP(e, hipMemcpyAsync(s->frames.get(), frames.data(), need_f, hipMemcpyHostToDevice, e->main_stream()));
        PA_HIP(e, hipMemcpyAsync(s->ivls.get(), ivls.data(), need_i, hipMemcpyHostToDevice, e->main_stream()));
        PA_HIP(e, hipMemcpyAsync(s->order.get(), order.data(), need_o, hipMemcpyHostToDevice, e->main_stream()));
        JpegDecArgs a{};
        a.data = s->data.get(); a.ivls = s->ivls.get(); a.frames = s->frames.get(); a.coef = s->coef.get(); a.ivl_status = s->status.get(); a.planes = s->planes.get();
        a.dst = dst + (size_t)f0 * h * w * 3;
        a.n = nf; a.n_ivls = (int)ivls.size(); a.h = h; a.w = w; a.mcus_x = mcus_x; a.mcus_y = mcus_y;
        a.order = s->order.get(); a.n_serial = n_serial; a.n_split = n_split; a.sub_bytes = split_sub;
        a.split_threads = std::min(kSplitMaxThreads, (most_sub + 63) / 64 * 64);
        int path = 0;
        const hipError_t r = launch_jpeg_decode(a, &path, e->main_stream(), timed ? s->ev + 1 : nullptr);
        if (r != hipSuccess) PA_FAIL(e, "jpeg decode launch failed: %s", hipGetErrorString(r));
        e->jpeg_dec_last_path = path;
        ivl_status.resize(2 * ivls.size());
        PA_HIP(e, hipMemcpyAsync(ivl_status.data(), s->status.get(), need_s, hipMemcpyDeviceToHost, e->main_stream()));
        PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
        if (timed)
            for (int k = 0; k < 4; ++k) {
                float ms = 0;
                PA_HIP(e, hipEventElapsedTime(&ms, s->ev[k], s->ev[k + 1]));
                s->ms[k + 1] += ms;
            }
        for (int i = 0; i < nf; ++i) status_host[f0 + i] = infos[(size_t)(f0 + i)].status;
        for (size_t k = 0; k < ivls.size(); ++k) status_host[f0 + ivls[k].frame] |= ivl_status[k];
        for (int k = n_serial; k < n_serial + n_split; ++k)
            last_split[2] = std::max<long long>(last_split[2], ivl_status[ivls.size() + (size_t)order[(size_t)k]]);
    }
    for (int k = 0; k < 4; ++k) e->jpeg_dec_last_split[k] = last_split[k];
    return 0;
}

int pa_jpeg_decode_set_split(pa_engine* e, int64_t min_bytes, int32_t sub_bytes) {
    if (min_bytes < -1) PA_FAIL(e, "pa_jpeg_decode_set_split: min_bytes = %lld: 0 (the default), -1 (never split) or a length in bytes", (long long)min_bytes);
    if (sub_bytes != 0 && (sub_bytes < jpeg::kSplitMinSubBytes || sub_bytes > jpeg::kSplitMaxSubBytes))
        PA_FAIL(e, "pa_jpeg_decode_set_split: sub_bytes = %d outside %d .. %d (0: the default)", (int)sub_bytes, jpeg::kSplitMinSubBytes, jpeg::kSplitMaxSubBytes);
    if (sub_bytes % 4) PA_FAIL(e, "pa_jpeg_decode_set_split: sub_bytes = %d is not a multiple of 4", (int)sub_bytes);
    if (!e) PA_FAIL(e, "pa_jpeg_decode_set_split: the engine is NULL");
    e->jpeg_dec_split_min = min_bytes;
    e->jpeg_dec_split_sub = sub_bytes;
    return 0;
}

int pa_jpeg_decode_last_split(pa_engine* e, int64_t out[4]) {
    if (!out) PA_FAIL(e, "pa_jpeg_decode_last_split: out is NULL");
    if (!e) PA_FAIL(e, "pa_jpeg_decode_last_split: the engine is NULL");
    for (int k = 0; k < 4; ++k) out[k] = e->jpeg_dec_last_split[k];
    return 0;
}

int pa_jpeg_decode_last_path(pa_engine* e) { return e ? e->jpeg_dec_last_path : 0; }

int pa_jpeg_decode_last_times(pa_engine* e, double ms[5]) {
    if (!e) return 1;
    if (!e->jpeg_dec || !ms) PA_FAIL(e, "pa_jpeg_decode_last_times: no pa_jpeg_decode has run on this engine");
    for (int k = 0; k < 5; ++k) ms[k] = e->jpeg_dec->ms[k];
    return 0;
}
