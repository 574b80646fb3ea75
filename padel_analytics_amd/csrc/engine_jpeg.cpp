// pa_jpeg_encode: YUV 4:2:0 frames in HBM -> one baseline JPEG per frame, back to back in host memory (jpeg_encode.hip).  What is
// refused, the tables, the header and the sizes are host-only code in jpeg_check.cpp.
#include "engine_internal.h"
#include "jpeg_check.h"

// Scratch of the call in flight, grown on demand, freed with the engine; filled and read on the compute stream only.
struct JpegScratch {
    DevMem<uint8_t> slots;                // [frames of a sub-batch][MCU rows] slots
    DevMem<int32_t> lens;                 // one per interval of a sub-batch
    DevMem<long long> offs;               // frame_off[257], then ivl_off[as many as lens]
    DevMem<uint8_t> out;                  // the frames of the call, gathered
    DevMem<JpegDevTables> tab;
};

// the slots of one sub-batch stay under this many bytes (one frame's slots where a single frame needs more)
static const size_t kSlotBudget = (size_t)256 << 20;

void jpeg_scratch_free(pa_engine* e) {
    if (!e->jpeg) return;
    if (e->main_stream_wait_only()) hipStreamSynchronize(e->main_stream_wait_only());
    delete e->jpeg;
    e->jpeg = nullptr;
}

int pa_jpeg_encode(pa_engine* e, const uint8_t* src, int n, int h, int w, const pa_yuv_desc* geom, int quality, uint8_t* dst_host, size_t cap,
                   int64_t* offsets_host) {
    if (!e) return 1;
    if (!src || !offsets_host) PA_FAIL(e, "pa_jpeg_encode: src or offsets_host is NULL");
    if (!dst_host && cap) PA_FAIL(e, "pa_jpeg_encode: dst_host is NULL");
    size_t span = 0;
    std::string why;
    if (jpeg_validate(n, h, w, geom, quality, &span, why)) PA_FAIL(e, "%s", why.c_str());
    PA_HIP(e, hipSetDevice(e->dev));
    if (!e->jpeg) e->jpeg = new JpegScratch();
    JpegScratch* s = e->jpeg;
    const int mcus = jpeg::mcus_per_row(w), rows = jpeg::mcu_rows(h);
    const size_t slot_cap = (jpeg::interval_max_bytes(w) + 15) & ~(size_t)15;
    const size_t per_frame = slot_cap * rows;
    const int sub = (int)std::max<size_t>(1, std::min<size_t>(std::min(n, 256), kSlotBudget / per_frame));
    const size_t ivls = (size_t)sub * rows;
    const size_t lens_bytes = ivls * sizeof(int32_t), offs_bytes = (257 + ivls) * sizeof(long long);
    if (s->slots.bytes() < per_frame * sub || s->lens.bytes() < lens_bytes || s->offs.bytes() < offs_bytes || !s->tab) {
        PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));              // an encode still queued uses what is about to go
        PA_HIP(e, s->slots.fit(per_frame * sub, per_frame * sub));
        PA_HIP(e, s->lens.fit(lens_bytes, lens_bytes));
        PA_HIP(e, s->offs.fit(offs_bytes, offs_bytes));
        PA_HIP(e, s->tab.fit(sizeof(JpegDevTables), sizeof(JpegDevTables)));
    }
    JpegDevTables tab;
    jpeg_fill_tables(h, w, quality, &tab);
    // (pageable source: the runtime has consumed it when hipMemcpyAsync returns; an earlier call's kernels are ahead of it in the stream)
    PA_HIP(e, hipMemcpyAsync(s->tab.get(), &tab, sizeof(tab), hipMemcpyHostToDevice, e->main_stream()));

    std::vector<int64_t> offsets((size_t)n + 1, 0);
    std::vector<long long> frame_off(257);
    size_t total = 0;
    for (int f0 = 0; f0 < n; f0 += sub) {
        const int nf = std::min(sub, n - f0);
        JpegEncArgs a{};
        a.src = src + (size_t)f0 * (size_t)geom->frame_stride; a.tab = s->tab.get(); a.slots = s->slots.get(); a.lens = s->lens.get();
        a.n = nf; a.h = h; a.w = w; a.mcus = mcus; a.rows = rows; a.nv12 = geom->layout == PA_YUV_NV12;
        a.pitch_y = geom->pitch_y; a.pitch_c = geom->pitch_c; a.off_u = geom->off_u; a.off_v = geom->off_v;
        a.frame_stride = geom->frame_stride; a.slot_cap = slot_cap;
        hipError_t r = launch_jpeg_encode(a, e->main_stream());
        if (r != hipSuccess) PA_FAIL(e, "jpeg encode launch failed: %s", hipGetErrorString(r));
        long long* d_frame_off = s->offs.get();
        long long* d_ivl_off = s->offs.get() + 257;
        r = launch_jpeg_offsets(s->lens.get(), nf, rows, d_frame_off, d_ivl_off, e->main_stream());
        if (r != hipSuccess) PA_FAIL(e, "jpeg offsets launch failed: %s", hipGetErrorString(r));
        // the sizes come back before the gather: `out` is then known to hold this sub-batch (no size is guessed)
        PA_HIP(e, hipMemcpyAsync(frame_off.data(), d_frame_off, (size_t)(nf + 1) * sizeof(long long), hipMemcpyDeviceToHost, e->main_stream()));
        PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
        const size_t bytes = (size_t)frame_off[nf];
        // (the stream is idle after the wait above: the gathered frames so far move into the larger buffer with a blocking copy)
        PA_HIP(e, s->out.fit_keep(total + bytes, std::max((total + bytes) * 2, (size_t)1 << 20), total,
                                  [](void* to, const void* from, size_t nb) { return (int)hipMemcpy(to, from, nb, hipMemcpyDeviceToDevice); }));
        r = launch_jpeg_gather(s->slots.get(), slot_cap, s->lens.get(), d_frame_off, d_ivl_off, s->tab.get(), s->out.get() + total, nf, rows, e->main_stream());
        if (r != hipSuccess) PA_FAIL(e, "jpeg gather launch failed: %s", hipGetErrorString(r));
        for (int i = 0; i <= nf; ++i) offsets[(size_t)f0 + i] = (int64_t)(total + (size_t)frame_off[i]);
        total += bytes;
    }
    if (total > cap) {
        PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
        offsets_host[0] = 0;
        offsets_host[n] = (int64_t)total;
        PA_FAIL(e, "pa_jpeg_encode: the %d frames take %zu bytes, dst_host holds %zu", n, total, cap);
    }
    PA_HIP(e, hipMemcpyAsync(dst_host, s->out.get(), total, hipMemcpyDeviceToHost, e->main_stream()));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    memcpy(offsets_host, offsets.data(), ((size_t)n + 1) * sizeof(int64_t));
    return 0;
}
