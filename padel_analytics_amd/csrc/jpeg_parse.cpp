// The markers of one baseline JPEG -> pa_jpeg_frame_info and its restart-interval table: host-only code (no HIP), built with g++
// like jpeg_check.cpp.  mjpeg.parse_frame is its twin; include/padel_hip.h (pa_jpeg_decode) says what is accepted.
#include "jpeg_parse.h"

#include "jpeg_entropy.h"
#include "jpeg_tables.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace padel {

static_assert(jpeg::kMaxFrameBytes == PA_JPEG_DEC_MAX_BYTES, "the size limit is stated twice");

#define FAIL(...)                                                \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        err = _b;                                                \
        return 1;                                                \
    } while (0)

static void set_huff(pa_jpeg_huff* t, const jpeg::HuffSpec& s) {
    memset(t, 0, sizeof(*t));
    memcpy(t->bits, s.bits, 16);
    memcpy(t->vals, s.vals, (size_t)s.nvals);
    t->nvals = s.nvals;
}

int jpeg_parse_frame(const uint8_t* p, size_t len, pa_jpeg_frame_info* info, std::vector<pa_jpeg_interval>& ivls, std::string& err) {
    memset(info, 0, sizeof(*info));
    ivls.clear();
    if (!p || len < 4 || p[0] != 0xff || p[1] != 0xd8) FAIL("jpeg: no SOI marker at the start (%zu bytes)", len);
    if (len > (size_t)PA_JPEG_DEC_MAX_BYTES) FAIL("jpeg: a frame of %zu bytes is beyond the %d the decoder counts bits for", len, PA_JPEG_DEC_MAX_BYTES);
    uint8_t qt[4][64];
    bool have_q[4] = {false, false, false, false}, have_h[2][2] = {{false, false}, {false, false}};
    bool any_dht = false, have_sof = false;
    int comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > len) FAIL("jpeg: truncated header: the bytes end at %zu, before any scan", len);
        if (p[pos] != 0xff) FAIL("jpeg: truncated header: byte %zu is 0x%02x where a marker belongs", pos, p[pos]);
        const int m = p[pos + 1];
        if (m == 0xff) { ++pos; continue; }                      // fill byte
        if (m == 0x01 || (m >= 0xd0 && m <= 0xd8)) { pos += 2; continue; }   // markers without a segment
        if (m == 0xd9) FAIL("jpeg: EOI at byte %zu, before any scan", pos);
        if (pos + 4 > len) FAIL("jpeg: truncated header: the bytes end inside the segment of marker FF%02X", m);
        const size_t L = (size_t)p[pos + 2] << 8 | p[pos + 3];
        if (L < 2 || pos + 2 + L > len) FAIL("jpeg: truncated header: the segment of marker FF%02X at byte %zu claims %zu bytes, %zu remain", m, pos, L, len - pos - 2);
        const uint8_t* s = p + pos + 4;
        const size_t n = L - 2;
        if (m == 0xc2 || m == 0xc6) FAIL("jpeg: progressive frame (SOF%d): baseline sequential only", m - 0xc0);
        if (m == 0xc1 || m == 0xc5) FAIL("jpeg: extended sequential frame (SOF%d): baseline sequential only", m - 0xc0);
        if (m == 0xc3 || m == 0xc7) FAIL("jpeg: lossless frame (SOF%d): baseline sequential only", m - 0xc0);
        if (m == 0xcc || (m >= 0xc9 && m <= 0xcf)) FAIL("jpeg: arithmetic coding (marker FF%02X): Huffman coding only", m);
        if (m == 0xc0) {
            if (have_sof) FAIL("jpeg: a second SOF0 at byte %zu: one frame per JPEG", pos);
            if (n < 6) FAIL("jpeg: truncated header: SOF0 of %zu bytes", n);
            if (s[0] != 8) FAIL("jpeg: %d-bit samples: 8-bit data only", s[0]);
            const int h = s[1] << 8 | s[2], w = s[3] << 8 | s[4], nf = s[5];
            if (nf != 3) FAIL("jpeg: %d component(s): three (Y, Cb, Cr) are needed", nf);
            if (n < 6 + 9) FAIL("jpeg: truncated header: SOF0 of %zu bytes for 3 components", n);
            if (w < 1 || h < 1 || w > PA_JPEG_DEC_MAX_DIM || h > PA_JPEG_DEC_MAX_DIM)
                FAIL("jpeg: %d x %d frame outside 1 .. %d pixels a side", w, h, PA_JPEG_DEC_MAX_DIM);
            for (int c = 0; c < 3; ++c) {
                comp_id[c] = s[6 + 3 * c];
                const int hv = s[7 + 3 * c];
                comp_tq[c] = s[8 + 3 * c];
                if (hv != (c == 0 ? 0x22 : 0x11))
                    FAIL("jpeg: sampling %dx%d of component %d: 4:2:0 only (Y 2x2, Cb and Cr 1x1)", hv >> 4, hv & 15, c);
                if (comp_tq[c] > 3) FAIL("jpeg: component %d names quantisation table %d", c, comp_tq[c]);
            }
            info->w = w; info->h = h;
            info->mcus_x = jpeg::mcus_per_row(w); info->mcus_y = jpeg::mcu_rows(h);
            have_sof = true;
        } else if (m == 0xdb) {
            for (size_t i = 0; i < n;) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (pq != 0) FAIL("jpeg: 16-bit quantisation table %d: 8-bit DQT only", tq);
                if (tq > 3) FAIL("jpeg: DQT defines table %d", tq);
                if (i + 65 > n) FAIL("jpeg: truncated header: DQT ends inside table %d", tq);
                memcpy(qt[tq], s + i + 1, 64);
                have_q[tq] = true;
                i += 65;
            }
        } else if (m == 0xc4) {
            for (size_t i = 0; i < n;) {
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 1) FAIL("jpeg: DHT defines table class %d id %d: baseline has DC / AC tables 0 and 1", tc, th);
                if (i + 17 > n) FAIL("jpeg: truncated header: DHT ends inside table %d/%d", tc, th);
                int total = 0;
                unsigned code = 0;
                for (int l = 1; l <= 16; ++l) {
                    total += s[i + l];
                    code += s[i + l];
                    if (code > (1u << l)) FAIL("jpeg: DHT table %d/%d has more codes of length %d than fit", tc, th, l);
                    code <<= 1;
                }
                if (total > 256) FAIL("jpeg: DHT table %d/%d lists %d symbols", tc, th, total);
                if (i + 17 + (size_t)total > n) FAIL("jpeg: truncated header: DHT ends inside the symbols of table %d/%d", tc, th);
                pa_jpeg_huff* t = tc ? &info->ac[th] : &info->dc[th];
                memset(t, 0, sizeof(*t));
                memcpy(t->bits, s + i + 1, 16);
                memcpy(t->vals, s + i + 17, (size_t)total);
                t->nvals = total;
                have_h[tc][th] = true;
                any_dht = true;
                i += 17 + (size_t)total;
            }
        } else if (m == 0xdd) {
            if (n != 2) FAIL("jpeg: truncated header: DRI of %zu bytes", n);
            info->restart_interval = s[0] << 8 | s[1];
        } else if (m == 0xda) {
            if (!have_sof) FAIL("jpeg: SOS at byte %zu before any SOF0", pos);
            if (n < 1) FAIL("jpeg: truncated header: empty SOS");
            const int ns = s[0];
            if (ns != 3) FAIL("jpeg: a scan of %d component(s): more than one scan is not supported (one interleaved scan of all three)", ns);
            if (n != 1 + 2 * 3 + 3) FAIL("jpeg: truncated header: SOS of %zu bytes for 3 components", n);
            for (int c = 0; c < 3; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) FAIL("jpeg: the scan lists component id %d where the frame has %d", s[1 + 2 * c], comp_id[c]);
                const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 1 || ta > 1) FAIL("jpeg: component %d names Huffman tables %d / %d: baseline has 0 and 1", c, td, ta);
                info->comp_dc[c] = (uint8_t)td;
                info->comp_ac[c] = (uint8_t)ta;
            }
            if (s[7] != 0 || s[8] != 63 || s[9] != 0)
                FAIL("jpeg: scan with Ss %d, Se %d, Ah/Al 0x%02x: one sequential scan (0, 63, 0) only", s[7], s[8], s[9]);
            pos += 2 + L;
            break;
        }
        pos += 2 + L;
    }
    for (int c = 0; c < 3; ++c) {
        if (!have_q[comp_tq[c]]) FAIL("jpeg: missing table: component %d names quantisation table %d, which no DQT defined", c, comp_tq[c]);
        memcpy(info->quant[c], qt[comp_tq[c]], 64);
    }
    if (!any_dht) {                                              // AVI 'MJPG': the Annex K tables are implied
        info->default_huffman = 1;
        set_huff(&info->dc[0], jpeg::kDcLumaSpec); set_huff(&info->dc[1], jpeg::kDcChromaSpec);
        set_huff(&info->ac[0], jpeg::kAcLumaSpec); set_huff(&info->ac[1], jpeg::kAcChromaSpec);
    } else {
        for (int c = 0; c < 3; ++c) {
            if (!have_h[0][info->comp_dc[c]]) FAIL("jpeg: missing table: component %d names DC Huffman table %d, which no DHT defined", c, info->comp_dc[c]);
            if (!have_h[1][info->comp_ac[c]]) FAIL("jpeg: missing table: component %d names AC Huffman table %d, which no DHT defined", c, info->comp_ac[c]);
        }
    }
    // the entropy-coded data: split at RSTm, ended by any other marker (or by the end of the bytes)
    std::vector<pa_jpeg_interval> segs;
    size_t i = pos, seg = pos;
    while (i < len) {
        if (p[i] != 0xff) { ++i; continue; }
        if (i + 1 >= len) { i = len; break; }                    // a lone FF: the reader ends the data there
        const int m = p[i + 1];
        if (m == 0) i += 2;
        else if (m == 0xff) ++i;
        else if (m >= 0xd0 && m <= 0xd7) {
            segs.push_back({(int64_t)seg, (int64_t)i, 0, 0});
            i += 2;
            seg = i;
        } else break;
    }
    segs.push_back({(int64_t)seg, (int64_t)i, 0, 0});
    info->scan_begin = (int64_t)pos;
    info->scan_end = (int64_t)i;
    // what follows the scan: segments up to EOI; another scan is refused
    for (size_t j = i; j + 4 <= len && p[j] == 0xff;) {
        const int m = p[j + 1];
        if (m == 0xd9) break;
        if (m == 0xda) FAIL("jpeg: a second SOS at byte %zu: more than one scan is not supported", j);
        if (m == 0xff) { ++j; continue; }
        j += 2 + ((size_t)p[j + 2] << 8 | p[j + 3]);
    }
    const long long total = (long long)info->mcus_x * info->mcus_y;
    const long long ri = info->restart_interval ? info->restart_interval : total;
    const long long expect = (total + ri - 1) / ri;
    info->n_intervals = (int32_t)expect;
    if ((long long)segs.size() != expect) info->status |= PA_JPEG_ST_MARKERS;
    ivls.resize((size_t)expect);
    for (long long k = 0; k < expect; ++k) {
        pa_jpeg_interval v = (size_t)k < segs.size() ? segs[(size_t)k] : pa_jpeg_interval{(int64_t)i, (int64_t)i, 0, 0};
        v.first_mcu = (int32_t)(k * ri);
        v.mcus = (int32_t)std::min<long long>(ri, total - k * ri);
        ivls[(size_t)k] = v;
    }
    return 0;
}

}  // namespace padel

extern "C" int pa_jpeg_parse(const uint8_t* jpeg, size_t len, pa_jpeg_frame_info* info, pa_jpeg_interval* ivls, size_t ivl_cap, char* why,
                             size_t cap) {
    std::string err;
    std::vector<pa_jpeg_interval> v;
    pa_jpeg_frame_info local;
    const int rc = padel::jpeg_parse_frame(jpeg, len, info ? info : &local, v, err);
    if (why && cap) snprintf(why, cap, "%s", rc ? err.c_str() : "");
    if (!rc && ivls)
        for (size_t k = 0; k < v.size() && k < ivl_cap; ++k) ivls[k] = v[k];
    return rc;
}
