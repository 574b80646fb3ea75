// What is decided about a pa_render call before anything runs, and the font: host-only code (no HIP runtime call), built with
// g++ like graph_plan.cpp, so that the same refusals and the same glyphs are available without a GPU (pa_render_check,
// pa_glyph_rows, tests/render_marks_main.cpp).
#include "render_check.h"
#include "render_scale.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace padel {

#define FAIL(...)                                                \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        err = _b;                                                \
        return 1;                                                \
    } while (0)

// ------------------------------------------------------------------------------- the font: 5 x 7, drawn here, 40 codes
struct Glyph { char code; const char* rows[kGlyphH]; };
static const Glyph kFont[] = {
    {'0', {".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."}},
    {'1', {"..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."}},
    {'2', {".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"}},
    {'3', {"#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."}},
    {'4', {"...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."}},
    {'5', {"#####", "#....", "####.", "....#", "....#", "#...#", ".###."}},
    {'6', {"..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."}},
    {'7', {"#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."}},
    {'8', {".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."}},
    {'9', {".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."}},
    {'A', {".###.", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"}},
    {'B', {"####.", "#...#", "#...#", "####.", "#...#", "#...#", "####."}},
    {'C', {".###.", "#...#", "#....", "#....", "#....", "#...#", ".###."}},
    {'D', {"###..", "#..#.", "#...#", "#...#", "#...#", "#..#.", "###.."}},
    {'E', {"#####", "#....", "#....", "####.", "#....", "#....", "#####"}},
    {'F', {"#####", "#....", "#....", "####.", "#....", "#....", "#...."}},
    {'G', {".###.", "#...#", "#....", "#.###", "#...#", "#...#", ".####"}},
    {'H', {"#...#", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"}},
    {'I', {".###.", "..#..", "..#..", "..#..", "..#..", "..#..", ".###."}},
    {'J', {"..###", "...#.", "...#.", "...#.", "...#.", "#..#.", ".##.."}},
    {'K', {"#...#", "#..#.", "#.#..", "##...", "#.#..", "#..#.", "#...#"}},
    {'L', {"#....", "#....", "#....", "#....", "#....", "#....", "#####"}},
    {'M', {"#...#", "##.##", "#.#.#", "#.#.#", "#...#", "#...#", "#...#"}},
    {'N', {"#...#", "#...#", "##..#", "#.#.#", "#..##", "#...#", "#...#"}},
    {'O', {".###.", "#...#", "#...#", "#...#", "#...#", "#...#", ".###."}},
    {'P', {"####.", "#...#", "#...#", "####.", "#....", "#....", "#...."}},
    {'Q', {".###.", "#...#", "#...#", "#...#", "#.#.#", "#..#.", ".##.#"}},
    {'R', {"####.", "#...#", "#...#", "####.", "#.#..", "#..#.", "#...#"}},
    {'S', {".####", "#....", "#....", ".###.", "....#", "....#", "####."}},
    {'T', {"#####", "..#..", "..#..", "..#..", "..#..", "..#..", "..#.."}},
    {'U', {"#...#", "#...#", "#...#", "#...#", "#...#", "#...#", ".###."}},
    {'V', {"#...#", "#...#", "#...#", "#...#", "#...#", ".#.#.", "..#.."}},
    {'W', {"#...#", "#...#", "#...#", "#.#.#", "#.#.#", "##.##", "#...#"}},
    {'X', {"#...#", "#...#", ".#.#.", "..#..", ".#.#.", "#...#", "#...#"}},
    {'Y', {"#...#", "#...#", ".#.#.", "..#..", "..#..", "..#..", "..#.."}},
    {'Z', {"#####", "....#", "...#.", "..#..", ".#...", "#....", "#####"}},
    {' ', {".....", ".....", ".....", ".....", ".....", ".....", "....."}},
    {':', {".....", "..#..", "..#..", ".....", "..#..", "..#..", "....."}},
    {'.', {".....", ".....", ".....", ".....", ".....", "..#..", "..#.."}},
    {'-', {".....", ".....", ".....", ".###.", ".....", ".....", "....."}},
};

int glyph_rows(int code, uint8_t rows[kGlyphH]) {
    for (const Glyph& g : kFont) {
        if (g.code != code) continue;
        for (int j = 0; j < kGlyphH; ++j) {
            rows[j] = 0;
            for (int i = 0; i < kGlyphW; ++i) if (g.rows[j][i] == '#') rows[j] |= (uint8_t)(1u << i);
        }
        return 0;
    }
    return 1;
}

void render_resolve_marks(const pa_mark* in, pa_mark* out, size_t count) {
    for (size_t k = 0; k < count; ++k) {
        out[k] = in[k];
        if (in[k].kind != PA_MARK_GLYPH) continue;
        uint8_t rows[kGlyphH] = {};
        glyph_rows(in[k].arg, rows);
        unsigned long long bits = 0;
        for (int j = 0; j < kGlyphH; ++j) bits |= (unsigned long long)rows[j] << (j * kGlyphW);
        out[k].x1 = (int32_t)(uint32_t)(bits & 0xffffffffull);
        out[k].y1 = (int32_t)(uint32_t)(bits >> 32);
    }
}

// ------------------------------------------------------------------------------- the refusals of pa_render
static bool coord_ok(int v) { return v >= kMarkCoordMin && v <= kMarkCoordMax; }

int render_validate(int n, int h, int w, const pa_mark* marks, const int32_t* first, int out, const pa_yuv_desc* g, const pa_yuv_enc* enc,
                    size_t* dst_span, std::string& err) {
    if (n < 1 || n > 65535) FAIL("pa_render: n = %d frames outside [1, 65535]", n);
    if (w < 1 || h < 1 || w > kRenderMaxSide || h > kRenderMaxSide) FAIL("pa_render: %d x %d frames: width and height must lie in [1, %d]", w, h, kRenderMaxSide);
    if (out != PA_RENDER_BGR && out != PA_RENDER_YUV420) FAIL("pa_render: unknown output %d", out);
    if (!first) FAIL("pa_render: first is NULL");
    if (first[0] != 0) FAIL("pa_render: first[0] = %d, must be 0", first[0]);
    for (int i = 0; i < n; ++i)
        if (first[i + 1] < first[i]) FAIL("pa_render: first[] decreases at frame %d (%d after %d)", i, first[i + 1], first[i]);
    const int total = first[n];
    if (total > 0 && !marks) FAIL("pa_render: %d marks announced by first[], marks is NULL", total);
    for (int k = 0; k < total; ++k) {
        const pa_mark& m = marks[k];
        if (m.kind < PA_MARK_DISC || (m.kind > PA_MARK_BLEND && m.kind != PA_MARK_ARC)) FAIL("pa_render: mark %d has unknown kind %d", k, m.kind);
        if (!coord_ok(m.x0) || !coord_ok(m.y0) || !coord_ok(m.x1) || !coord_ok(m.y1))
            FAIL("pa_render: mark %d has a coordinate outside [%d, %d] (%d, %d, %d, %d)", k, kMarkCoordMin, kMarkCoordMax, m.x0, m.y0, m.x1, m.y1);
        // (a fill and a blend have no size: 0..255 are accepted and ignored)
        const int lo = (m.kind == PA_MARK_DISC || m.kind == PA_MARK_FILL || m.kind == PA_MARK_BLEND) ? 0 : 1, hi = m.kind == PA_MARK_GLYPH ? kGlyphMaxScale : 255;
        if (m.size < lo || m.size > hi) FAIL("pa_render: mark %d (kind %d) has size %d outside [%d, %d]", k, m.kind, m.size, lo, hi);
        if (m.bgr > 0xffffffu) FAIL("pa_render: mark %d has colour 0x%x beyond 24 bits", k, m.bgr);
        uint8_t rows[kGlyphH];
        if (m.kind == PA_MARK_GLYPH) {
            if (glyph_rows(m.arg, rows)) FAIL("pa_render: mark %d names character code %d, which the font does not have", k, m.arg);
            if (m.x1 != 0 || m.y1 != 0) FAIL("pa_render: glyph mark %d has x1, y1 = %d, %d, must be 0", k, m.x1, m.y1);
        } else if (m.kind == PA_MARK_BLEND) {
            if (m.arg < 1 || m.arg > 255) FAIL("pa_render: blend mark %d has weight %d outside [1, 255]", k, m.arg);
        } else if (m.kind == PA_MARK_ARC) {
            if (m.x1 < 1 || m.x1 > kArcMaxAxis || m.y1 < 1 || m.y1 > kArcMaxAxis)
                FAIL("pa_render: arc mark %d has a semi-axis outside [1, %d] (a = x1 = %d, b = y1 = %d)", k, kArcMaxAxis, m.x1, m.y1);
            if (m.arg < 1 || m.arg > 255) FAIL("pa_render: arc mark %d has octant mask %d outside [1, 255]", k, m.arg);
        } else if (m.arg != 0) FAIL("pa_render: mark %d (kind %d) has arg %d, must be 0", k, m.kind, m.arg);
    }
    if (out == PA_RENDER_BGR) {
        *dst_span = (size_t)n * h * w * 3;
        return 0;
    }
    if (!g || !enc) FAIL("pa_render: YUV output needs a geometry descriptor and an encode table");
    if (w < 2 || h < 2 || (w & 1) || (h & 1)) FAIL("pa_render: %d x %d frames: 4:2:0 needs an even width and height of at least 2", w, h);
    if (g->layout != PA_YUV_NV12 && g->layout != PA_YUV_I420) FAIL("pa_render: unknown layout %d", g->layout);
    const bool nv12 = g->layout == PA_YUV_NV12;
    const int crow = nv12 ? w : w / 2;
    if (g->pitch_y < w) FAIL("pa_render: pitch_y %d is smaller than a luma row of %d bytes", g->pitch_y, w);
    if (g->pitch_c < crow) FAIL("pa_render: pitch_c %d is smaller than a chroma row of %d bytes", g->pitch_c, crow);
    if (g->off_u < 0 || g->off_v < 0) FAIL("pa_render: negative plane offset (off_u %d, off_v %d)", g->off_u, g->off_v);
    if (nv12 && g->off_v != g->off_u + 1) FAIL("pa_render: NV12 needs off_v == off_u + 1 (off_u %d, off_v %d)", g->off_u, g->off_v);
    const long long y_end = (long long)(h - 1) * g->pitch_y + w;
    const long long c_len = (long long)(h / 2 - 1) * g->pitch_c + crow;
    const long long extent = std::max(y_end, std::max(g->off_u + c_len, nv12 ? 0ll : g->off_v + c_len));
    if (extent > 0x7fffffffll) FAIL("pa_render: a frame of %lld bytes is beyond 2 GiB", extent);
    if (g->frame_stride < extent)
        FAIL("pa_render: frame_stride %lld is smaller than the %lld bytes the planes of one frame span (they would reach into the next frame)",
             (long long)g->frame_stride, extent);
    // the written planes of one frame must not overlap each other either: a later plane's bytes would replace an earlier one's
    if (g->off_u < y_end) FAIL("pa_render: the chroma at off_u %d starts inside the luma plane (%lld bytes)", g->off_u, y_end);
    if (!nv12) {
        if (g->off_v < y_end) FAIL("pa_render: the V plane at off_v %d starts inside the luma plane (%lld bytes)", g->off_v, y_end);
        const long long lo = std::min(g->off_u, g->off_v), hi = std::max(g->off_u, g->off_v);
        if (lo + c_len > hi) FAIL("pa_render: the U and V planes overlap (off_u %d, off_v %d, %lld bytes each)", g->off_u, g->off_v, c_len);
    }
    const auto mag = [](int32_t c) { return (long long)(c < 0 ? -(long long)c : c); };
    if (enc->y_off < 0 || enc->y_off > 255) FAIL("pa_render: y_off %d outside [0, 255]", enc->y_off);
    const long long worst_y = 255 * (mag(enc->yr) + mag(enc->yg) + mag(enc->yb)) + (1 << 19) + ((long long)enc->y_off << 20);
    const long long worst_c = 1020 * std::max(mag(enc->ur) + mag(enc->ug) + mag(enc->ub), mag(enc->vr) + mag(enc->vg) + mag(enc->vb)) + (1 << 21) + (128ll << 22);
    if (worst_y > 0x7fffffffll || worst_c > 0x7fffffffll) FAIL("pa_render: encode coefficients leave int32 (worst case luma %lld, chroma %lld)", worst_y, worst_c);
    *dst_span = (size_t)(n - 1) * (size_t)g->frame_stride + (size_t)extent;
    return 0;
}

// ------------------------------------------------------------------------------- the refusals of pa_render_scaled
int render_scaled_validate(int n, int h, int w, const pa_mark* marks, const int32_t* first, int scale, int out, const pa_yuv_desc* g,
                           const pa_yuv_enc* enc, int dst_is_src, size_t* dst_span, std::string& err) {
    if (scale == 1) return render_validate(n, h, w, marks, first, out, g, enc, dst_span, err);       // pa_render itself
    if (scale < 1 || scale > kRenderMaxScale) FAIL("pa_render_scaled: scale %d outside [1, %d]", scale, kRenderMaxScale);
    if (w < 1 || h < 1 || w > kRenderMaxSide || h > kRenderMaxSide)
        FAIL("pa_render_scaled: %d x %d source frames: width and height must lie in [1, %d]", w, h, kRenderMaxSide);
    if (w % scale || h % scale) FAIL("pa_render_scaled: %d x %d source frames are no multiple of scale %d each way", w, h, scale);
    const int wo = w / scale, ho = h / scale;
    if (out == PA_RENDER_YUV420 && (wo < 2 || ho < 2 || (wo & 1) || (ho & 1)))
        FAIL("pa_render_scaled: %d x %d source frames at scale %d give %d x %d: 4:2:0 needs an even output width and height of at least 2",
             w, h, scale, wo, ho);
    if (dst_is_src) FAIL("pa_render_scaled: dst == src at scale %d (only scale 1 renders in place)", scale);
    return render_validate(n, ho, wo, marks, first, out, g, enc, dst_span, err);                     // marks, first[], the output's geometry
}

}  // namespace padel

extern "C" int pa_render_scaled_check(int n, int h, int w, const pa_mark* marks, const int32_t* first, int scale, int out, const pa_yuv_desc* geom,
                                      const pa_yuv_enc* enc, int dst_is_src, char* why, size_t cap) {
    std::string err;
    size_t span = 0;
    const int rc = padel::render_scaled_validate(n, h, w, marks, first, scale, out, geom, enc, dst_is_src, &span, err);
    if (why && cap) snprintf(why, cap, "%s", rc ? err.c_str() : "");
    return rc;
}

extern "C" int pa_glyph_rows(int code, uint8_t rows[7]) {
    if (!rows) return 1;
    return padel::glyph_rows(code, rows);
}

extern "C" int pa_render_check(int n, int h, int w, const pa_mark* marks, const int32_t* first, int out, const pa_yuv_desc* geom,
                               const pa_yuv_enc* enc, char* why, size_t cap) {
    std::string err;
    size_t span = 0;
    const int rc = padel::render_validate(n, h, w, marks, first, out, geom, enc, &span, err);
    if (why && cap) snprintf(why, cap, "%s", rc ? err.c_str() : "");
    return rc;
}
