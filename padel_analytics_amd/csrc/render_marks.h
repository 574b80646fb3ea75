// The coverage rules of the renderer's marks (include/padel_hip.h, pa_mark), each mark's bounding box and what a covered pixel becomes
// (mark_apply: the colour, or PA_MARK_BLEND's weighted sum), for host and device:
// render.hip applies them to pixel registers, render_check.cpp and tests/render_marks_main.cpp run the same code on the CPU.
// No HIP runtime call, no table: a glyph mark reaches this code RESOLVED (render_resolve_marks, render_check.cpp: the font lives
// there, once) — its 35 font bits, bit j * 5 + i for column i of row j, sit in x1 (bits 0..31) and y1 (bits 32..34).
#pragma once
#include "../../include/padel_hip.h"

#if defined(__HIPCC__)
#define PA_HD __host__ __device__ __forceinline__
#else
#define PA_HD inline
#endif

namespace padel {

constexpr int kMarkCoordMin = -8192, kMarkCoordMax = 8191, kRenderMaxSide = 8192;
constexpr int kGlyphW = 5, kGlyphH = 7, kGlyphMaxScale = 16;
constexpr int kArcMaxAxis = 4095;           // PA_MARK_ARC: a semi-axis; with |dx| <= 16384 every term of its rule stays below 2^54

struct MarkBox { int x0, y0, x1, y1; };      // inclusive on every side; every covered pixel lies inside

PA_HD int mark_min(int a, int b) { return a < b ? a : b; }
PA_HD int mark_max(int a, int b) { return a > b ? a : b; }

PA_HD MarkBox mark_bbox(const pa_mark& m) {
    switch (m.kind) {
    case PA_MARK_DISC:                       // dx^2 <= r^2 + r < (r + 1)^2
        return {m.x0 - m.size, m.y0 - m.size, m.x0 + m.size, m.y0 + m.size};
    case PA_MARK_SEGMENT: {                  // every covered pixel is within t / 2 of the segment: floor(t / 2) in whole pixels
        const int e = m.size >> 1;
        return {mark_min(m.x0, m.x1) - e, mark_min(m.y0, m.y1) - e, mark_max(m.x0, m.x1) + e, mark_max(m.y0, m.y1) + e};
    }
    case PA_MARK_FILL:
    case PA_MARK_BOX:
    case PA_MARK_BLEND:
        return {mark_min(m.x0, m.x1), mark_min(m.y0, m.y1), mark_max(m.x0, m.x1), mark_max(m.y0, m.y1)};
    case PA_MARK_GLYPH:
        return {m.x0, m.y0, m.x0 + kGlyphW * m.size - 1, m.y0 + kGlyphH * m.size - 1};
    case PA_MARK_ARC:                        // the outer ellipse's box: semi-axes x1, y1 <= 4095, so every edge fits 16 bits
        return {m.x0 - m.x1, m.y0 - m.y1, m.x0 + m.x1, m.y0 + m.y1};
    default:
        return {0, 0, -1, -1};
    }
}

PA_HD bool mark_box_meets(const MarkBox& b, int x0, int y0, int x1, int y1) {
    return b.x0 <= x1 && b.x1 >= x0 && b.y0 <= y1 && b.y1 >= y0;
}

// Is pixel (x, y), 0 <= x, y < 8192, covered?  The caller has checked the mark (render_validate): with its bounds the int32
// terms below stay under 2^31 and the int64 ones under 2^62.
PA_HD bool mark_covers(const pa_mark& m, int x, int y) {
    switch (m.kind) {
    case PA_MARK_DISC: {
        const int dx = x - m.x0, dy = y - m.y0, r = m.size;            // |dx|, |dy| <= 16383: the sum is below 2^30
        return dx * dx + dy * dy <= r * r + r;
    }
    case PA_MARK_SEGMENT: {
        const int dx = m.x1 - m.x0, dy = m.y1 - m.y0, px = x - m.x0, py = y - m.y0;
        const long long t2 = (long long)m.size * m.size;
        const long long L2 = (long long)dx * dx + (long long)dy * dy;
        const long long s = (long long)px * dx + (long long)py * dy;
        if (L2 == 0 || s <= 0) return 4 * ((long long)px * px + (long long)py * py) <= t2;
        if (s >= L2) {
            const long long qx = x - m.x1, qy = y - m.y1;
            return 4 * (qx * qx + qy * qy) <= t2;
        }
        const long long cross = (long long)px * dy - (long long)py * dx;
        return 4 * cross * cross <= t2 * L2;
    }
    case PA_MARK_FILL:
    case PA_MARK_BLEND:
        return x >= mark_min(m.x0, m.x1) && x <= mark_max(m.x0, m.x1) && y >= mark_min(m.y0, m.y1) && y <= mark_max(m.y0, m.y1);
    case PA_MARK_BOX: {
        const int ax = mark_min(m.x0, m.x1), bx = mark_max(m.x0, m.x1), ay = mark_min(m.y0, m.y1), by = mark_max(m.y0, m.y1), t = m.size;
        if (x < ax || x > bx || y < ay || y > by) return false;
        return !(x >= ax + t && x <= bx - t && y >= ay + t && y <= by - t);
    }
    case PA_MARK_GLYPH: {
        const int k = m.size, ex = x - m.x0, ey = y - m.y0;
        if (ex < 0 || ey < 0 || ex >= kGlyphW * k || ey >= kGlyphH * k) return false;
        const int bit = (ey / k) * kGlyphW + ex / k;
        return bit < 32 ? ((unsigned)m.x1 >> bit) & 1u : ((unsigned)m.y1 >> (bit - 32)) & 1u;
    }
    case PA_MARK_ARC: {
        // |dx|, |dy| <= 16383 + 1 and a, b <= 4095: a squared offset times a squared semi-axis is below 2^53, a sum of two below 2^54
        const int dx = x - m.x0, dy = y - m.y0, a = m.x1, b = m.y1, t = m.size;
        const int ex = dx < 0 ? -dx : dx, ey = dy < 0 ? -dy : dy;
        const long long A2 = (long long)a * a, B2 = (long long)b * b, full = A2 * B2;
        const long long X2 = (long long)ex * ex * B2, Y2 = (long long)ey * ey * A2;
        if (X2 + Y2 > full) return false;                                  // 1. outside the outer ellipse
        // 3. the octant, in parameter space: (uu, vv) is (u, v) rotated into u > 0, v >= 0 by k quarter turns (v, -u)
        const int u = dx * b, v = dy * a;                                  // below 2^26
        int k = 0, uu = 1, vv = 0;                                         // (the centre: octant 0)
        if (u > 0 && v >= 0) { uu = u; vv = v; }
        else if (v > 0 && u <= 0) { k = 1; uu = v; vv = -u; }
        else if (u < 0 && v <= 0) { k = 2; uu = -u; vv = -v; }
        else if (v < 0 && u >= 0) { k = 3; uu = -v; vv = u; }
        if (!(((unsigned)m.arg >> (2 * k + (vv >= uu ? 1 : 0))) & 1u)) return false;
        // 2. the hole rule ...
        const int ai = a - t, bi = b - t;
        if (ai < 1 || bi < 1) return true;
        const long long Ai2 = (long long)ai * ai, Bi2 = (long long)bi * bi;
        if ((long long)ex * ex * Bi2 + (long long)ey * ey * Ai2 > Ai2 * Bi2) return true;
        // ... or the rim rule.  The pixel is inside the outer ellipse, so of its four neighbours only the two farther from the centre,
        // (|dx| + 1, dy) and (dx, |dy| + 1), can be outside it: (|dx| + 1)^2 = dx^2 + 2 |dx| + 1
        return X2 + (2 * ex + 1) * B2 + Y2 > full || X2 + Y2 + (2 * ey + 1) * A2 > full;
    }
    default:
        return false;
    }
}

// What a COVERED pixel p (B | G << 8 | R << 16) becomes under mark m: the mark's colour, or for PA_MARK_BLEND with weight a = arg in
// 1..255 (render_validate) per channel (p * (256 - a) + c * a + 128) >> 8 — at most 255 * 256 + 128 < 2^16, so B and R are blended
// together in one multiply (bits 0..15 and 16..31 of a 32-bit word, the sum of the two weights being 256: no carry between them)
PA_HD unsigned mark_apply(const pa_mark& m, unsigned p) {
    if (m.kind != PA_MARK_BLEND) return m.bgr;
    const unsigned a = (unsigned)m.arg, b = 256u - a, c = m.bgr;
    const unsigned rb = ((p & 0xff00ffu) * b + (c & 0xff00ffu) * a + 0x800080u) >> 8;
    const unsigned g = ((p & 0xff00u) * b + (c & 0xff00u) * a + 0x8000u) >> 8;
    return (rb & 0xff00ffu) | (g & 0xff00u);
}

}  // namespace padel
