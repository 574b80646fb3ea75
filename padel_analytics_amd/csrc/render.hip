// Marks drawn on packed BGR frames, written as BGR or as 8-bit YUV 4:2:0 (NV12 / I420) — the reverse of yuv_convert.hip and the
// same shape (gfx950), HBM-bound: 3 bytes read and 1.5 (or 3) written per pixel, the marks applied in registers on the way through.
// The coverage rules are include/padel_hip.h (pa_mark), their code render_marks.h, the readable twin render.render_host.
// One thread owns a 2-row x 4-pixel block (one chroma pair per 2 x 2), a workgroup is 32 x 8 threads: a tile of 128 x 16 pixels.
// The workgroup walks its frame's marks in list order, kCullChunk at a time: every thread tests one mark's bounding box (8 bytes,
// computed once on the host with the same mark_bbox) against the tile, the survivors — only they are read in full — are compacted
// into LDS IN LIST ORDER (ballot + popcount inside a wave, the four waves' counts in LDS: a
// thread's slot = survivors before it in the chunk) and applied to the pixel registers before the next chunk is looked at — so a
// later mark always applies to what the earlier ones left (mark_apply: overwrites it, or PA_MARK_BLEND blends into it), within a chunk
// and across chunks.  A chunk can keep at most kCullChunk marks: the
// LDS list cannot overflow.
// kVec: three dword loads per 4-pixel row, dword stores of Y, of BGR and of NV12's UV, 16-bit stores for I420's planes — only when
// the launcher has checked every address of THIS launch; otherwise bytes, which also cover widths that are no multiple of 4.
#include <type_traits>

#include "kernels.h"
#include "render_marks.h"
#include "render_scale.h"

namespace padel {

constexpr int kCullChunk = 256;          // marks looked at per pass = threads of the workgroup = capacity of the LDS list
enum { OUT_BGR = 0, OUT_NV12 = 1, OUT_I420 = 2 };

// clamp(x >> s, 0, 255) with the clamp applied BEFORE the shift: see yuv_clamp8 (yuv_convert.hip) for why not the other order
template <int S>
__device__ __forceinline__ unsigned enc_clamp8(int x) { return (unsigned)(min(max(x, 0), (255 << S) | ((1 << S) - 1)) >> S); }

__device__ __forceinline__ unsigned enc_luma(const RenderArgs& a, unsigned p) {
    const int B = p & 0xff, G = (p >> 8) & 0xff, R = (p >> 16) & 0xff;
    return enc_clamp8<20>(a.yr * R + a.yg * G + a.yb * B + (1 << 19) + (a.y_off << 20));      // (s >> 20) + y_off == (s + (y_off << 20)) >> 20
}

// U | V << 8 of the 2 x 2 block p00 p01 / p10 p11
__device__ __forceinline__ unsigned enc_chroma(const RenderArgs& a, unsigned p00, unsigned p01, unsigned p10, unsigned p11) {
    const int B = (p00 & 0xff) + (p01 & 0xff) + (p10 & 0xff) + (p11 & 0xff);
    const int G = ((p00 >> 8) & 0xff) + ((p01 >> 8) & 0xff) + ((p10 >> 8) & 0xff) + ((p11 >> 8) & 0xff);
    const int R = ((p00 >> 16) & 0xff) + ((p01 >> 16) & 0xff) + ((p10 >> 16) & 0xff) + ((p11 >> 16) & 0xff);
    const int bias = (1 << 21) + (128 << 22);
    return enc_clamp8<22>(a.ur * R + a.ug * G + a.ub * B + bias) | (enc_clamp8<22>(a.vr * R + a.vg * G + a.vb * B + bias) << 8);
}

// a mark's box as the host packed it: x0 | y0 << 16, x1 | y1 << 16, each a signed 16-bit number
__device__ __forceinline__ MarkBox unpack_box(uint2 b) {
    return {(int)(short)(b.x & 0xffff), (int)b.x >> 16, (int)(short)(b.y & 0xffff), (int)b.y >> 16};
}

// PA_MARK_ARC's coverage of a thread's 2 x 4 block, bit r * 4 + c.  One pixel at a time ON PURPOSE: the rule is 64-bit products, and
// the eight pixels' worth of them live at once (the unrolled loop the other kinds use) took the kernel from 46-53 to 80-90 VGPRs
// and from 8 to 5-6 waves per SIMD for every scene, arcs or none (profiles/render_arc.txt).  An arc's box is mostly hole: few
// threads get here, and those that do pay eight short iterations
__device__ __forceinline__ unsigned arc_block_bits(const pa_mark& m, int px, int py) {
    unsigned bits = 0;
#pragma unroll 1
    for (int i = 0; i < 8; ++i) bits |= (mark_covers(m, px + (i & 3), py + (i >> 2)) ? 1u : 0u) << i;
    return bits;
}

template <bool kVec, int kOut>
__global__ void __launch_bounds__(256) render_kernel(const RenderArgs a) {
    __shared__ uint4 s_marks[kCullChunk * 2];            // pa_mark = 2 x uint4
    __shared__ uint2 s_boxes[kCullChunk];                // their boxes: what a thread rejects by before it reads a mark
    __shared__ int s_count[4];
    const int tid = threadIdx.y * 32 + threadIdx.x;      // (x fastest: waves are tid >> 6)
    const int tx0 = blockIdx.x * 128, ty0 = blockIdx.y * 16;
    const int px = tx0 + threadIdx.x * 4, py = ty0 + threadIdx.y * 2;
    const int frame = blockIdx.z;
    const size_t row_bytes = (size_t)a.w * 3;
    const uint8_t* sp = a.src + ((size_t)frame * a.h + py) * row_bytes + (size_t)px * 3;
    // columns / rows of this thread's block that exist (w and h need not be multiples of the block in BGR mode)
    const int ncol = min(4, a.w - px), nrow = min(2, a.h - py);      // <= 0: nothing of the block is inside the frame

    // ---- the frame's marks, kCullChunk at a time, in list order.  The first chunk's boxes are asked for BEFORE the pixels, so that
    // the cull waits for 8 bytes per thread, not behind the tile's own 6 KB (loads return in order), and runs under the pixel loads
    const pa_mark* marks = reinterpret_cast<const pa_mark*>(a.marks);
    const uint2* boxes = reinterpret_cast<const uint2*>(a.boxes);
    const int m_begin = a.first[frame], m_end = a.first[frame + 1];
    const int lane = tid & 63, wave = tid >> 6;
    uint2 bx = {0, 0};
    if (m_begin + tid < m_end) bx = boxes[m_begin + tid];

    unsigned pix[2][4];                                  // B | G << 8 | R << 16
    unsigned raw[2][3];                                  // kVec: the 12 bytes of a row as loaded, B G R B | G R B G | R B G R
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) pix[r][c] = 0;
        if (kVec) {
            // w % 4 == 0: a block is whole or absent.  The loads are UNCONDITIONAL — a block outside the frame reads the frame's
            // last block / row instead and never stores — so that the compiler can count them: the cull below then waits for the
            // boxes alone (vmcnt(2)), not for these
            const uint8_t* q = a.src + ((size_t)frame * a.h + min(py + r, a.h - 1)) * row_bytes + (size_t)min(px, a.w - 4) * 3;
            const unsigned* qd = reinterpret_cast<const unsigned*>(q);
            raw[r][0] = qd[0]; raw[r][1] = qd[1]; raw[r][2] = qd[2];
        } else {
            raw[r][0] = raw[r][1] = raw[r][2] = 0;
            if (r >= nrow || ncol <= 0) continue;
            const uint8_t* q = sp + (size_t)r * row_bytes;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < ncol) pix[r][c] = (unsigned)q[3 * c] | ((unsigned)q[3 * c + 1] << 8) | ((unsigned)q[3 * c + 2] << 16);
        }
    }
#ifdef PADEL_RENDER_PROBE
    const long long t_begin = clock64();
    long long t_cull = 0, t_apply = 0;
#endif

    // marks [base, base + kCullChunk) -> the LDS list, in order; returns how many the tile keeps (uniform).  Two barriers
    const auto cull = [&](int base, uint2 box) -> int {
        const int mi = base + tid;
        const bool keep = mi < m_end && mark_box_meets(unpack_box(box), tx0, ty0, tx0 + 127, ty0 + 15);
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_count[wave] = __popcll(vote);
        __syncthreads();                                 // counts visible; the previous chunk's list has been applied by everyone
        const int c0 = s_count[0], c1 = s_count[1], c2 = s_count[2], c3 = s_count[3];
        if (keep) {
            const int before = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0) + __popcll(vote & ((1ull << lane) - 1ull));
            const uint4* g = reinterpret_cast<const uint4*>(marks + mi);
            s_marks[before * 2] = g[0];
            s_marks[before * 2 + 1] = g[1];
            s_boxes[before] = box;
        }
        __syncthreads();                                 // the list is complete
        return c0 + c1 + c2 + c3;
    };

    int base = m_begin, total = 0;
    if (base < m_end) total = cull(base, bx);
#ifdef PADEL_RENDER_PROBE
    t_cull += clock64() - t_begin;
#endif
    if (kVec) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            pix[r][0] = raw[r][0] & 0xffffff;
            pix[r][1] = (raw[r][0] >> 24) | ((raw[r][1] & 0xffff) << 8);
            pix[r][2] = (raw[r][1] >> 16) | ((raw[r][2] & 0xff) << 16);
            pix[r][3] = raw[r][2] >> 8;
        }
    }
    bool touched = false;                                // uniform: some mark's box met this tile
    while (base < m_end) {
#ifdef PADEL_RENDER_PROBE
        const long long t1 = clock64();
#endif
        if (total > 0) touched = true;
        if (nrow > 0 && ncol > 0) {
            for (int k = 0; k < total; ++k) {
                if (!mark_box_meets(unpack_box(s_boxes[k]), px, py, px + 3, py + 1)) continue;
                const uint4 l = s_marks[k * 2], u = s_marks[k * 2 + 1];
                pa_mark m;
                m.kind = (int)l.x; m.x0 = (int)l.y; m.y0 = (int)l.z; m.x1 = (int)l.w; m.y1 = (int)u.x; m.size = (int)u.y; m.bgr = u.z; m.arg = (int)u.w;
                // One switch per mark, not one per pixel: the record is the same for every lane (the compiler keeps it in scalar
                // registers), so this is a scalar branch, and inside an arm the kind is a constant — mark_covers is that kind's rule
                // alone and mark_apply the colour, or for PA_MARK_BLEND the weighted sum: an opaque mark pays nothing for the kind
                // that blends.  (One loop over the pixels with the kind tested inside it cost the 206-mark scene 13-24 % once there
                // were six kinds: profiles/render_blend.txt)
                const auto apply = [&](auto kind) {
                    pa_mark mk = m;
                    mk.kind = decltype(kind)::value;
                    if constexpr (decltype(kind)::value == PA_MARK_ARC) {
                        const unsigned bits = arc_block_bits(mk, px, py);
#pragma unroll
                        for (int r = 0; r < 2; ++r)
#pragma unroll
                            for (int c = 0; c < 4; ++c)
                                if ((bits >> (r * 4 + c)) & 1u) pix[r][c] = mk.bgr;
                        return;
                    }
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (mark_covers(mk, px + c, py + r)) pix[r][c] = mark_apply(mk, pix[r][c]);
                };
                switch (m.kind) {
                case PA_MARK_DISC: apply(std::integral_constant<int, PA_MARK_DISC>()); break;
                case PA_MARK_SEGMENT: apply(std::integral_constant<int, PA_MARK_SEGMENT>()); break;
                case PA_MARK_FILL: apply(std::integral_constant<int, PA_MARK_FILL>()); break;
                case PA_MARK_BOX: apply(std::integral_constant<int, PA_MARK_BOX>()); break;
                case PA_MARK_GLYPH: apply(std::integral_constant<int, PA_MARK_GLYPH>()); break;
                case PA_MARK_BLEND: apply(std::integral_constant<int, PA_MARK_BLEND>()); break;
                case PA_MARK_ARC: apply(std::integral_constant<int, PA_MARK_ARC>()); break;
                default: break;                              // (render_validate lets no other kind through)
                }
            }
        }
        __syncthreads();                                 // everyone is done with the list and the counts before the next chunk rewrites them
#ifdef PADEL_RENDER_PROBE
        const long long t2 = clock64();
        t_apply += t2 - t1;
#endif
        base += kCullChunk;
        if (base < m_end) {
            bx = uint2{0, 0};
            if (base + tid < m_end) bx = boxes[base + tid];
            total = cull(base, bx);
        }
#ifdef PADEL_RENDER_PROBE
        t_cull += clock64() - t2;
#endif
    }
#ifdef PADEL_RENDER_PROBE
    if (tid == 0 && a.probe) {
        atomicAdd(a.probe + 0, (unsigned long long)t_cull);
        atomicAdd(a.probe + 1, (unsigned long long)t_apply);
        atomicAdd(a.probe + 2, (unsigned long long)(clock64() - t_begin));      // (from the loads' issue up to the stores, which follow)
        atomicAdd(a.probe + 3, 1ull);
    }
#endif
    if (nrow <= 0 || ncol <= 0) return;                  // (after the last barrier)

    if (kOut == OUT_BGR) {
        if (a.in_place && !touched) return;
        uint8_t* dp = a.dst + ((size_t)frame * a.h + py) * row_bytes + (size_t)px * 3;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= nrow) continue;
            uint8_t* q = dp + (size_t)r * row_bytes;
            if (kVec) {
                unsigned* qd = reinterpret_cast<unsigned*>(q);
                qd[0] = pix[r][0] | (pix[r][1] << 24);
                qd[1] = (pix[r][1] >> 8) | (pix[r][2] << 16);
                qd[2] = (pix[r][2] >> 16) | (pix[r][3] << 8);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < ncol) { q[3 * c] = (uint8_t)pix[r][c]; q[3 * c + 1] = (uint8_t)(pix[r][c] >> 8); q[3 * c + 2] = (uint8_t)(pix[r][c] >> 16); }
            }
        }
    } else {                                             // w, h even: nrow == 2, ncol is 2 or 4
        uint8_t* f = a.dst + (size_t)frame * (size_t)a.frame_stride;
        uint8_t* yp = f + (size_t)py * a.pitch_y + px;
        const size_t crow = (size_t)(py >> 1) * a.pitch_c;
        const unsigned uv0 = enc_chroma(a, pix[0][0], pix[0][1], pix[1][0], pix[1][1]);
        const unsigned uv1 = enc_chroma(a, pix[0][2], pix[0][3], pix[1][2], pix[1][3]);
        if (kVec) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
                *reinterpret_cast<unsigned*>(yp + (size_t)r * a.pitch_y) =
                    enc_luma(a, pix[r][0]) | (enc_luma(a, pix[r][1]) << 8) | (enc_luma(a, pix[r][2]) << 16) | (enc_luma(a, pix[r][3]) << 24);
            if (kOut == OUT_NV12) {
                *reinterpret_cast<unsigned*>(f + a.off_u + crow + px) = uv0 | (uv1 << 16);          // U0 V0 U1 V1
            } else {
                *reinterpret_cast<unsigned short*>(f + a.off_u + crow + (px >> 1)) = (unsigned short)((uv0 & 0xff) | ((uv1 & 0xff) << 8));
                *reinterpret_cast<unsigned short*>(f + a.off_v + crow + (px >> 1)) = (unsigned short)((uv0 >> 8) | (uv1 & 0xff00));
            }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < ncol) yp[(size_t)r * a.pitch_y + c] = (uint8_t)enc_luma(a, pix[r][c]);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (2 * k >= ncol) continue;
                const unsigned uv = k ? uv1 : uv0;
                if (kOut == OUT_NV12) {
                    uint8_t* pc = f + a.off_u + crow + px + 2 * k;
                    pc[0] = (uint8_t)uv; pc[1] = (uint8_t)(uv >> 8);
                } else {
                    f[a.off_u + crow + (px >> 1) + k] = (uint8_t)uv;
                    f[a.off_v + crow + (px >> 1) + k] = (uint8_t)(uv >> 8);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------- pa_render_scaled, s = 2, 3, 4
// The same pass with an s x s box average behind the marks (include/padel_hip.h): a.h x a.w is the SOURCE, the output is
// (a.h / S) x (a.w / S) and the geometry fields describe it.  One thread owns ONE output pixel — its S x S source pixels stay in
// registers across the chunks of marks — a workgroup of 32 x 8 threads a tile of 32 S x 8 S source pixels.  A wave is two rows of 32
// threads, so the 2 x 2 block of output pixels that shares a chroma sample is lanes l, l ^ 1, l ^ 32, l ^ 33 of one wave: chroma,
// and the packing of four neighbours' bytes into a dword, are cross-lane moves, no LDS.
// The cull, the list and the per-mark switch are render_kernel's, restated for an R x C block of any size: sharing one copy with
// render_kernel was tried and took its six instantiations from 47-53 to 59-63 VGPRs (profiles/render_scale.txt), and their
// register count is pinned (profiles/render_arc.txt).
template <int R, int C>
__device__ __forceinline__ unsigned arc_bits_rc(const pa_mark& m, int px, int py) {      // arc_block_bits for an R x C block, R * C <= 32
    unsigned bits = 0;
#pragma unroll 1
    for (int i = 0; i < R * C; ++i) bits |= (mark_covers(m, px + i % C, py + i / C) ? 1u : 0u) << i;
    return bits;
}

// the first `total` marks of the LDS list applied, in list order, to a thread's R x C block of pixel registers at (px, py)
template <int R, int C>
__device__ __forceinline__ void apply_list(const uint4* s_marks, const uint2* s_boxes, int total, int px, int py, unsigned (&pix)[R][C]) {
    for (int k = 0; k < total; ++k) {
        if (!mark_box_meets(unpack_box(s_boxes[k]), px, py, px + C - 1, py + R - 1)) continue;
        const uint4 l = s_marks[k * 2], u = s_marks[k * 2 + 1];
        pa_mark m;
        m.kind = (int)l.x; m.x0 = (int)l.y; m.y0 = (int)l.z; m.x1 = (int)l.w; m.y1 = (int)u.x; m.size = (int)u.y; m.bgr = u.z; m.arg = (int)u.w;
        const auto apply = [&](auto kind) {              // (one scalar switch per mark, the kind a constant inside an arm: render_kernel)
            pa_mark mk = m;
            mk.kind = decltype(kind)::value;
            if constexpr (decltype(kind)::value == PA_MARK_ARC) {
                const unsigned bits = arc_bits_rc<R, C>(mk, px, py);
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        if ((bits >> (r * C + c)) & 1u) pix[r][c] = mk.bgr;
                return;
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < C; ++c)
                    if (mark_covers(mk, px + c, py + r)) pix[r][c] = mark_apply(mk, pix[r][c]);
        };
        switch (m.kind) {
        case PA_MARK_DISC: apply(std::integral_constant<int, PA_MARK_DISC>()); break;
        case PA_MARK_SEGMENT: apply(std::integral_constant<int, PA_MARK_SEGMENT>()); break;
        case PA_MARK_FILL: apply(std::integral_constant<int, PA_MARK_FILL>()); break;
        case PA_MARK_BOX: apply(std::integral_constant<int, PA_MARK_BOX>()); break;
        case PA_MARK_GLYPH: apply(std::integral_constant<int, PA_MARK_GLYPH>()); break;
        case PA_MARK_BLEND: apply(std::integral_constant<int, PA_MARK_BLEND>()); break;
        case PA_MARK_ARC: apply(std::integral_constant<int, PA_MARK_ARC>()); break;
        default: break;
        }
    }
}

template <int S, bool kVec, int kOut>
__global__ void __launch_bounds__(256) render_scaled_kernel(const RenderArgs a) {
    __shared__ uint4 s_marks[kCullChunk * 2];
    __shared__ uint2 s_boxes[kCullChunk];
    __shared__ int s_count[4];
    const int tid = threadIdx.y * 32 + threadIdx.x;      // lane = (threadIdx.y & 1) * 32 + threadIdx.x
    const int wo = a.w / S, ho = a.h / S;                // (a.w, a.h are multiples of S)
    const int X = blockIdx.x * 32 + threadIdx.x, Y = blockIdx.y * 8 + threadIdx.y;          // this thread's output pixel
    const int tx0 = blockIdx.x * (32 * S), ty0 = blockIdx.y * (8 * S);
    const int px = X * S, py = Y * S;
    const int frame = blockIdx.z;
    const bool valid = X < wo && Y < ho;
    const size_t row_bytes = (size_t)a.w * 3;

    const pa_mark* marks = reinterpret_cast<const pa_mark*>(a.marks);
    const uint2* boxes = reinterpret_cast<const uint2*>(a.boxes);
    const int m_begin = a.first[frame], m_end = a.first[frame + 1];
    const int lane = tid & 63, wave = tid >> 6;
    uint2 bx = {0, 0};
    if (m_begin + tid < m_end) bx = boxes[m_begin + tid];               // (asked for before the pixels: render_kernel)

    // kVec: the 3 S bytes of a row of the block sit `sh` bytes into kDw aligned dwords (rows start on a dword: a.w % 4 == 0).  Every
    // one of those dwords holds at least one byte of the block, and the frames end on a dword, so none reaches past the source
    constexpr int kDw = S == 2 ? 2 : 3;
    unsigned pix[S][S];                                  // B | G << 8 | R << 16
    unsigned raw[S][kDw];
    const int xoff = min(X, wo - 1) * (3 * S);           // (a thread outside the frame reads the last block / row instead and never stores)
    const unsigned sh = (unsigned)xoff & 3u;
#pragma unroll
    for (int r = 0; r < S; ++r) {
#pragma unroll
        for (int c = 0; c < S; ++c) pix[r][c] = 0;
        if (kVec) {
            const uint8_t* q = a.src + ((size_t)frame * a.h + min(py + r, a.h - 1)) * row_bytes + (size_t)(xoff & ~3);
            const unsigned* qd = reinterpret_cast<const unsigned*>(q);
#pragma unroll
            for (int i = 0; i < kDw; ++i) raw[r][i] = qd[i];
        } else {
#pragma unroll
            for (int i = 0; i < kDw; ++i) raw[r][i] = 0;
            if (!valid) continue;
            const uint8_t* q = a.src + ((size_t)frame * a.h + py + r) * row_bytes + (size_t)px * 3;
#pragma unroll
            for (int c = 0; c < S; ++c) pix[r][c] = (unsigned)q[3 * c] | ((unsigned)q[3 * c + 1] << 8) | ((unsigned)q[3 * c + 2] << 16);
        }
    }

    const auto cull = [&](int base, uint2 box) -> int {  // render_kernel's, the tile being 32 S x 8 S
        const int mi = base + tid;
        const bool keep = mi < m_end && mark_box_meets(unpack_box(box), tx0, ty0, tx0 + 32 * S - 1, ty0 + 8 * S - 1);
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_count[wave] = __popcll(vote);
        __syncthreads();
        const int c0 = s_count[0], c1 = s_count[1], c2 = s_count[2], c3 = s_count[3];
        if (keep) {
            const int before = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0) + __popcll(vote & ((1ull << lane) - 1ull));
            const uint4* g = reinterpret_cast<const uint4*>(marks + mi);
            s_marks[before * 2] = g[0];
            s_marks[before * 2 + 1] = g[1];
            s_boxes[before] = box;
        }
        __syncthreads();
        return c0 + c1 + c2 + c3;
    };

    int base = m_begin, total = 0;
    if (base < m_end) total = cull(base, bx);
    if (kVec) {
#pragma unroll
        for (int r = 0; r < S; ++r) {
            unsigned al[kDw];                            // the row's bytes from the block's first one on
#pragma unroll
            for (int i = 0; i < kDw; ++i) al[i] = __builtin_amdgcn_alignbyte(i + 1 < kDw ? raw[r][i + 1] : 0u, raw[r][i], sh);
#pragma unroll
            for (int c = 0; c < S; ++c) {
                const int wd = (3 * c) / 4, k = (3 * c) % 4;
                unsigned v = al[wd] >> (8 * k);
                if (k >= 2) v |= (wd + 1 < kDw ? al[wd + 1] : 0u) << (32 - 8 * k);
                pix[r][c] = v & 0xffffffu;
            }
        }
    }
    while (base < m_end) {
        if (valid) apply_list<S, S>(s_marks, s_boxes, total, px, py, pix);
        __syncthreads();                                 // everyone is done with the list and the counts before the next chunk rewrites them
        base += kCullChunk;
        if (base < m_end) {
            bx = uint2{0, 0};
            if (base + tid < m_end) bx = boxes[base + tid];
            total = cull(base, bx);
        }
    }

    // ---- the average: B and R summed side by side in 16-bit fields (16 x 255 < 2^16), G in its own word
    unsigned rb = 0, gs = 0;
#pragma unroll
    for (int r = 0; r < S; ++r)
#pragma unroll
        for (int c = 0; c < S; ++c) { rb += pix[r][c] & 0xff00ffu; gs += pix[r][c] & 0xff00u; }
    const unsigned D = scale_round<S>(rb & 0xffffu) | (scale_round<S>(gs >> 8) << 8) | (scale_round<S>(rb >> 16) << 16);

    // ---- the stores.  No thread has left: every lane takes part in the cross-lane moves, `valid` guards the stores alone.  kVec: wo
    // % 4 == 0, so the four threads of a quad (q = 0..3, X - q a multiple of 4) are all inside the frame or all outside
    const int q = threadIdx.x & 3;
    if (kOut == OUT_BGR) {
        uint8_t* dp = a.dst + (((size_t)frame * ho + Y) * wo + X) * 3;
        if (kVec) {
            const unsigned nxt = __shfl_down(D, 1);      // the quad's 12 bytes as three dwords, one from each of its first three threads
            if (valid && q < 3) *reinterpret_cast<unsigned*>(dp + q) = (D >> (8 * q)) | (nxt << (24 - 8 * q));
        } else if (valid) {
            dp[0] = (uint8_t)D; dp[1] = (uint8_t)(D >> 8); dp[2] = (uint8_t)(D >> 16);
        }
    } else {                                             // wo, ho even: the three other pixels of a valid pixel's 2 x 2 block are valid
        uint8_t* f = a.dst + (size_t)frame * (size_t)a.frame_stride;
        uint8_t* yp = f + (size_t)Y * a.pitch_y + X;
        const size_t crow = (size_t)(Y >> 1) * a.pitch_c;
        const unsigned y = enc_luma(a, D);
        const unsigned uv = enc_chroma(a, D, __shfl_xor(D, 1), __shfl_xor(D, 32), __shfl_xor(D, 33));
        const bool chroma = valid && !(threadIdx.x & 1) && !(threadIdx.y & 1);               // the block's top-left thread stores it
        if (kVec) {
            const unsigned y4 = y | (__shfl_down(y, 1) << 8) | (__shfl_down(y, 2) << 16) | (__shfl_down(y, 3) << 24);
            const unsigned uv1 = __shfl_down(uv, 2);     // the next block's
            if (valid && q == 0) *reinterpret_cast<unsigned*>(yp) = y4;
            if (chroma && q == 0) {
                if (kOut == OUT_NV12) {
                    *reinterpret_cast<unsigned*>(f + a.off_u + crow + X) = uv | (uv1 << 16);  // U0 V0 U1 V1
                } else {
                    *reinterpret_cast<unsigned short*>(f + a.off_u + crow + (X >> 1)) = (unsigned short)((uv & 0xff) | ((uv1 & 0xff) << 8));
                    *reinterpret_cast<unsigned short*>(f + a.off_v + crow + (X >> 1)) = (unsigned short)((uv >> 8) | (uv1 & 0xff00));
                }
            }
        } else {
            if (valid) *yp = (uint8_t)y;
            if (chroma) {
                if (kOut == OUT_NV12) {
                    uint8_t* pc = f + a.off_u + crow + X;
                    pc[0] = (uint8_t)uv; pc[1] = (uint8_t)(uv >> 8);
                } else {
                    f[a.off_u + crow + (X >> 1)] = (uint8_t)uv;
                    f[a.off_v + crow + (X >> 1)] = (uint8_t)(uv >> 8);
                }
            }
        }
    }
}

bool render_vector_path_ok(const RenderArgs& a) {
    const uintptr_t s = reinterpret_cast<uintptr_t>(a.src), d = reinterpret_cast<uintptr_t>(a.dst);
    if (a.w % 4 || s % 4 || d % 4) return false;         // (rows and frames of packed BGR are then multiples of 4 bytes)
    if (a.out == OUT_BGR) return true;
    if (a.pitch_y % 4) return false;
    if (a.n > 1 && a.frame_stride % 4) return false;
    if (a.out == OUT_NV12) return a.off_u % 4 == 0 && a.pitch_c % 4 == 0;
    return a.off_u % 2 == 0 && a.off_v % 2 == 0 && a.pitch_c % 2 == 0;
}

template <bool kVec>
static void launch_render_out(const RenderArgs& a, dim3 grid, dim3 block, hipStream_t s) {
    if (a.out == OUT_BGR) hipLaunchKernelGGL((render_kernel<kVec, OUT_BGR>), grid, block, 0, s, a);
    else if (a.out == OUT_NV12) hipLaunchKernelGGL((render_kernel<kVec, OUT_NV12>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((render_kernel<kVec, OUT_I420>), grid, block, 0, s, a);
}

hipError_t launch_render(const RenderArgs& a, hipStream_t s, int* vec_out) {
    const bool vec = render_vector_path_ok(a);
    const dim3 grid((unsigned)((a.w + 127) / 128), (unsigned)((a.h + 15) / 16), (unsigned)a.n), block(32, 8);
    if (vec) launch_render_out<true>(a, grid, block, s);
    else launch_render_out<false>(a, grid, block, s);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess && vec_out) *vec_out = vec ? 1 : 0;
    return e;
}

// the scaled pass stores what render_kernel stores, at the OUTPUT's width: the same rule with a.w / scale in the place of a.w (the
// source rows are then multiples of 4 bytes too)
bool render_scaled_vector_path_ok(const RenderArgs& a, int scale) {
    RenderArgs o = a;
    o.w = a.w / scale;
    o.h = a.h / scale;
    return render_vector_path_ok(o);
}

template <int S, bool kVec>
static void launch_render_scaled_out(const RenderArgs& a, dim3 grid, dim3 block, hipStream_t s) {
    if (a.out == OUT_BGR) hipLaunchKernelGGL((render_scaled_kernel<S, kVec, OUT_BGR>), grid, block, 0, s, a);
    else if (a.out == OUT_NV12) hipLaunchKernelGGL((render_scaled_kernel<S, kVec, OUT_NV12>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((render_scaled_kernel<S, kVec, OUT_I420>), grid, block, 0, s, a);
}

template <int S>
static void launch_render_scaled_vec(const RenderArgs& a, bool vec, dim3 grid, dim3 block, hipStream_t s) {
    if (vec) launch_render_scaled_out<S, true>(a, grid, block, s);
    else launch_render_scaled_out<S, false>(a, grid, block, s);
}

hipError_t launch_render_scaled(const RenderArgs& a, int scale, hipStream_t s, int* vec_out) {
    if (scale < 2 || scale > kRenderMaxScale || a.w % scale || a.h % scale) return hipErrorInvalidValue;      // (pa_render_scaled has refused these)
    const bool vec = render_scaled_vector_path_ok(a, scale);
    const dim3 grid((unsigned)((a.w / scale + 31) / 32), (unsigned)((a.h / scale + 7) / 8), (unsigned)a.n), block(32, 8);
    if (scale == 2) launch_render_scaled_vec<2>(a, vec, grid, block, s);
    else if (scale == 3) launch_render_scaled_vec<3>(a, vec, grid, block, s);
    else launch_render_scaled_vec<4>(a, vec, grid, block, s);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess && vec_out) *vec_out = vec ? 1 : 0;
    return e;
}

}  // namespace padel
