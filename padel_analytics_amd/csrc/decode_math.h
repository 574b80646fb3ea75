// The arithmetic of the Detect / Pose decode, shared by decode_kernel (postproc.hip) and the fused head tail (head_tail_h2.hip):
// one statement of each expression, so that both kernels round the same way.  Which multiply-add pairs are ONE rounding is
// written out (fmaf) and everything else is kept apart (fp contract off): left to the compiler, decode_kernel — four sides side by
// side, packed math — and the fused kernel — one side per lane — fused different pairs and boxes differed by an ulp.  The pairs
// named here are the ones decode_kernel has always fused: the expectation's accumulation and centre * stride -/+ half size.
#pragma once
#include <hip/hip_runtime.h>

namespace padel {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// DFL: softmax over the 16 bins of one box side, expectation with arange(16)
__device__ __forceinline__ float dfl_expect(float (&v)[16]) {
#pragma clang fp contract(off)
    float m = v[0];
#pragma unroll
    for (int i = 0; i < 16; ++i) m = fmaxf(m, v[i]);
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { v[i] = expf(v[i] - m); sum += v[i]; }
    float e = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) e = fmaf(v[i] / sum, (float)i, e);
    return e;
}

// dist2bbox(xywh=True) * stride, then xywh2xyxy (same op order as upstream), for anchor `pix` of a level W pixels wide
__device__ __forceinline__ void dfl_box(const float (&d)[4], int pix, int W, int stride, float (&bx)[4]) {
#pragma clang fp contract(off)
    const float ax = (float)(pix % W) + 0.5f, ay = (float)(pix / W) + 0.5f;
    const float st = (float)stride;
    const float x1 = ax - d[0], y1 = ay - d[1], x2 = ax + d[2], y2 = ay + d[3];
    const float mx = (x1 + x2) / 2.0f, my = (y1 + y2) / 2.0f;           // cx = mx * st, cy = my * st: never rounded on their own
    const float w = (x2 - x1) * st, hh = (y2 - y1) * st;
    const float hw = w / 2.0f, hhh = hh / 2.0f;
    bx[0] = fmaf(mx, st, -hw); bx[1] = fmaf(my, st, -hhh); bx[2] = fmaf(mx, st, hw); bx[3] = fmaf(my, st, hhh);
}

}  // namespace padel
