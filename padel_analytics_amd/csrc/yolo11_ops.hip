// The two ops YOLO11 adds to the conv families (ultralytics 8.3: C3k2 / C2PSA backbone, depthwise class branch in the head):
//   dwconv3_kernel   : depthwise Conv 3x3 stride 1 pad 1 + bias (BatchNorm folded) + none | SiLU (+ residual) on fp32 or h2 channel slices
//   psa_attn_kernel  : the spatial self-attention of C2PSA's Attention block, softmax_keys((q^T k) * scale) applied to v, per head
// Both are written to be correct at every border and independent of batch and launch shape; neither has been tuned
// (the depthwise conv moves bytes, the attention is ~2 of ~300 GFLOP per frame at yolo11m-pose @ 1280^2).
#include "h2_common.h"
#include <algorithm>

namespace padel {

// ------------------------------------------------------------------------------ depthwise 3x3
// One thread per output pixel and 4 channels.  A tap outside the map is SKIPPED, never read: zero padding contributes nothing to
// the sum, and no address outside the slice's own pixels is formed (stale arena bytes stay unreachable).  The sum
// is one fp32 FMA chain over the taps that exist in the fixed order (ky, kx) row-major, started at zero; then + bias, activation,
// + residual.  A value therefore depends on its own 3x3 neighbourhood alone: not on the batch, not on the launch shape.
template <bool H2>
__device__ __forceinline__ f32x4 dw_load4(const float* base, long long pix, int cs, int ch) {
    if constexpr (H2) {
        const char* q = reinterpret_cast<const char*>(base) + pix * cs * 4 + h2_chan_off(ch);
        return h2_decode4(*reinterpret_cast<const h16x4*>(q), *reinterpret_cast<const h16x4*>(q + 32));
    } else {
        return *reinterpret_cast<const f32x4*>(base + pix * cs + ch);
    }
}

template <bool H2>
__global__ void __launch_bounds__(256) dwconv3_kernel(const DwConvArgs a) {
    const int un = a.C >> 2;
    const long long total = (long long)a.B * a.H * a.W * un;
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    bool bad = false;
    if (i < total) {
        const int u = (int)(i % un);
        long long t = i / un;
        const int x = (int)(t % a.W); t /= a.W;
        const int y = (int)(t % a.H);
        const int n = (int)(t / a.H);
        const int c0 = u * 4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = y + ky - 1;
            if ((unsigned)yy >= (unsigned)a.H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = x + kx - 1;
                if ((unsigned)xx >= (unsigned)a.W) continue;
                const f32x4 v = dw_load4<H2>(a.in, ((long long)n * a.H + yy) * a.W + xx, a.in_cs, a.in_choff + c0);
                const f32x4 w = *reinterpret_cast<const f32x4*>(a.w + (ky * 3 + kx) * a.C + c0);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = fmaf(v[r], w[r], acc[r]);
            }
        }
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + c0);
        const long long pix = ((long long)n * a.H + y) * a.W + x;
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float z = acc[r] + b[r];
            o[r] = a.act == ACT_SILU ? fast_act<ACT_SILU>(z) : z;
        }
        if (a.res) {
            const f32x4 rv = dw_load4<H2>(a.res, pix, a.res_cs, a.res_choff + c0);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] += rv[r];
        }
        if (H2 && !a.out_f32) {
            h16x4 hv, mv;
            h2_encode4(o, hv, mv, bad);
            char* q = reinterpret_cast<char*>(a.out) + pix * a.out_cs * 4 + h2_chan_off(a.out_choff + c0);
            *reinterpret_cast<h16x4*>(q) = hv;
            *reinterpret_cast<h16x4*>(q + 32) = mv;
        } else {
            *reinterpret_cast<f32x4*>(a.out + pix * a.out_cs + a.out_choff + c0) = o;
        }
    }
    if (H2 && !a.out_f32) h2_raise(a.ovf_flag, bad);
}

hipError_t launch_dwconv3(const DwConvArgs& a, hipStream_t s) {
    if (a.C <= 0 || ((a.C | a.in_choff | a.out_choff | a.in_cs | a.out_cs) & 3) || a.B <= 0 || a.H <= 0 || a.W <= 0) return hipErrorInvalidValue;
    if (a.res && ((a.res_choff | a.res_cs) & 3)) return hipErrorInvalidValue;
    if (a.act != ACT_NONE && a.act != ACT_SILU) return hipErrorNotSupported;
    const long long total = (long long)a.B * a.H * a.W * (a.C / 4);
    if ((total + 255) / 256 >= (1ll << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (a.h2) hipLaunchKernelGGL(dwconv3_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dwconv3_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ PSA attention
// out[:, i] = sum_j softmax_j((q_i . k_j) * scale) v_j  per image and head; q_i, k_j: kd = 32 channels, v_j: hd = 64 channels of
// token (pixel) i / j of the qkv buffer, laid out [q of all heads | k of all heads | v of all heads].
//
// Flash-style, fp32 throughout, plain FMA.  A workgroup of 256 threads owns (image, head, 64 query tokens).  It walks the key
// tokens in tiles of 64 IN ORDER, keeping per query a running maximum m, a running sum l and the unnormalised output o:
//     s = (q . k) * scale;  m' = max(m, max_tile s);  p = e^(s - m');  l = l e^(m - m') + sum_tile p;  o = o e^(m - m') + sum_tile p v
// and stores o / l at the end.  The q block (transposed), the k tile (transposed), the v tile and the tile's p matrix sit in LDS
// (row pitch 68 floats: 16-byte aligned rows, neighbouring rows in different banks).  Thread (tq, tk) = (tid / 16, tid % 16)
// computes the 4 x 4 block of s for queries 4 tq .. + 3 and keys 4 tk .. + 3 (FMA chain over the 32 channels in order) and owns
// the output block of the same 4 queries x channels 4 tk .. + 3; the 16 threads of a query row are 16 neighbouring lanes, so the
// row maximum and the row sum are four butterfly steps.  The products p v of a tile are summed from zero in key order and then
// added to o: the rounding error of a 1 600-term sum grows with the tile count, not with the token count.
// Keys past the last token are masked out of the maximum and contribute p = 0 (their LDS rows are zero-filled, never read from
// HBM); query rows past the last token compute on zeros and store nothing.  The sentinel for "no key yet" is -1e30, not -inf:
// e^-(m' - m) through fast_exp_neg stays finite (0) for it.  Nothing here depends on the batch or on the other workgroups:
// one image gives the same bits alone and as part of any batch.
constexpr int kAttnKd = 32, kAttnHd = 64, kAttnBlk = 64, kAttnPitch = 68;
constexpr float kAttnNone = -1.0e30f;

template <bool H2>
__global__ void __launch_bounds__(256) psa_attn_kernel(const AttnArgs a) {
    __shared__ float Qt[kAttnKd * kAttnPitch];        // [channel][query]
    __shared__ float Kt[kAttnKd * kAttnPitch];        // [channel][key]
    __shared__ float Vs[kAttnBlk * kAttnPitch];       // [key][channel]
    __shared__ float Ps[kAttnBlk * kAttnPitch];       // [query][key]
    const int tid = threadIdx.x;
    const int tq = tid >> 4, tk = tid & 15;
    const int q0 = blockIdx.x * kAttnBlk, head = blockIdx.y, n = blockIdx.z;
    const long long img = (long long)n * a.N;
    const int qch = a.q_choff + head * kAttnKd, kch = a.k_choff + head * kAttnKd, vch = a.v_choff + head * kAttnHd;

    // the q block, transposed: element idx = (token, 4 channels)
    for (int idx = tid; idx < kAttnBlk * (kAttnKd / 4); idx += 256) {
        const int tok = idx >> 3, c4 = (idx & 7) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q0 + tok < a.N) v = dw_load4<H2>(a.qkv, img + q0 + tok, a.cs, qch + c4);
#pragma unroll
        for (int r = 0; r < 4; ++r) Qt[(c4 + r) * kAttnPitch + tok] = v[r];
    }

    float m[4], l[4];
    f32x4 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { m[i] = kAttnNone; l[i] = 0.0f; o[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

    const int ntiles = (a.N + kAttnBlk - 1) / kAttnBlk;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int k0 = tile * kAttnBlk;
        __syncthreads();                               // the previous tile's readers of Kt / Vs / Ps are done (first pass: Qt is written)
        for (int idx = tid; idx < kAttnBlk * (kAttnKd / 4); idx += 256) {
            const int tok = idx >> 3, c4 = (idx & 7) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k0 + tok < a.N) v = dw_load4<H2>(a.qkv, img + k0 + tok, a.cs, kch + c4);
#pragma unroll
            for (int r = 0; r < 4; ++r) Kt[(c4 + r) * kAttnPitch + tok] = v[r];
        }
        for (int idx = tid; idx < kAttnBlk * (kAttnHd / 4); idx += 256) {
            const int tok = idx >> 4, c4 = (idx & 15) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k0 + tok < a.N) v = dw_load4<H2>(a.qkv, img + k0 + tok, a.cs, vch + c4);
            *reinterpret_cast<f32x4*>(Vs + tok * kAttnPitch + c4) = v;
        }
        __syncthreads();

        // s[i][j] = q(4 tq + i) . k(4 tk + j): FMA chain over the channels in order
        f32x4 sacc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) sacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int d = 0; d < kAttnKd; ++d) {
            const f32x4 qv = *reinterpret_cast<const f32x4*>(Qt + d * kAttnPitch + 4 * tq);
            const f32x4 kv = *reinterpret_cast<const f32x4*>(Kt + d * kAttnPitch + 4 * tk);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) sacc[i][j] = fmaf(qv[i], kv[j], sacc[i][j]);
        }
        bool kvalid[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) kvalid[j] = k0 + 4 * tk + j < a.N;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float mx = kAttnNone;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sacc[i][j] *= a.scale;
                mx = kvalid[j] ? fmaxf(mx, sacc[i][j]) : mx;
            }
#pragma unroll
            for (int dlt = 1; dlt < 16; dlt <<= 1) mx = fmaxf(mx, __shfl_xor(mx, dlt, 64));
            const float mnew = fmaxf(m[i], mx);
            const float alpha = fast_exp_neg(mnew - m[i]);
            f32x4 p;
            float rs = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                p[j] = kvalid[j] ? fast_exp_neg(mnew - sacc[i][j]) : 0.0f;
                rs += p[j];
            }
#pragma unroll
            for (int dlt = 1; dlt < 16; dlt <<= 1) rs += __shfl_xor(rs, dlt, 64);
            l[i] = fmaf(l[i], alpha, rs);
            m[i] = mnew;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[i][r] *= alpha;
            *reinterpret_cast<f32x4*>(Ps + (4 * tq + i) * kAttnPitch + 4 * tk) = p;
        }
        __syncthreads();

        // this tile's sum_j p[i][j] v[j][4 tk ..]: from zero, keys in order
        f32x4 t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int j4 = 0; j4 < kAttnBlk; j4 += 4) {
            f32x4 pv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) pv[i] = *reinterpret_cast<const f32x4*>(Ps + (4 * tq + i) * kAttnPitch + j4);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const f32x4 vv = *reinterpret_cast<const f32x4*>(Vs + (j4 + jj) * kAttnPitch + 4 * tk);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) t[i][r] = fmaf(pv[i][jj], vv[r], t[i][r]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[i][r] += t[i][r];
    }

    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int tok = q0 + 4 * tq + i;
        if (tok >= a.N) continue;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = o[i][r] / l[i];
        const int ch = a.out_choff + head * kAttnHd + 4 * tk;
        if (H2 && !a.out_f32) {
            h16x4 hv, mv;
            h2_encode4(v, hv, mv, bad);
            char* q = reinterpret_cast<char*>(a.out) + (img + tok) * a.out_cs * 4 + h2_chan_off(ch);
            *reinterpret_cast<h16x4*>(q) = hv;
            *reinterpret_cast<h16x4*>(q + 32) = mv;
        } else {
            *reinterpret_cast<f32x4*>(a.out + (img + tok) * a.out_cs + ch) = v;
        }
    }
    if (H2 && !a.out_f32) h2_raise(a.ovf_flag, bad);
}

hipError_t launch_psa_attn(const AttnArgs& a, hipStream_t s) {
    if (a.kd != kAttnKd || a.hd != kAttnHd) return hipErrorNotSupported;
    if (a.heads <= 0 || a.heads > 65535 || a.B <= 0 || a.B > 65535 || a.N <= 0 || (long long)a.B * a.N >= (1ll << 31)) return hipErrorInvalidValue;
    if ((a.cs | a.out_cs | a.q_choff | a.k_choff | a.v_choff | a.out_choff) & 3) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.N + kAttnBlk - 1) / kAttnBlk), (unsigned)a.heads, (unsigned)a.B);
    if (a.h2) hipLaunchKernelGGL(psa_attn_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(psa_attn_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace padel
