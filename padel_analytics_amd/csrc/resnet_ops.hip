// The three ops a torchvision ResNet-50 needs beyond the conv families (the court-keypoint regressor of
// trackers/keypoints_tracker: conv1 7x7 stride 2, MaxPool2d(3, 2, 1), adaptive average pool + fc + sigmoid).
//   stem7_kernel      : conv1 + folded BatchNorm + ReLU straight from the u8 NHWC4 network input, normalisation through a table
//   maxpool3s2_kernel : MaxPool2d(3, 2, 1) on fp32 or h2 channel slices
//   gap_fc_kernel     : mean over the map, linear layer, sigmoid: n x nout logits and probabilities
// None of them is a hot spot (0.24 GFLOP of 8.2 per frame in the stem; the other two move a few MB): they are written to be
// correct at every border and plain.
#include "h2_common.h"
#include <algorithm>

namespace padel {

// ------------------------------------------------------------------------------ conv1 (7x7 stride 2)
// Implicit GEMM on v_mfma_f32_16x16x4_f32 like stem_mfma_kernel (kernels_misc.hip): K = 7 * 7 * 3 = 147 -> 37 steps of 4.  A wave
// owns 16 output pixels x 64 channels per iteration of a grid-stride loop; the weights ([148][64], one zero row) and the tap
// decode of the 148 K slots sit in LDS, the weights with a row pitch of 80 floats so that the four K rows a step reads fall into
// different banks.  A K slot is (tap, colour): the lane loads the pixel word of its tap from a CLAMPED address (always valid;
// masked afterwards — 37 independent loads per tile) and maps the colour byte through the normalisation table: padding taps
// contribute exact zeros IN NORMALISED SPACE, as Conv2d(padding=3) does behind transforms.Normalize.
constexpr int kStem7K = 148, kStem7Pitch = 80;

__global__ void __launch_bounds__(256) stem7_kernel(const Stem7Args a) {
    __shared__ float wl[kStem7K * kStem7Pitch];
    __shared__ float lut[768];
    __shared__ unsigned tapt[kStem7K];
    for (int i = threadIdx.x; i < kStem7K * 64; i += 256) wl[(i >> 6) * kStem7Pitch + (i & 63)] = a.w[i];
    for (int i = threadIdx.x; i < 768; i += 256) lut[i] = a.lut[i];
    if (threadIdx.x < kStem7K) {
        const int k = threadIdx.x, t = k / 3, c = k - 3 * t, dy = t / 7, dx = t - 7 * dy;
        tapt[k] = k < 147 ? (unsigned)(dy | (dx << 8) | (c << 16) | (1 << 24)) : 0u;      // bit 24: a real slot (147 is padding)
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    f32x4 bias4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bias4[j] = *reinterpret_cast<const f32x4*>(a.bias + j * 16 + lq * 4);
    const int P = a.B * a.Ho * a.Wo;                 // < 2^31 (launch_stem7 checks)
    const int ntiles = (P + 15) / 16;
    const int HoWo = a.Ho * a.Wo;
    const uint32_t* const img0 = reinterpret_cast<const uint32_t*>(a.in);
    bool bad = false;
    for (int tile = blockIdx.x * 4 + wave; tile < ntiles; tile += gridDim.x * 4) {
        const int p = tile * 16 + lr;
        const bool pv = p < P;
        const int pc = pv ? p : 0;
        const int n = (int)((__umulhi((unsigned)pc, a.howo_magic) + (unsigned)pc) >> a.howo_shift);
        const int rem = pc - n * HoWo;
        const int oy = (int)((__umulhi((unsigned)rem, a.wo_magic) + (unsigned)rem) >> a.wo_shift), ox = rem - oy * a.Wo;
        const uint32_t* img = img0 + (long long)n * a.H * a.W;
        uint32_t pxw[37];
        bool okk[37];
#pragma unroll
        for (int kk = 0; kk < 37; ++kk) {
            const unsigned ti = tapt[4 * kk + lq];
            const int iy = oy * 2 - 3 + (int)(ti & 255u), ix = ox * 2 - 3 + (int)((ti >> 8) & 255u);
            okk[kk] = pv && (ti >> 24) != 0u && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const int iyc = min(max(iy, 0), a.H - 1), ixc = min(max(ix, 0), a.W - 1);
            pxw[kk] = img[(long long)iyc * a.W + ixc];
        }
        f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 37; ++kk) {
            const int c = (int)(tapt[4 * kk + lq] >> 16) & 3;
            const float v = lut[c * 256 + (int)((pxw[kk] >> (8 * c)) & 255u)];
            const float av = okk[kk] ? v : 0.0f;
            const float* wrow = wl + (4 * kk + lq) * kStem7Pitch + lr;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[j * 16], av, acc[j], 0, 0, 0);
        }
        if (pv) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = acc[j][r] + bias4[j][r];
                    v[r] = a.act == ACT_RELU ? (x > 0.0f ? x : 0.0f) : x;
                }
                if (a.out_h2) {
                    h16x4 hv, mv;
                    h2_encode4(v, hv, mv, bad);
                    char* op = reinterpret_cast<char*>(a.out) + (long long)p * a.out_cs * 4 + h2_chan_off(a.out_choff + j * 16 + lq * 4);
                    *reinterpret_cast<h16x4*>(op) = hv;
                    *reinterpret_cast<h16x4*>(op + 32) = mv;
                } else {
                    *reinterpret_cast<f32x4*>(a.out + (long long)p * a.out_cs + a.out_choff + j * 16 + lq * 4) = v;
                }
            }
        }
    }
    if (a.out_h2) h2_raise(a.ovf_flag, bad);
}

hipError_t launch_stem7(const Stem7Args& a_in, hipStream_t s) {
    Stem7Args a = a_in;
    if (a.B <= 0 || a.H <= 0 || a.W <= 0 || a.Ho != (a.H + 1) / 2 || a.Wo != (a.W + 1) / 2) return hipErrorInvalidValue;
    if ((long long)a.B * a.Ho * a.Wo >= (1ll << 31) - 16) return hipErrorInvalidValue;
    if ((a.act != ACT_RELU && a.act != ACT_NONE) || !a.lut) return hipErrorNotSupported;
    if (a.out_h2 ? ((a.out_choff | a.out_cs) & 15) : ((a.out_choff | a.out_cs) & 3)) return hipErrorInvalidValue;
    fill_fastdiv((unsigned)(a.Ho * a.Wo), &a.howo_magic, &a.howo_shift);
    fill_fastdiv((unsigned)a.Wo, &a.wo_magic, &a.wo_shift);
    const long long ntiles = ((long long)a.B * a.Ho * a.Wo + 15) / 16;
    const unsigned grid = (unsigned)std::min<long long>((ntiles + 3) / 4, 256 * 3);
    hipLaunchKernelGGL(stem7_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ MaxPool2d(3, 2, 1)
// One thread per output pixel and 4 channels.  Padding is -inf: a tap outside the map is skipped (the centre tap (2y, 2x) always
// exists).  h2 pairs are ordered like every other h2 max-pool (kernels_misc.hip:h2_max): by value h + m / 2048, then by the
// bits of the pair — a total order, the winning PAIR is copied, nothing is re-encoded.
template <bool H2>
__global__ void __launch_bounds__(256) maxpool3s2_kernel(const float* in, int in_cs, int in_choff, float* out, int out_cs, int out_choff,
                                                          int un, int B, int H, int W, int Ho, int Wo) {
    const long long total = (long long)B * Ho * Wo * un;
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= total) return;
    const int u = (int)(i % un);
    long long t = i / un;
    const int x = (int)(t % Wo); t /= Wo;
    const int y = (int)(t % Ho);
    const int n = (int)(t / Ho);
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    unsigned bp[4] = {0u, 0u, 0u, 0u};
    bool first = true;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yy = 2 * y + dy - 1;
        if ((unsigned)yy >= (unsigned)H) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int xx = 2 * x + dx - 1;
            if ((unsigned)xx >= (unsigned)W) continue;
            const long long pix = ((long long)n * H + yy) * W + xx;
            f32x4 v;
            unsigned pk[4] = {0u, 0u, 0u, 0u};
            if constexpr (H2) {
                const char* q = reinterpret_cast<const char*>(in) + pix * in_cs * 4 + h2_chan_off(in_choff + u * 4);
                const uint2 hw = *reinterpret_cast<const uint2*>(q), mw = *reinterpret_cast<const uint2*>(q + 32);      // 4 h halves, 4 m halves
                const unsigned hb[4] = {hw.x & 0xffffu, hw.x >> 16, hw.y & 0xffffu, hw.y >> 16};
                const unsigned mb[4] = {mw.x & 0xffffu, mw.x >> 16, mw.y & 0xffffu, mw.y >> 16};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const _Float16 hh = __builtin_bit_cast(_Float16, (unsigned short)hb[r]), mm = __builtin_bit_cast(_Float16, (unsigned short)mb[r]);
                    v[r] = fmaf((float)mm, kH2InvScale, (float)hh);
                    pk[r] = (hb[r] << 16) | mb[r];
                }
            } else {
                v = *reinterpret_cast<const f32x4*>(in + pix * in_cs + in_choff + u * 4);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool win = first || v[r] > bv[r] || (H2 && v[r] == bv[r] && pk[r] > bp[r]);
                bv[r] = win ? v[r] : bv[r];
                bp[r] = win ? pk[r] : bp[r];
            }
            first = false;
        }
    }
    const long long opix = ((long long)n * Ho + y) * Wo + x;
    if constexpr (H2) {
        const uint2 hw = {(bp[0] >> 16) | (bp[1] & 0xffff0000u), (bp[2] >> 16) | (bp[3] & 0xffff0000u)};
        const uint2 mw = {(bp[0] & 0xffffu) | (bp[1] << 16), (bp[2] & 0xffffu) | (bp[3] << 16)};
        char* q = reinterpret_cast<char*>(out) + opix * out_cs * 4 + h2_chan_off(out_choff + u * 4);
        *reinterpret_cast<uint2*>(q) = hw;
        *reinterpret_cast<uint2*>(q + 32) = mw;
    } else {
        *reinterpret_cast<f32x4*>(out + opix * out_cs + out_choff + u * 4) = bv;
    }
}

hipError_t launch_maxpool3s2(const float* in, int in_cs, int in_choff, float* out, int out_cs, int out_choff,
                             int c, int B, int H, int W, int Ho, int Wo, hipStream_t s, int h2) {
    if (c <= 0 || ((c | in_choff | out_choff | in_cs | out_cs) & 3) || B <= 0 || Ho <= 0 || Wo <= 0) return hipErrorInvalidValue;
    // every output pixel's centre tap lies inside the input map
    if (2 * (Ho - 1) >= H || 2 * (Wo - 1) >= W) return hipErrorInvalidValue;
    const long long total = (long long)B * Ho * Wo * (c / 4);
    if ((total + 255) / 256 >= (1ll << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (h2) hipLaunchKernelGGL(maxpool3s2_kernel<true>, grid, dim3(256), 0, s, in, in_cs, in_choff, out, out_cs, out_choff, c / 4, B, H, W, Ho, Wo);
    else hipLaunchKernelGGL(maxpool3s2_kernel<false>, grid, dim3(256), 0, s, in, in_cs, in_choff, out, out_cs, out_choff, c / 4, B, H, W, Ho, Wo);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ average pool + fc + sigmoid
// One workgroup per image.  Step 1: the mean of every channel over the HW pixels in fp32 — a thread owns 4 channels, adds the
// pixels in order, divides by HW — into LDS (h2 pairs are decoded on the fly).  Step 2: wave w computes outputs w, w + 4, ...:
// each lane runs an fp32 FMA chain over channels lane, lane + 64, ..., the 64 partial sums meet in a butterfly.  The logit
// (sum + bias) and 1 / (1 + expf(-logit)) are both written: the caller scales the probabilities, the tests read the logits.
template <bool H2>
__global__ void __launch_bounds__(256) gap_fc_kernel(const float* in, int in_cs, int in_choff, int c, int HW, const float* w, const float* bias,
                                                      int nout, float* logits, float* probs) {
    __shared__ float mean[kGapFcMaxC];
    const int n = blockIdx.x;
    const float cnt = (float)HW;
    for (int u = threadIdx.x; u < c / 4; u += 256) {
        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < HW; ++p) {
            const long long pix = (long long)n * HW + p;
            f32x4 v;
            if constexpr (H2) {
                const char* q = reinterpret_cast<const char*>(in) + pix * in_cs * 4 + h2_chan_off(in_choff + u * 4);
                v = h2_decode4(*reinterpret_cast<const h16x4*>(q), *reinterpret_cast<const h16x4*>(q + 32));
            } else {
                v = *reinterpret_cast<const f32x4*>(in + pix * in_cs + in_choff + u * 4);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[r] += v[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) mean[u * 4 + r] = sum[r] / cnt;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = wave; o < nout; o += 4) {
        const float* wr = w + (long long)o * c;
        float acc = 0.0f;
        for (int ch = lane; ch < c; ch += 64) acc = fmaf(mean[ch], wr[ch], acc);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
        if (lane == 0) {
            const float z = acc + bias[o];
            logits[(long long)n * nout + o] = z;
            probs[(long long)n * nout + o] = 1.0f / (1.0f + expf(-z));
        }
    }
}

hipError_t launch_gap_fc(const float* in, int in_cs, int in_choff, int c, int B, int HW, const float* w, const float* bias, int nout,
                         float* logits, float* probs, hipStream_t s, int h2) {
    if (c <= 0 || c > kGapFcMaxC || ((c | in_choff | in_cs) & 3) || nout <= 0 || nout > kGapFcMaxOut || B <= 0 || HW <= 0 || !logits || !probs)
        return hipErrorInvalidValue;
    if (h2) hipLaunchKernelGGL(gap_fc_kernel<true>, dim3((unsigned)B), dim3(256), 0, s, in, in_cs, in_choff, c, HW, w, bias, nout, logits, probs);
    else hipLaunchKernelGGL(gap_fc_kernel<false>, dim3((unsigned)B), dim3(256), 0, s, in, in_cs, in_choff, c, HW, w, bias, nout, logits, probs);
    return hipGetLastError();
}

}  // namespace padel
