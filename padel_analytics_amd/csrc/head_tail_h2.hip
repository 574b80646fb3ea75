// The tail of every Detect / Pose head of an h2 model in ONE launch: the last 1x1 convs of the box, class and keypoint branches
// (model.22.cv2/cv3/cv4.l.2) and the decode of their outputs — candidates straight from the branches' h2 activations, no head map.
//
// Why.  The three convs have K = 2 .. 6 k-steps; on the tap kernel (conv_tap_h2.hip) every k-step is an HBM round trip behind
// wait_vm<0> + s_barrier, a 192 -> 1 class conv runs a 32-channel tile for one channel, and the fp32 map they write
// ([64 + nc + nk] floats per anchor) is a pure intermediate: decode_kernel reads the class logits of every anchor, the box logits of
// the few that pass `conf`, nms_kernel the keypoints of the kept ones.  Here a wave owns a FRAGMENT of 16 anchors, requests every
// activation operand of the three convs up front (at most 10 k-steps x (h + m) x 16 bytes per lane: no LDS staging, no barrier),
// and the maps never reach HBM.
//
// Same numbers.  Per output the products are those of conv_tap_h2.hip in the same order — per k-step cross += wh * am,
// cross += wm * ah (absent in the two-product form), part += wh * ah, one flush (K <= 9), h2_conv_value with the op's bias and
// inverse row scale; the lanes of the absent group of a cin % 32 == 16 tail chunk contribute zeros — in the same MFMA operand
// placement: lane (lr, lq) feeds channels 8 lq .. 8 lq + 7 of a chunk of anchor lr and owns outputs 4 lq .. 4 lq + 3 of it.
// Scores, arg-max, class filter, DFL and dist2bbox are the expressions of decode_kernel (decode_math.h).  The order of the
// candidate list differs (as it does between two runs of decode_kernel: one atomic per wave); nms_kernel's sort key carries the
// anchor index, not the slot.
//
// Weights: a workgroup walks fragments of ONE level (HeadTailArgs::wg_end) and stages that level's three weight matrices, biases
// and row scales in LDS once, the planes in MFMA operand order [fragment][k-step][h | m][lane][16 B] (conflict-free 16-byte reads).
// Box logits go through a per-wave LDS transposition so that lane (lr, s) holds the 16 bins of side s of anchor lr.
// Keypoints: the nk raw values of a passing anchor are written to its row of the head map, where nms_kernel looks for them.
#include "h2_common.h"
#include "decode_math.h"
#include <algorithm>

namespace padel {

namespace {

constexpr int kHtWaves = 4;
constexpr int kHtClsFrags = 5;            // class fragments held in registers: nc <= 80
constexpr int kHtKptFrags = 4;            // nk <= 64
constexpr int kHtRow = 68;                // floats per anchor row of the box transposition (64 + 4: rows 16 bytes apart in the banks)
constexpr size_t kHtMaxLds = 160 * 1024;

constexpr size_t ht_conv_lds(int n16, int K, int P) { return (size_t)n16 * K * P * 1024 + (size_t)n16 * 16 * 8; }

// weights of one conv -> LDS in operand order, then bias[npad] and oscale[npad]
template <int K, int P>
__device__ __forceinline__ void ht_stage(const HeadTailConv& cv, char* dst, int tid) {
    const char* wsrc = reinterpret_cast<const char*>(cv.w);
    const int units = cv.n16 * K * P * 64;
    for (int u = tid; u < units; u += 64 * kHtWaves) {
        const int ln = u & 63, t = u >> 6;
        const int p = t % P, k = (t / P) % K, j = t / (P * K);
        const char* src = wsrc + ((size_t)(j * 16 + (ln & 15)) * (K * 128) + k * 128 + p * 64 + (ln >> 4) * 16);
        *reinterpret_cast<u32x4*>(dst + (size_t)u * 16) = *reinterpret_cast<const u32x4*>(src);
    }
    float* bs = reinterpret_cast<float*>(dst + (size_t)units * 16);
    const int npad = cv.n16 * 16;
    for (int u = tid; u < npad; u += 64 * kHtWaves) { bs[u] = cv.bias[u]; bs[npad + u] = cv.oscale[u]; }
}

// every activation operand of one conv for this lane: chunk k of anchor m, K slots 8 lq .. 8 lq + 7 (h plane, m plane 32 bytes on)
template <int K>
__device__ __forceinline__ void ht_load(const HeadTailConv& cv, int m, int lq, h16x8 (&ah)[K], h16x8 (&am)[K]) {
    const float* p = cv.in + ((long long)m * cv.in_cs + cv.in_choff + (lq >> 1) * 16 + (lq & 1) * 4);
    const bool absent = (cv.cin & 16) && lq >= 2;          // last chunk of a cin % 32 == 16 layer: its second group does not exist
#pragma unroll
    for (int k = 0; k < K; ++k) {
        f32x4 h = {0.f, 0.f, 0.f, 0.f}, mm = h;
        if (!(k == K - 1 && absent)) {
            h = *reinterpret_cast<const f32x4*>(p + k * 32);
            mm = *reinterpret_cast<const f32x4*>(p + k * 32 + 8);
        }
        ah[k] = __builtin_bit_cast(h16x8, h);
        am[k] = __builtin_bit_cast(h16x8, mm);
    }
}

// outputs 16 j + 4 lq .. + 3 of this lane's anchor: the k-steps of conv_tap_h2.hip, one flush, h2_conv_value
template <int K, bool WS>
__device__ __forceinline__ f32x4 ht_frag(const char* wl, const float* bs, int npad, int j, int lane, const h16x8 (&ah)[K], const h16x8 (&am)[K]) {
    constexpr int P = WS ? 1 : 2;
    const char* wj = wl + ((size_t)j * K * P * 64 + lane) * 16;
    f32x4 cross = {0.f, 0.f, 0.f, 0.f}, part = cross, acc = cross;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const h16x8 wh = __builtin_bit_cast(h16x8, *reinterpret_cast<const f32x4*>(wj + (k * P) * 1024));
        cross = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, am[k], cross, 0, 0, 0);
        if constexpr (!WS) {
            const h16x8 wm = __builtin_bit_cast(h16x8, *reinterpret_cast<const f32x4*>(wj + (k * P + 1) * 1024));
            cross = __builtin_amdgcn_mfma_f32_16x16x32_f16(wm, ah[k], cross, 0, 0, 0);
        }
        part = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, ah[k], k == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : part, 0, 0, 0);
    }
    acc += part;
    const int co0 = j * 16 + (lane >> 4) * 4;
    const f32x4 b = *reinterpret_cast<const f32x4*>(bs + co0), sc = *reinterpret_cast<const f32x4*>(bs + npad + co0);
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = h2_conv_value(cross[r], acc[r], sc[r], b[r]);
    return v;
}

__device__ __forceinline__ void ht_wave_sync() {          // this wave's LDS writes are visible to its other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace

template <int K2, int K3, int K4, bool WS>
__global__ void __launch_bounds__(64 * kHtWaves, K2 + K3 + K4 <= 10 ? 3 : 2) head_tail_h2_kernel(const HeadTailArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ht_lds[];
    constexpr int P = WS ? 1 : 2;
    constexpr int K4A = K4 > 0 ? K4 : 1;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = blockIdx.x;
    const int l = bid >= a.wg_end[1] ? 2 : bid >= a.wg_end[0] ? 1 : 0;
    const int wg0 = l == 2 ? a.wg_end[1] : l == 1 ? a.wg_end[0] : 0, nwg = (l == 2 ? a.wg_end[2] : l == 1 ? a.wg_end[1] : a.wg_end[0]) - wg0;
    // (static indices and selects: a dynamic index into the kernel arguments would move them to scratch)
    const HeadLevel lv = l == 2 ? a.d.lv[2] : l == 1 ? a.d.lv[1] : a.d.lv[0];
    const HeadTailConv cbox = l == 2 ? a.cv[2][0] : l == 1 ? a.cv[1][0] : a.cv[0][0];
    const HeadTailConv ccls = l == 2 ? a.cv[2][1] : l == 1 ? a.cv[1][1] : a.cv[0][1];
    const HeadTailConv ckpt = l == 2 ? a.cv[2][2] : l == 1 ? a.cv[1][2] : a.cv[0][2];
    const int nf3 = ccls.n16, nf4 = K4 > 0 ? ckpt.n16 : 0;
    char* const wbox = ht_lds;
    char* const wcls = wbox + ht_conv_lds(cbox.n16, K2, P);
    char* const wkpt = wcls + ht_conv_lds(nf3, K3, P);
    float* const tr = reinterpret_cast<float*>(wkpt + ht_conv_lds(nf4, K4A, P)) + wave * (16 * kHtRow);
    const float* const bbox = reinterpret_cast<const float*>(wbox + (size_t)cbox.n16 * K2 * P * 1024);
    const float* const bcls = reinterpret_cast<const float*>(wcls + (size_t)nf3 * K3 * P * 1024);
    const float* const bkpt = reinterpret_cast<const float*>(wkpt + (size_t)nf4 * K4A * P * 1024);
    ht_stage<K2, P>(cbox, wbox, tid);
    ht_stage<K3, P>(ccls, wcls, tid);
    if constexpr (K4 > 0) ht_stage<K4, P>(ckpt, wkpt, tid);
    __syncthreads();

    const int HW = lv.H * lv.W;
    const int M = a.d.B * HW;
    const int nfrag = (M + 15) >> 4;
    const int nc = a.d.nc, nk = a.d.nk;
    for (int f = (bid - wg0) * kHtWaves + wave; f < nfrag; f += nwg * kHtWaves) {
        const int m_ = f * 16 + lr;
        const bool valid = m_ < M;
        const int m = valid ? m_ : M - 1;              // a lane past the end repeats the last anchor and passes nothing
        h16x8 ah2[K2], am2[K2], ah3[K3], am3[K3], ah4[K4A], am4[K4A];
        ht_load<K3>(ccls, m, lq, ah3, am3);
        ht_load<K2>(cbox, m, lq, ah2, am2);
        if constexpr (K4 > 0) ht_load<K4>(ckpt, m, lq, ah4, am4);

        // ---- class logits, score: max over sigmoid == sigmoid of the max logit
        float cl[kHtClsFrags][4];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < kHtClsFrags; ++j) {
            if (j < nf3) {
                const f32x4 v = ht_frag<K3, WS>(wcls, bcls, nf3 * 16, j, lane, ah3, am3);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    cl[j][r] = v[r];
                    if (j * 16 + lq * 4 + r < nc) mx = fmaxf(mx, v[r]);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float score = sigmoidf_(mx);
        bool pass = valid && score > a.d.conf;         // the same in the four lanes of an anchor
        if (__builtin_amdgcn_ballot_w64(pass) == 0ull) continue;
        // arg-max in sigmoid space, first index wins (torch.max); class filter
        int cls = 0x7fffffff;
        if (pass) {
#pragma unroll
            for (int j = 0; j < kHtClsFrags; ++j) {
                if (j < nf3) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int c = j * 16 + lq * 4 + r;
                        if (c < nc && c < cls && sigmoidf_(cl[j][r]) == score) cls = c;
                    }
                }
            }
        }
        cls = min(cls, __shfl_xor(cls, 16));
        cls = min(cls, __shfl_xor(cls, 32));
        if (pass && a.d.n_classes > 0) {
            bool ok = false;
            for (int k = 0; k < a.d.n_classes; ++k) ok |= (a.d.classes[k] == cls);
            pass = ok;
        }
        if (__builtin_amdgcn_ballot_w64(pass) == 0ull) continue;

        // ---- box logits -> lane (lr, s) gets the 16 bins of side s of anchor lr -> DFL, dist2bbox
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 v = ht_frag<K2, WS>(wbox, bbox, 64, j, lane, ah2, am2);
            *reinterpret_cast<f32x4*>(tr + lr * kHtRow + j * 16 + lq * 4) = v;
        }
        ht_wave_sync();
        float bins[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(tr + lr * kHtRow + lq * 16 + q * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) bins[q * 4 + r] = t[r];
        }
        ht_wave_sync();                                // (the next fragment of this wave overwrites the rows)
        const float side = dfl_expect(bins);
        float d[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) d[s] = __shfl(side, lr + 16 * s);
        const int b = m / HW, pix = m - b * HW;
        float bx[4];
        dfl_box(d, pix, lv.W, lv.stride, bx);

        // ---- stream compaction, one atomic per wave and image (a fragment may straddle images)
        const bool mine = pass && lq == 0;
        unsigned long long rem = __builtin_amdgcn_ballot_w64(mine);
        while (rem) {
            const int first = __builtin_ctzll(rem);
            const int bb = __shfl(b, first);
            const bool now = mine && b == bb;
            const unsigned long long mk = __builtin_amdgcn_ballot_w64(now);
            int base = 0;
            if (lane == first) base = atomicAdd(&a.d.cand_cnt[bb], __builtin_popcountll(mk));
            base = __shfl(base, first);
            if (now) {
                const int slot = base + __builtin_popcountll(mk & ((1ull << lane) - 1ull));
                float* o = a.d.cand + ((long long)bb * a.d.A + slot) * 6;
                o[0] = bx[0]; o[1] = bx[1]; o[2] = bx[2]; o[3] = bx[3]; o[4] = score; o[5] = (float)cls;
                a.d.cand_idx[(long long)bb * a.d.A + slot] = lv.anchor0 + pix;
            }
            rem &= ~mk;
        }

        // ---- keypoints of the passing anchors into their row of the head map
        if constexpr (K4 > 0) {
            float* const hk = const_cast<float*>(lv.buf) + ((long long)m * a.d.cs + 64 + nc);
            for (int j = 0; j < nf4; ++j) {
                const f32x4 v = ht_frag<K4, WS>(wkpt, bkpt, nf4 * 16, j, lane, ah4, am4);
                if (pass) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int c = j * 16 + lq * 4 + r;
                        if (c < nk) hk[c] = v[r];
                    }
                }
            }
        }
    }
}

__global__ void head_tail_zero_kernel(int32_t* p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

namespace {

struct HtShape { int k3, k4, nf3, nf4; bool ok; };

HtShape ht_shape(const HeadTailArgs& a) {
    HtShape s{0, 0, 0, 0, false};
    const bool pose = a.d.nk > 0;
    for (int l = 0; l < 3; ++l)
        for (int c = 0; c < 3; ++c) {
            const HeadTailConv& v = a.cv[l][c];
            if (c == 2 && !pose) { if (v.in) return s; continue; }
            const HeadTailConv& v0 = a.cv[0][c];
            if (!v.in || !v.w || !v.bias || !v.oscale || v.cin < 16 || (v.cin & 15) || ((v.in_cs | v.in_choff) & 15) || v.cin != v0.cin || v.n16 != v0.n16)
                return s;
        }
    const auto ksteps = [](int cin) { return (cin + 31) >> 5; };
    s.k3 = ksteps(a.cv[0][1].cin); s.nf3 = a.cv[0][1].n16;
    s.k4 = pose ? ksteps(a.cv[0][2].cin) : 0; s.nf4 = pose ? a.cv[0][2].n16 : 0;
    if (ksteps(a.cv[0][0].cin) != 2 || a.cv[0][0].n16 != 4) return s;
    if (s.k3 != 2 && s.k3 != 3 && s.k3 != 4 && s.k3 != 6 && s.k3 != 8) return s;
    if (a.d.nc < 1 || s.nf3 < 1 || s.nf3 > kHtClsFrags || s.nf3 * 16 < a.d.nc) return s;
    if (pose && (s.k4 != 2 || s.nf4 < 1 || s.nf4 > kHtKptFrags || s.nf4 * 16 < a.d.nk)) return s;
    if (a.d.cs < 64 + a.d.nc + a.d.nk) return s;
    s.ok = true;
    return s;
}

size_t ht_lds_bytes(const HtShape& s, bool ws) {
    const int P = ws ? 1 : 2;
    return ht_conv_lds(4, 2, P) + ht_conv_lds(s.nf3, s.k3, P) + ht_conv_lds(s.nf4, s.k4 > 0 ? s.k4 : 1, P) + (size_t)kHtWaves * 16 * kHtRow * 4;
}

typedef void (*HtKernel)(const HeadTailArgs);
template <int K3>
HtKernel ht_pick(int k4, bool ws) {
    if (k4) return ws ? head_tail_h2_kernel<2, K3, 2, true> : head_tail_h2_kernel<2, K3, 2, false>;
    return ws ? head_tail_h2_kernel<2, K3, 0, true> : head_tail_h2_kernel<2, K3, 0, false>;
}
HtKernel ht_kernel(int k3, int k4, bool ws) {
    switch (k3) {
        case 2: return ht_pick<2>(k4, ws);
        case 3: return ht_pick<3>(k4, ws);
        case 4: return ht_pick<4>(k4, ws);
        case 6: return ht_pick<6>(k4, ws);
        case 8: return ht_pick<8>(k4, ws);
    }
    return nullptr;
}

}  // namespace

bool head_tail_h2_supported(const HeadTailArgs& a) {
    const HtShape s = ht_shape(a);
    return s.ok && ht_lds_bytes(s, a.w_single != 0) <= kHtMaxLds;
}

hipError_t init_head_tail_kernels() {
    static const int k3s[] = {2, 3, 4, 6, 8};
    for (int k3 : k3s)
        for (int k4 = 0; k4 <= 2; k4 += 2)
            for (int ws = 0; ws < 2; ++ws) {
                const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ht_kernel(k3, k4, ws != 0)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHtMaxLds);
                if (e != hipSuccess) return e;
            }
    return hipSuccess;
}

hipError_t launch_head_tail_h2(const HeadTailArgs& a_in, hipStream_t s) {
    const HtShape sh = ht_shape(a_in);
    const bool ws = a_in.w_single != 0;
    const size_t lds = ht_lds_bytes(sh, ws);
    if (!sh.ok || lds > kHtMaxLds) return hipErrorNotSupported;
    HeadTailArgs a = a_in;
    static int ncu = 0;
    if (!ncu) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        ncu = n;
    }
    // workgroups per level in proportion to its fragments, three per CU in all (the VGPR budget of the widest instantiation)
    long long frags[3], total = 0;
    for (int l = 0; l < 3; ++l) { frags[l] = ((long long)a.d.B * a.d.lv[l].H * a.d.lv[l].W + 15) / 16; total += frags[l]; }
    if (total < 1) return hipErrorInvalidValue;
    const long long budget = (long long)ncu * 3;
    int end = 0;
    for (int l = 0; l < 3; ++l) {
        long long w = (budget * frags[l] + total - 1) / total;
        w = std::min(w, (frags[l] + kHtWaves - 1) / kHtWaves);
        end += (int)std::max(w, 1ll);
        a.wg_end[l] = end;
    }
    hipLaunchKernelGGL(head_tail_zero_kernel, dim3((a.d.B + 255) / 256), dim3(256), 0, s, a.d.cand_cnt, a.d.B);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ht_kernel(sh.k3, sh.k4, ws), dim3(end), dim3(64 * kHtWaves), lds, s, a);
    return hipGetLastError();
}

}  // namespace padel
