// K3/K4 "h2" — the fp32 convolutions on the F16 matrix pipe with THREE products per operand pair (h2_common.h).
//
// Activations arrive in HBM as fp16 pairs (x ~ h + m / 2048, 16-channel groups of 64 bytes [h | m]) written by their
// producer's epilogue, weights as pre-split planes [Npad][k-step][h | m][32].  This file is the implicit-GEMM TAP
// kernel family for them — stride-2 3x3, 1x1 (optionally absorbing a preceding nn.Upsample(2)) and whatever stride-1
// 3x3 the patch kernel (conv_patch_h2.hip) does not take.  It is the machine of conv_tap_bx3.hip (buffer-addressed
// LDS-DMA ring with prefetch distance 1, XOR-swizzled 64-byte rows, one raw barrier per k-step, XCD-aware tile map)
// with the in-register operand split REMOVED: sub-row A0 of a k-step is the h plane of its 32 channels, A1 the m plane,
// both fetched with the same lane offsets (the lane that fills 16-byte slot s of a row fetches K slots 8s..8s+7: group
// s >> 1, half s & 1 of the 128-byte chunk), and a k-step is 3 x MF x NF v_mfma_f32_16x16x32_f16:
//     cross += wh * am;   cross += wm * ah;   part += wh * ah;          part -> acc once per 9-step block (two-level)
// cin % 32 == 16: the 3x3 tail block pairs TAPS (K slots 0-15 = the 16 channels at tap 2t, 16-31 = at tap 2t+1: the
// lanes of slots 2, 3 of a row fetch from the second tap's pixel); the 1x1 runs its last k-step with the lanes of the
// absent group switched off (out-of-range offsets -> zeros).
#include "h2_tap.h"

namespace padel {

// =====================================================================================================  3x3
template <int WM, int WN, int MF, int NF, bool WS = false>
__global__ void __launch_bounds__(64 * WM * WN, MF * NF <= 6 ? 3 : 2) conv_h2_kernel(const ConvArgs a) {
    PADEL_H2T_GEOMETRY()
    unsigned voffA[AP][9];
#pragma unroll
    for (int p = 0; p < AP; ++p) {
        int m = m0 + srow + RP * p;
        const bool rv = m < a.M;
        if (!rv) m = m0;
        const int n = fastdiv(m, a.howo_magic, a.howo_shift);
        const int rem = m - n * HoWo;
        const int oy = fastdiv(rem, a.wo_magic, a.wo_shift);
        const int ox = rem - oy * a.Wo;
        const long long lin = ((long long)n * a.H + oy * a.stride) * a.W + ox * a.stride;
        const unsigned off = (unsigned)((lin - lin0) * a.in_cs * 4) + slot_b;
        bool vy[3], vx[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            vy[d] = rv && (unsigned)(oy * a.stride - 1 + d) < (unsigned)a.H;
            vx[d] = (unsigned)(ox * a.stride - 1 + d) < (unsigned)a.W;
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) voffA[p][t] = (vy[h2_tap_ky(t)] && vx[h2_tap_kx(t)]) ? off : kOORh;
    }
    const i32x4 rsrcA = make_rsrc(a.in + ((lin0 - (a.W + 1)) * a.in_cs + a.in_choff));
    unsigned tapoff[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) tapoff[t] = __builtin_amdgcn_readfirstlane((unsigned)(((h2_tap_ky(t) * a.W + h2_tap_kx(t)) * a.in_cs) * 4));
    // K walk: nfull 32-channel chunks x 9 taps, then — for cin % 32 == 16 — a TAIL block of 5 steps that pair taps
    const int nfull = a.cin >> 5;
    PADEL_H2T_WEIGHTS(nfull * 9 + (half_tail ? 5 : 0))

    unsigned s_chunk = 0, s_kb = 0;
#define PADEL_H2T_REQ_FULL(SR_, CH_, KB_, T_)                                                                      \
    PADEL_H2T_DMA_R(rsrcA, SR_, (CH_) + tapoff[T_], KB_, voffA[0][T_], voffA[AP - 1][T_])
    // tail step JT_: lanes of slots 0, 1 fetch the group's parts at tap 2 JT_, lanes of slots 2, 3 at tap 2 JT_ + 1 (their
    // offsets carry + 64 for "second group of a chunk": taken back out; the tap distance goes in instead)
    // (column-major taps: the second tap of a pair may lie BEFORE the first in memory — the scalar offset carries the smaller
    //  of the two tap offsets, each lane group adds its own distance: lane offsets stay non-negative)
#define PADEL_H2T_TB(JT_) (2 * (JT_) + 1 < 9 ? 2 * (JT_) + 1 : 8)
#define PADEL_H2T_TMIN(JT_) min(tapoff[2 * (JT_)], tapoff[PADEL_H2T_TB(JT_)])
#define PADEL_H2T_TV(P_, JT_)                                                                                      \
    (sc_hi ? (2 * (JT_) + 1 < 9 ? voffA[P_][PADEL_H2T_TB(JT_)] + (tapoff[PADEL_H2T_TB(JT_)] - PADEL_H2T_TMIN(JT_)) - 64u : kOORh) \
           : voffA[P_][2 * (JT_)] + (tapoff[2 * (JT_)] - PADEL_H2T_TMIN(JT_)))
#define PADEL_H2T_REQ_TAIL(SR_, CH_, KB_, JT_)                                                                     \
    do {                                                                                                          \
        const unsigned v0_ = PADEL_H2T_TV(0, JT_), v1_ = PADEL_H2T_TV(AP - 1, JT_);                                \
        PADEL_H2T_DMA_R(rsrcA, SR_, (CH_) + PADEL_H2T_TMIN(JT_), KB_, v0_, v1_);                                   \
    } while (0)
    bool nxt_tail = false;       // the block after the current full chunk is the tail block

    // step J waits for ITS requests (issued one step earlier), passes the barrier, requests step J + 1 into the stage
    // everybody just finished reading, computes.  Stage = parity of the step inside the block; blocks have odd length
    // (9 / 5), so the two stages swap roles after every block.
#define PADEL_H2T_STEP2(J)                                                                                        \
    do {                                                                                                          \
        wait_vm<0>();                                                                                             \
        __builtin_amdgcn_s_barrier();                                                                             \
        if constexpr ((J) + 1 < 9) {                                                                              \
            PADEL_H2T_REQ_FULL((J) + 1, s_chunk, s_kb + ((J) + 1) * 128u, (J) + 1 < 9 ? (J) + 1 : 0);             \
        } else {                                                                                                  \
            if (nxt_tail) { PADEL_H2T_REQ_TAIL((J) + 1, s_chunk + 128u, s_kb + ((J) + 1) * 128u, 0); }            \
            else if (c + 1 < nfull) { PADEL_H2T_REQ_FULL((J) + 1, s_chunk + 128u, s_kb + ((J) + 1) * 128u, 0); }  \
        }                                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PADEL_H2T_COMPUTE(J, (J) == 0);                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    } while (0)
#define PADEL_H2T_TSTEP2(JT)                                                                                      \
    do {                                                                                                          \
        wait_vm<0>();                                                                                             \
        __builtin_amdgcn_s_barrier();                                                                             \
        if constexpr ((JT) + 1 < 5) { PADEL_H2T_REQ_TAIL((JT) + 1, s_chunk, s_kb + ((JT) + 1) * 128u, (JT) + 1 < 5 ? (JT) + 1 : 0); } \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PADEL_H2T_COMPUTE(JT, (JT) == 0);                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    } while (0)
    if (nfull > 0) { PADEL_H2T_REQ_FULL(0, 0u, 0u, 0); } else { PADEL_H2T_REQ_TAIL(0, 0u, 0u, 0); }
    for (int c = 0; c < nfull; ++c) {
        nxt_tail = half_tail && c == nfull - 1;
        PADEL_H2T_STEP2(0); PADEL_H2T_STEP2(1); PADEL_H2T_STEP2(2); PADEL_H2T_STEP2(3); PADEL_H2T_STEP2(4);
        PADEL_H2T_STEP2(5); PADEL_H2T_STEP2(6); PADEL_H2T_STEP2(7); PADEL_H2T_STEP2(8);
        PADEL_H2T_FLUSH();
        PADEL_H2T_SWAP();
        s_chunk += 128u;
        s_kb += 9u * 128u;
    }
    if (half_tail) {
        PADEL_H2T_TSTEP2(0); PADEL_H2T_TSTEP2(1); PADEL_H2T_TSTEP2(2); PADEL_H2T_TSTEP2(3); PADEL_H2T_TSTEP2(4);
        PADEL_H2T_FLUSH();
    }
    wait_vm<0>();
    PADEL_H2T_FINISH()
#undef PADEL_H2T_STEP2
#undef PADEL_H2T_TSTEP2
#undef PADEL_H2T_REQ_FULL
#undef PADEL_H2T_REQ_TAIL
#undef PADEL_H2T_TV
#undef PADEL_H2T_TMIN
#undef PADEL_H2T_TB
}

// =====================================================================================================  1x1
// UP: the first a.up_c channels (whole 32-channel chunks) are read from a.in2, a map of half the spatial size, at
// [y >> 1][x >> 1] — an nn.Upsample(2) + torch.cat in front of this conv that is never materialised
template <int WM, int WN, int MF, int NF, bool UP, bool WS = false>
__global__ void __launch_bounds__(64 * WM * WN, MF * NF <= 6 ? 3 : 2) conv_h2_1_kernel(const ConvArgs a) {
    PADEL_H2T_GEOMETRY()
    unsigned voffA[AP], voffT[AP], voffU[AP];
    const int H2 = a.H >> 1, W2 = a.W >> 1;
    const long long linU0 = ((long long)n0 * H2 + (oy0 >> 1)) * W2;      // first coarse pixel of the coarse row of m0
#pragma unroll
    for (int p = 0; p < AP; ++p) {
        int m = m0 + srow + RP * p;
        const bool rv = m < a.M;
        if (!rv) m = m0;
        const int n = fastdiv(m, a.howo_magic, a.howo_shift);
        const int rem = m - n * HoWo;
        const int oy = fastdiv(rem, a.wo_magic, a.wo_shift);
        const int ox = rem - oy * a.Wo;
        const long long lin = ((long long)n * a.H + oy * a.stride) * a.W + ox * a.stride;
        voffA[p] = rv ? (unsigned)((lin - lin0) * a.in_cs * 4) + slot_b : kOORh;
        voffT[p] = sc_hi ? kOORh : voffA[p];               // last chunk of a cin % 32 == 16 layer: its second group does not exist
        if constexpr (UP) {
            const long long linU = ((long long)n * H2 + (oy >> 1)) * W2 + (ox >> 1);
            voffU[p] = rv ? (unsigned)((linU - linU0) * a.in2_cs * 4) + slot_b : kOORh;
        }
    }
    (void)voffU; (void)linU0;
    const i32x4 rsrcA = make_rsrc(a.in + (lin0 * a.in_cs + a.in_choff));
    const i32x4 rsrcU = make_rsrc(UP ? a.in2 + (linU0 * a.in2_cs + a.in2_choff) : a.in);
    const unsigned nup = UP ? (unsigned)(a.up_c >> 5) : 0u;
    (void)rsrcU; (void)nup;
    PADEL_H2T_WEIGHTS(nch)
    // requests of chunk K_ into stage SR_: from the coarse map while K_ < nup
#define PADEL_H2T_1REQ(SR_, K_)                                                                                   \
    do {                                                                                                          \
        const unsigned k_ = (K_);                                                                                 \
        if (UP && k_ < nup) {                                                                                     \
            PADEL_H2T_DMA_R(rsrcU, SR_, k_ * 128u, k_ * 128u, voffU[0], voffU[AP - 1]);                            \
        } else if (half_tail && (int)k_ >= nch - 1) {                                                             \
            PADEL_H2T_DMA_R(rsrcA, SR_, k_ * 128u, k_ * 128u, voffT[0], voffT[AP - 1]);                            \
        } else {                                                                                                  \
            PADEL_H2T_DMA_R(rsrcA, SR_, k_ * 128u, k_ * 128u, voffA[0], voffA[AP - 1]);                            \
        }                                                                                                         \
    } while (0)

    unsigned s_k = 0;                         // index of the first k-step of the current 9-step accumulation block
#define PADEL_H2T_1STEP2(J)                                                                                       \
    if ((J) < nb) {                                                                                               \
        wait_vm<0>();                                                                                             \
        __builtin_amdgcn_s_barrier();                                                                             \
        if ((int)(s_k + (J) + 1) < nch) PADEL_H2T_1REQ((J) + 1, s_k + (J) + 1);                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PADEL_H2T_COMPUTE(J, (J) == 0);                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    }
    PADEL_H2T_1REQ(0, 0u);
    for (int k = 0; k < nch; k += 9) {
        const int nb = min(9, nch - k);
        PADEL_H2T_1STEP2(0) PADEL_H2T_1STEP2(1) PADEL_H2T_1STEP2(2) PADEL_H2T_1STEP2(3) PADEL_H2T_1STEP2(4)
        PADEL_H2T_1STEP2(5) PADEL_H2T_1STEP2(6) PADEL_H2T_1STEP2(7) PADEL_H2T_1STEP2(8)
        PADEL_H2T_FLUSH();
        PADEL_H2T_SWAP();
        s_k += 9u;
    }
    wait_vm<0>();
    PADEL_H2T_FINISH()
#undef PADEL_H2T_1STEP2
#undef PADEL_H2T_1REQ
}

template <int WM, int WN, int MF, int NF>
static hipError_t launch_h2t(const ConvArgs& a_in, hipStream_t s) {
    ConvArgs a = a_in;
    constexpr int BM = WM * MF * 16;
    a.n_mtiles = (a.M + BM - 1) / BM;
    a.n_ntiles = (a.n16 + WN * NF - 1) / (WN * NF);
    dim3 grid(8u * (unsigned)((a.n_mtiles + 7) / 8) * (unsigned)a.n_ntiles, 1, 1);
    if (a.ksize == 3) {
        if (a.w_single) hipLaunchKernelGGL((conv_h2_kernel<WM, WN, MF, NF, true>), grid, dim3(64 * WM * WN), 0, s, a);
        else hipLaunchKernelGGL((conv_h2_kernel<WM, WN, MF, NF>), grid, dim3(64 * WM * WN), 0, s, a);
    } else if (a.in2) {
        if (a.w_single) hipLaunchKernelGGL((conv_h2_1_kernel<WM, WN, MF, NF, true, true>), grid, dim3(64 * WM * WN), 0, s, a);
        else hipLaunchKernelGGL((conv_h2_1_kernel<WM, WN, MF, NF, true>), grid, dim3(64 * WM * WN), 0, s, a);
    } else {
        if (a.w_single) hipLaunchKernelGGL((conv_h2_1_kernel<WM, WN, MF, NF, false, true>), grid, dim3(64 * WM * WN), 0, s, a);
        else hipLaunchKernelGGL((conv_h2_1_kernel<WM, WN, MF, NF, false>), grid, dim3(64 * WM * WN), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_conv_h2t(const ConvArgs& a, int tile, hipStream_t s) {
    switch (tile) {
        case 207: return launch_h2t<2, 2, 2, 3>(a, s);    //  64 x  96
        case 220: return launch_h2t<4, 1, 2, 3>(a, s);    // 128 x  48
        case 209: return launch_h2t<4, 1, 2, 4>(a, s);    // 128 x  64
        case 211: return launch_h2t<4, 1, 2, 2>(a, s);    // 128 x  32
        case 213: return launch_h2t<4, 1, 2, 6>(a, s);    // 128 x  96, 4 waves of 2 x 6 fragments
        case 225: return launch_h2t<4, 1, 1, 5>(a, s);    //  64 x  80: the 19-fragment (304-channel) fused pose heads
    }
    return hipErrorNotSupported;
}

}  // namespace padel
