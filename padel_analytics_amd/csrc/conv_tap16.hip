// K3/K4 fp16 — the tap-unrolled LDS-DMA ring (conv_tap.hip) on 16-bit operands: fp16 activations and weights,
// fp32 accumulation on v_mfma_f32_16x16x32_f16 (BASELINE configs[4]: "1920x1080 fp16 ... HBM-bound stress";
// the reference itself runs half=False, players_tracker.py:351-359, so this path reports its own L-inf).
//
// What carries over unchanged from the fp32 kernel is everything that moves bytes: a k-step is still one 64-byte
// run per tile row (now 32 channels instead of 16), the XOR-swizzled LDS image, the 3-/4-stage ring filled by
// `buffer_load_dwordx4 ... offen lds` with per-lane tap offsets whose out-of-image / past-M values are out of range
// (zeros by the raw-buffer range check), the wave-uniform SGPR offsets, the counted vmcnt + one raw s_barrier per
// k-step, the XCD-aware tile map.  A 3x3 accumulation block is one 64-channel chunk (9 taps x 2 halves = 18
// k-steps), cin % 64 == 32 adds the 9-step tail block; the 1x1 kernel walks 32-channel k-steps.
//
// What changes is the arithmetic per byte: a lane's 16-byte fragment is 8 halves = ONE 16x16x32 MFMA (8 passes)
// instead of four 16x16x4 fp32 MFMAs (32 passes), so the matrix pipe has ~16x less work per k-step and the kernel
// lives off instruction issue and HBM.  Consequences built in here:
//   * operands are swapped (A := weights, B := pixels), so a lane ends up with 4 CONSECUTIVE CHANNELS of one pixel:
//     the epilogue does one 8-byte bias load, one 8-byte residual load and one 8-byte store per fragment instead of
//     four scattered 2-byte ones;
//   * single-level accumulation (fp32 accumulators over K <= 5184: the two-level scheme bought parity margin at the
//     fp32 noise floor, irrelevant at fp16 input precision) — no partial set, no flush;
//   * convs that feed the Detect/Pose decode write fp32 (ConvArgs::out_f32): the head maps stay fp32, so DFL
//     softmax / box decode / NMS are the same kernels and the same arithmetic as on the fp32 path.
#include "kernels.h"
#include "conv_prims.h"
#include "act_fast.h"
#include "f16_epilogue.h"
#include <cmath>

namespace padel {

namespace {

constexpr int min_waves16(int nw, int frags) { return nw == 4 ? (frags <= 6 ? 4 : (frags <= 8 ? 3 : 2)) : 2; }

}  // namespace

#define PADEL_T16_DMA(SR_, SA_, SB_, VA0_, VA1_)                                                                  \
    do {                                                                                                          \
        const unsigned sa_ = (SA_), sb_ = (SB_);                                                                  \
        lds_dma<(SR_) * STAGE_B>((VA0_), rsrcA, sa_, lds_wave);                                                   \
        if constexpr (AP >= 2) lds_dma<(SR_) * STAGE_B + RP * 64>((VA1_), rsrcA, sa_, lds_wave);                  \
        if constexpr (BFULL >= 1) lds_dma<(SR_) * STAGE_B + BM * 64>(voffB[0], rsrcB, sb_, lds_wave);             \
        if constexpr (BFULL >= 2) lds_dma<(SR_) * STAGE_B + BM * 64 + RP * 64>(voffB[1], rsrcB, sb_, lds_wave);   \
        if constexpr (BP > BFULL) { if (b_last) lds_dma<(SR_) * STAGE_B + BM * 64 + BFULL * RP * 64>(voffB[BP - 1], rsrcB, sb_, lds_wave); } \
    } while (0)

// fragments of ring stage ST_ -> MF * NF MFMAs (weights as the A operand: D rows = channels, D columns = pixels)
#define PADEL_T16_COMPUTE(ST_)                                                                                    \
    do {                                                                                                          \
        f32x4 A_[MF], B_[NF];                                                                                     \
        _Pragma("unroll") for (int f = 0; f < MF; ++f) A_[f] = *reinterpret_cast<const f32x4*>(a_rd + (ST_) * STAGE + f * 256); \
        _Pragma("unroll") for (int j = 0; j < NF; ++j) B_[j] = *reinterpret_cast<const f32x4*>(b_rd + (ST_) * STAGE + j * 256); \
        __builtin_amdgcn_s_setprio(1);                                                                            \
        _Pragma("unroll") for (int f = 0; f < MF; ++f)                                                            \
            _Pragma("unroll") for (int j = 0; j < NF; ++j)                                                        \
                acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, B_[j]), __builtin_bit_cast(h16x8, A_[f]), acc[f][j], 0, 0, 0); \
        __builtin_amdgcn_s_setprio(0);                                                                            \
    } while (0)

// epilogue: f16_epilogue.h (shared with conv_patch16.hip)

#define PADEL_T16_GEOMETRY(NST_)                                                                                  \
    constexpr int NW = WM * WN;                                                                                   \
    constexpr int RP = NW * 16;                                                                                   \
    constexpr int BM = WM * MF * 16, BN = WN * NF * 16;                                                           \
    constexpr int AP = BM / RP, BP = (BN + RP - 1) / RP, BFULL = BN / RP;                                         \
    constexpr int NST = (NST_);                                                                                   \
    constexpr int STAGE = (BM + BN) * 16;    /* 4-byte words per ring stage: A rows then B rows, 64 bytes each */ \
    constexpr int STAGE_B = STAGE * 4;                                                                            \
    static_assert(NW == 4 || NW == 8, "4 or 8 waves per workgroup");                                              \
    static_assert(BM % RP == 0 && AP <= 2 && BFULL <= 2, "A in 1-2 full passes, B in at most 2 full + 1 partial"); \
    __shared__ __attribute__((aligned(16))) float lds[NST * STAGE];                                               \
    const int tid = threadIdx.x;                                                                                  \
    const int lane = tid & 63;                                                                                    \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                    \
    const int lr = lane & 15, lq = lane >> 4;                                                                     \
    const int wm = wave / WN, wn = wave % WN;                                                                     \
    const int nmt = a.n_mtiles, nnt = a.n_ntiles;                                                                 \
    const int bid = blockIdx.x;                                                                                   \
    const XcdSlot slot = xcd_slot(nmt, nnt, bid);     /* XCD-aware 1-D tile map (conv_index.h) */                 \
    if (xcd_slot_padding(slot)) return;               /* the grid is padded to 8 x max tiles per XCD */           \
    const int mt = xcd_slot_mtile(slot), nt = slot.nt;                                                            \
    const int m0 = mt * BM;                                                                                       \
    const int f0 = nt * (WN * NF);                                                                                \
    const int HoWo = a.Ho * a.Wo;                                                                                 \
    const int srow = tid >> 2;                                                                                    \
    const int sc = (tid & 3) ^ ((4 - ((srow >> 2) & 3)) & 3);                                                     \
    const int n0 = fastdiv(m0, a.howo_magic, a.howo_shift), rem0 = m0 - n0 * HoWo;                                \
    const int oy0 = fastdiv(rem0, a.wo_magic, a.wo_shift), ox0 = rem0 - oy0 * a.Wo;                               \
    const long long lin0 = ((long long)n0 * a.H + oy0 * a.stride) * a.W + ox0 * a.stride;                         \
    const unsigned lds_wave = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)lds + wave * 1024u);            \
    const int ld_off = lr * 16 + ((lq ^ ((4 - ((lr >> 2) & 3)) & 3)) << 2);                                       \
    const float* const a_rd = lds + (wm * MF * 16) * 16 + ld_off;                                                 \
    const float* const b_rd = lds + BM * 16 + (wn * NF * 16) * 16 + ld_off;                                       \
    const bool b_last = BP > BFULL && (BFULL * RP + wave * 16 < BN);                                              \
    const _Float16* const in16 = reinterpret_cast<const _Float16*>(a.in);                                         \
    const _Float16* const w16 = reinterpret_cast<const _Float16*>(a.w);                                           \
    f32x4 acc[MF][NF];                                                                                            \
    _Pragma("unroll") for (int f = 0; f < MF; ++f)                                                                \
        _Pragma("unroll") for (int j = 0; j < NF; ++j) acc[f][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

#define PADEL_T16_WEIGHTS()                                                                                       \
    unsigned voffB[BP];                                                                                           \
    _Pragma("unroll") for (int p = 0; p < BP; ++p) {                                                              \
        const int rr = srow + RP * p;                                                                             \
        const int frag = min(f0 + (rr >> 4), a.n16 - 1);                                                          \
        voffB[p] = (unsigned)((((frag - f0) * 16 + (rr & 15)) * Ktot) * 2 + sc * 16);                             \
    }                                                                                                             \
    const i32x4 rsrcB = make_rsrc(w16 + (long long)f0 * 16 * Ktot);

#define PADEL_T16_FINISH()                                                                                        \
    const bool fast_ = m0 + BM <= a.M && (f0 + WN * NF) * 16 <= a.cout && ((a.out_choff & 3) == 0) &&             \
                       ((a.out_cs & 3) == 0) && (!a.res || (((a.res_choff | a.res_cs) & 3) == 0));                \
    int mpix_[MF];                                                                                                \
    _Pragma("unroll") for (int f = 0; f < MF; ++f) { const int m_ = m0 + wm * MF * 16 + f * 16 + lr; mpix_[f] = m_ < a.M ? m_ : -1; } \
    f16_epilogue<MF, NF>(a, acc, mpix_, f0 + wn * NF, lq, fast_);

// =====================================================================================================  3x3
template <int WM, int WN, int MF, int NF>
__global__ void __launch_bounds__(64 * WM * WN, min_waves16(WM * WN, MF * NF)) conv_tap16_kernel(const ConvArgs a) {
    PADEL_T16_GEOMETRY(3)
    const int nfull = a.cin >> 6;            // 64-channel chunks: 18 k-steps each
    const bool has_tail = (a.cin & 32) != 0; // + 9 k-steps of the last 32 channels
    const int Ktot = (nfull * 18 + (has_tail ? 9 : 0)) * 32;      // halves per weight row

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
        const unsigned off = (unsigned)((lin - lin0) * a.in_cs * 2 + sc * 16);
        bool vy[3], vx[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            vy[d] = rv && (unsigned)(oy * a.stride - 1 + d) < (unsigned)a.H;
            vx[d] = (unsigned)(ox * a.stride - 1 + d) < (unsigned)a.W;
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) voffA[p][t] = (vy[t / 3] && vx[t % 3]) ? off : kOOR;
    }
    const i32x4 rsrcA = make_rsrc(in16 + ((lin0 - (a.W + 1)) * a.in_cs + a.in_choff));
    unsigned tapoff[18];
#pragma unroll
    for (int j = 0; j < 18; ++j) {
        const int t = j >> 1, ky = t / 3, kx = t % 3;
        tapoff[j] = __builtin_amdgcn_readfirstlane((unsigned)((ky * a.W + kx) * a.in_cs * 2 + (j & 1) * 64));
    }
    PADEL_T16_WEIGHTS()

    unsigned s_chunk = 0, s_kb = 0;
    bool nxt_tail = nfull == 0;
    unsigned wrap_off1 = nxt_tail ? tapoff[2] : tapoff[1];
    unsigned wrapv1[AP];
#pragma unroll
    for (int p = 0; p < AP; ++p) wrapv1[p] = nxt_tail ? voffA[p][1] : voffA[p][0];

#define PADEL_T16_STEP(J)                                                                                         \
    do {                                                                                                          \
        wait_vm<AP + BFULL>();                                                                                    \
        __builtin_amdgcn_s_barrier();                                                                             \
        if constexpr ((J) + 2 < 18)                                                                               \
            PADEL_T16_DMA(((J) + 2) % 3, s_chunk + tapoff[((J) + 2) % 18], s_kb + ((J) + 2) * 64u,                \
                          voffA[0][(((J) + 2) % 18) >> 1], voffA[AP - 1][(((J) + 2) % 18) >> 1]);                 \
        else if constexpr ((J) == 16)                                                                             \
            PADEL_T16_DMA(0, s_chunk + 128u + tapoff[0], s_kb + 18 * 64u, voffA[0][0], voffA[AP - 1][0]);         \
        else                                                                                                      \
            PADEL_T16_DMA(1, s_chunk + 128u + wrap_off1, s_kb + 19 * 64u, wrapv1[0], wrapv1[AP - 1]);             \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PADEL_T16_COMPUTE((J) % 3);                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    } while (0)
#define PADEL_T16_TSTEP(J)                                                                                        \
    do {                                                                                                          \
        if constexpr ((J) == 8) wait_vm<0>(); else wait_vm<AP + BFULL>();                                         \
        __builtin_amdgcn_s_barrier();                                                                             \
        if constexpr ((J) + 2 < 9)                                                                                \
            PADEL_T16_DMA(((J) + 2) % 3, s_chunk + tapoff[2 * ((J) + 2 < 9 ? (J) + 2 : 0)], s_kb + ((J) + 2) * 64u, \
                          voffA[0][(J) + 2 < 9 ? (J) + 2 : 0], voffA[AP - 1][(J) + 2 < 9 ? (J) + 2 : 0]);         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PADEL_T16_COMPUTE((J) % 3);                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    } while (0)

    PADEL_T16_DMA(0, tapoff[0], 0u, voffA[0][0], voffA[AP - 1][0]);
    PADEL_T16_DMA(1, wrap_off1, 64u, wrapv1[0], wrapv1[AP - 1]);
    for (int c = 0; c < nfull; ++c) {
        nxt_tail = has_tail && c == nfull - 1;
        wrap_off1 = nxt_tail ? tapoff[2] : tapoff[1];
#pragma unroll
        for (int p = 0; p < AP; ++p) wrapv1[p] = nxt_tail ? voffA[p][1] : voffA[p][0];
        PADEL_T16_STEP(0);  PADEL_T16_STEP(1);  PADEL_T16_STEP(2);  PADEL_T16_STEP(3);  PADEL_T16_STEP(4);  PADEL_T16_STEP(5);
        PADEL_T16_STEP(6);  PADEL_T16_STEP(7);  PADEL_T16_STEP(8);  PADEL_T16_STEP(9);  PADEL_T16_STEP(10); PADEL_T16_STEP(11);
        PADEL_T16_STEP(12); PADEL_T16_STEP(13); PADEL_T16_STEP(14); PADEL_T16_STEP(15); PADEL_T16_STEP(16); PADEL_T16_STEP(17);
        s_chunk += 128u;
        s_kb += 18u * 64u;
    }
    if (has_tail) {
        PADEL_T16_TSTEP(0); PADEL_T16_TSTEP(1); PADEL_T16_TSTEP(2); PADEL_T16_TSTEP(3); PADEL_T16_TSTEP(4);
        PADEL_T16_TSTEP(5); PADEL_T16_TSTEP(6); PADEL_T16_TSTEP(7); PADEL_T16_TSTEP(8);
    } else {
        wait_vm<0>();
    }
    PADEL_T16_FINISH()
#undef PADEL_T16_STEP
#undef PADEL_T16_TSTEP
}

// =====================================================================================================  1x1
constexpr int tap16_1_min_waves(int nw, int frags, int stage_bytes) {
    const int by_lds = (160 * 1024 / (4 * stage_bytes)) * nw / 4;
    const int want = min_waves16(nw, frags);
    return by_lds < want ? (by_lds < 1 ? 1 : by_lds) : want;
}

template <int WM, int WN, int MF, int NF>
__global__ void __launch_bounds__(64 * WM * WN, tap16_1_min_waves(WM * WN, MF * NF, (WM * MF + WN * NF) * 16 * 64)) conv_tap16_1_kernel(const ConvArgs a) {
    PADEL_T16_GEOMETRY(4)
    const int nks = a.cin >> 5;              // 32 channels per k-step
    const int Ktot = nks * 32;

    unsigned voffA[AP];
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
        voffA[p] = rv ? (unsigned)((lin - lin0) * a.in_cs * 2 + sc * 16) : kOOR;
    }
    const i32x4 rsrcA = make_rsrc(in16 + (lin0 * a.in_cs + a.in_choff));
    PADEL_T16_WEIGHTS()

    unsigned s_k = 0;
    constexpr int PD = 3;                     // whole 4-stage ring in flight: the matrix pipe is no cover here
#define PADEL_T16_1STEP(J)                                                                                        \
    if ((J) < nb) {                                                                                               \
        wait_vm<(PD - 1) * (AP + BFULL)>();                                                                       \
        __builtin_amdgcn_s_barrier();                                                                             \
        PADEL_T16_DMA(((J) + PD) % 4, s_k + ((J) + PD) * 64u, s_k + ((J) + PD) * 64u, voffA[0], voffA[AP - 1]);   \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PADEL_T16_COMPUTE((J) % 4);                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    }
    PADEL_T16_DMA(0, 0u, 0u, voffA[0], voffA[AP - 1]);
    PADEL_T16_DMA(1, 64u, 64u, voffA[0], voffA[AP - 1]);
    PADEL_T16_DMA(2, 128u, 128u, voffA[0], voffA[AP - 1]);
    for (int k = 0; k < nks; k += 16) {
        const int nb = min(16, nks - k);
        PADEL_T16_1STEP(0)  PADEL_T16_1STEP(1)  PADEL_T16_1STEP(2)  PADEL_T16_1STEP(3)
        PADEL_T16_1STEP(4)  PADEL_T16_1STEP(5)  PADEL_T16_1STEP(6)  PADEL_T16_1STEP(7)
        PADEL_T16_1STEP(8)  PADEL_T16_1STEP(9)  PADEL_T16_1STEP(10) PADEL_T16_1STEP(11)
        PADEL_T16_1STEP(12) PADEL_T16_1STEP(13) PADEL_T16_1STEP(14) PADEL_T16_1STEP(15)
        s_k += 16u * 64u;
    }
    wait_vm<0>();
    PADEL_T16_FINISH()
#undef PADEL_T16_1STEP
}

// ===================================================================================================== double steps
// The same kernels with 64-channel k-steps: two 64-byte sub-rows per tile row and step (A0 | A1 | B0 | B1), i.e. two
// MFMAs per fragment pair between consecutive barriers.  The fp16 MFMAs are so short (16 cycles) that the fixed cost
// of a k-step — counted wait, barrier, DMA issue — dominates the single-step kernels; doubling the work per step
// amortises it.  No repacking: the two halves of a (chunk, tap) are adjacent 64-byte runs in pixels and weight rows
// alike.  cin % 64 == 32: the 3x3 kernel's tail block pairs taps (A0 = tap 2t, A1 = tap 2t+1 of the last 32
// channels; its weight rows are already tap-major), the 1x1 kernel switches the last step's second sub-row off —
// for A AND for the weights (the bytes behind a weight row are not weights: 0 x NaN-pattern would poison the sum).
#define PADEL_T16D_DMA(SR_, SA0_, SA1_, SB0_, SB1_, VA00_, VA01_, VA10_, VA11_, VBX_)                             \
    do {                                                                                                          \
        const unsigned sa0_ = (SA0_), sa1_ = (SA1_), sb0_ = (SB0_), sb1_ = (SB1_);                                \
        lds_dma<(SR_) * STAGE_B>((VA00_), rsrcA, sa0_, lds_wave);                                                 \
        if constexpr (AP >= 2) lds_dma<(SR_) * STAGE_B + RP * 64>((VA01_), rsrcA, sa0_, lds_wave);                \
        lds_dma<(SR_) * STAGE_B + BM * 64>((VA10_), rsrcA, sa1_, lds_wave);                                       \
        if constexpr (AP >= 2) lds_dma<(SR_) * STAGE_B + BM * 64 + RP * 64>((VA11_), rsrcA, sa1_, lds_wave);      \
        if constexpr (BFULL >= 1) lds_dma<(SR_) * STAGE_B + 2 * BM * 64>(voffB[0], rsrcB, sb0_, lds_wave);        \
        if constexpr (BFULL >= 2) lds_dma<(SR_) * STAGE_B + 2 * BM * 64 + RP * 64>(voffB[1], rsrcB, sb0_, lds_wave); \
        if constexpr (BP > BFULL) { if (b_last) lds_dma<(SR_) * STAGE_B + 2 * BM * 64 + BFULL * RP * 64>(voffB[BP - 1], rsrcB, sb0_, lds_wave); } \
        if constexpr (BFULL >= 1) lds_dma<(SR_) * STAGE_B + (2 * BM + BN) * 64>((VBX_) ? kOOR : voffB[0], rsrcB, sb1_, lds_wave); \
        if constexpr (BFULL >= 2) lds_dma<(SR_) * STAGE_B + (2 * BM + BN) * 64 + RP * 64>((VBX_) ? kOOR : voffB[1], rsrcB, sb1_, lds_wave); \
        if constexpr (BP > BFULL) { if (b_last) lds_dma<(SR_) * STAGE_B + (2 * BM + BN) * 64 + BFULL * RP * 64>((VBX_) ? kOOR : voffB[BP - 1], rsrcB, sb1_, lds_wave); } \
    } while (0)

#define PADEL_T16D_COMPUTE(ST_)                                                                                   \
    do {                                                                                                          \
        __builtin_amdgcn_s_setprio(1);                                                                            \
        _Pragma("unroll") for (int sub = 0; sub < 2; ++sub) {                                                     \
            f32x4 A_[MF], B_[NF];                                                                                 \
            _Pragma("unroll") for (int f = 0; f < MF; ++f) A_[f] = *reinterpret_cast<const f32x4*>(a_rd + (ST_) * STAGE + sub * BM * 16 + f * 256); \
            _Pragma("unroll") for (int j = 0; j < NF; ++j) B_[j] = *reinterpret_cast<const f32x4*>(b_rd + (ST_) * STAGE + sub * BN * 16 + j * 256); \
            _Pragma("unroll") for (int f = 0; f < MF; ++f)                                                        \
                _Pragma("unroll") for (int j = 0; j < NF; ++j)                                                    \
                    acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, B_[j]), __builtin_bit_cast(h16x8, A_[f]), acc[f][j], 0, 0, 0); \
        }                                                                                                         \
        __builtin_amdgcn_s_setprio(0);                                                                            \
    } while (0)

#define PADEL_T16D_GEOMETRY()                                                                                     \
    constexpr int NW = WM * WN;                                                                                   \
    constexpr int RP = NW * 16;                                                                                   \
    constexpr int BM = WM * MF * 16, BN = WN * NF * 16;                                                           \
    constexpr int AP = BM / RP, BP = (BN + RP - 1) / RP, BFULL = BN / RP;                                         \
    constexpr int STAGE = 2 * (BM + BN) * 16;      /* 4-byte words per ring stage: A0 | A1 | B0 | B1 */           \
    constexpr int STAGE_B = STAGE * 4;                                                                            \
    constexpr int NREQ = 2 * AP + 2 * BFULL;                                                                      \
    static_assert(NW == 4 || NW == 8, "4 or 8 waves per workgroup");                                              \
    static_assert(BM % RP == 0 && AP <= 2 && BFULL <= 2, "A in 1-2 full passes, B in at most 2 full + 1 partial"); \
    static_assert(3 * STAGE_B <= 160 * 1024, "ring must fit the LDS");                                            \
    __shared__ __attribute__((aligned(16))) float lds[3 * STAGE];                                                 \
    const int tid = threadIdx.x;                                                                                  \
    const int lane = tid & 63;                                                                                    \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                    \
    const int lr = lane & 15, lq = lane >> 4;                                                                     \
    const int wm = wave / WN, wn = wave % WN;                                                                     \
    const int nmt = a.n_mtiles, nnt = a.n_ntiles;                                                                 \
    const int bid = blockIdx.x;                                                                                   \
    const XcdSlot slot = xcd_slot(nmt, nnt, bid);     /* XCD-aware 1-D tile map (conv_index.h) */                 \
    if (xcd_slot_padding(slot)) return;               /* the grid is padded to 8 x max tiles per XCD */           \
    const int mt = xcd_slot_mtile(slot), nt = slot.nt;                                                            \
    const int m0 = mt * BM;                                                                                       \
    const int f0 = nt * (WN * NF);                                                                                \
    const int HoWo = a.Ho * a.Wo;                                                                                 \
    const int srow = tid >> 2;                                                                                    \
    const int sc = (tid & 3) ^ ((4 - ((srow >> 2) & 3)) & 3);                                                     \
    const int n0 = fastdiv(m0, a.howo_magic, a.howo_shift), rem0 = m0 - n0 * HoWo;                                \
    const int oy0 = fastdiv(rem0, a.wo_magic, a.wo_shift), ox0 = rem0 - oy0 * a.Wo;                               \
    const long long lin0 = ((long long)n0 * a.H + oy0 * a.stride) * a.W + ox0 * a.stride;                         \
    const unsigned lds_wave = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)lds + wave * 1024u);            \
    const int ld_off = lr * 16 + ((lq ^ ((4 - ((lr >> 2) & 3)) & 3)) << 2);                                       \
    const float* const a_rd = lds + (wm * MF * 16) * 16 + ld_off;                                                 \
    const float* const b_rd = lds + 2 * BM * 16 + (wn * NF * 16) * 16 + ld_off;                                   \
    const bool b_last = BP > BFULL && (BFULL * RP + wave * 16 < BN);                                              \
    const _Float16* const in16 = reinterpret_cast<const _Float16*>(a.in);                                         \
    const _Float16* const w16 = reinterpret_cast<const _Float16*>(a.w);                                           \
    f32x4 acc[MF][NF];                                                                                            \
    _Pragma("unroll") for (int f = 0; f < MF; ++f)                                                                \
        _Pragma("unroll") for (int j = 0; j < NF; ++j) acc[f][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

constexpr int min_waves16d(int nw, int frags) { return nw == 4 ? (frags <= 6 ? 3 : 2) : 2; }

template <int WM, int WN, int MF, int NF>
__global__ void __launch_bounds__(64 * WM * WN, min_waves16d(WM * WN, MF * NF)) conv_tap16d_kernel(const ConvArgs a) {
    PADEL_T16D_GEOMETRY()
    const int nfull = a.cin >> 6;
    const bool has_tail = (a.cin & 32) != 0;
    const int Ktot = (nfull * 18 + (has_tail ? 9 : 0)) * 32;      // halves per weight row (same packing as the single-step kernel)

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
        const unsigned off = (unsigned)((lin - lin0) * a.in_cs * 2 + sc * 16);
        bool vy[3], vx[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            vy[d] = rv && (unsigned)(oy * a.stride - 1 + d) < (unsigned)a.H;
            vx[d] = (unsigned)(ox * a.stride - 1 + d) < (unsigned)a.W;
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) voffA[p][t] = (vy[t / 3] && vx[t % 3]) ? off : kOOR;
    }
    const i32x4 rsrcA = make_rsrc(in16 + ((lin0 - (a.W + 1)) * a.in_cs + a.in_choff));
    unsigned tapoff[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) tapoff[t] = __builtin_amdgcn_readfirstlane((unsigned)(((t / 3) * a.W + (t % 3)) * a.in_cs * 2));
    PADEL_T16_WEIGHTS()

    unsigned s_chunk = 0, s_kb = 0;
#define PADEL_T16D_REQ_FULL(SR_, CH_, KB_, T_)                                                                    \
    PADEL_T16D_DMA(SR_, (CH_) + tapoff[T_], (CH_) + tapoff[T_] + 64u, KB_, (KB_) + 64u,                           \
                   voffA[0][T_], voffA[AP - 1][T_], voffA[0][T_], voffA[AP - 1][T_], false)
#define PADEL_T16D_REQ_TAIL(SR_, CH_, KB_, JT_)                                                                   \
    PADEL_T16D_DMA(SR_, (CH_) + tapoff[2 * (JT_)], (CH_) + tapoff[2 * (JT_) + 1 < 9 ? 2 * (JT_) + 1 : 8], KB_, (KB_) + 64u, \
                   voffA[0][2 * (JT_)], voffA[AP - 1][2 * (JT_)],                                                 \
                   2 * (JT_) + 1 < 9 ? voffA[0][2 * (JT_) + 1 < 9 ? 2 * (JT_) + 1 : 8] : kOOR,                    \
                   2 * (JT_) + 1 < 9 ? voffA[AP - 1][2 * (JT_) + 1 < 9 ? 2 * (JT_) + 1 : 8] : kOOR,               \
                   2 * (JT_) + 1 >= 9)
    bool nxt_tail = false;
#define PADEL_T16D_STEP(J)                                                                                        \
    do {                                                                                                          \
        wait_vm<NREQ>();                                                                                          \
        __builtin_amdgcn_s_barrier();                                                                             \
        if constexpr ((J) + 2 < 9) {                                                                              \
            PADEL_T16D_REQ_FULL(((J) + 2) % 3, s_chunk, s_kb + ((J) + 2) * 128u, (J) + 2 < 9 ? (J) + 2 : 0);      \
        } else {                                                                                                  \
            if (nxt_tail) { PADEL_T16D_REQ_TAIL(((J) + 2) % 3, s_chunk + 128u, s_kb + ((J) + 2) * 128u, ((J) + 2) % 9); } \
            else { PADEL_T16D_REQ_FULL(((J) + 2) % 3, s_chunk + 128u, s_kb + ((J) + 2) * 128u, ((J) + 2) % 9); }  \
        }                                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PADEL_T16D_COMPUTE((J) % 3);                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    } while (0)
#define PADEL_T16D_TSTEP(JT)                                                                                      \
    do {                                                                                                          \
        if constexpr ((JT) == 4) wait_vm<0>(); else wait_vm<NREQ>();                                              \
        __builtin_amdgcn_s_barrier();                                                                             \
        if constexpr ((JT) + 2 < 5) { PADEL_T16D_REQ_TAIL(((JT) + 2) % 3, s_chunk, s_kb + ((JT) + 2) * 128u, (JT) + 2 < 5 ? (JT) + 2 : 0); } \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PADEL_T16D_COMPUTE((JT) % 3);                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    } while (0)

    if (nfull > 0) {
        PADEL_T16D_REQ_FULL(0, 0u, 0u, 0);
        PADEL_T16D_REQ_FULL(1, 0u, 128u, 1);
    } else {
        PADEL_T16D_REQ_TAIL(0, 0u, 0u, 0);
        PADEL_T16D_REQ_TAIL(1, 0u, 128u, 1);
    }
    for (int c = 0; c < nfull; ++c) {
        nxt_tail = has_tail && c == nfull - 1;
        PADEL_T16D_STEP(0); PADEL_T16D_STEP(1); PADEL_T16D_STEP(2); PADEL_T16D_STEP(3); PADEL_T16D_STEP(4);
        PADEL_T16D_STEP(5); PADEL_T16D_STEP(6); PADEL_T16D_STEP(7); PADEL_T16D_STEP(8);
        s_chunk += 128u;
        s_kb += 9u * 128u;
    }
    if (has_tail) {
        PADEL_T16D_TSTEP(0); PADEL_T16D_TSTEP(1); PADEL_T16D_TSTEP(2); PADEL_T16D_TSTEP(3); PADEL_T16D_TSTEP(4);
    } else {
        wait_vm<0>();
    }
    PADEL_T16_FINISH()
#undef PADEL_T16D_STEP
#undef PADEL_T16D_TSTEP
#undef PADEL_T16D_REQ_FULL
#undef PADEL_T16D_REQ_TAIL
}

template <int WM, int WN, int MF, int NF>
__global__ void __launch_bounds__(64 * WM * WN, min_waves16d(WM * WN, MF * NF)) conv_tap16d_1_kernel(const ConvArgs a) {
    PADEL_T16D_GEOMETRY()
    const int nks = (a.cin + 63) >> 6;            // 64 channels per k-step; the last one half empty if cin & 32
    const bool half_tail = (a.cin & 32) != 0;
    const int Ktot = (a.cin >> 5) * 32;

    unsigned voffA[AP];
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
        voffA[p] = rv ? (unsigned)((lin - lin0) * a.in_cs * 2 + sc * 16) : kOOR;
    }
    const i32x4 rsrcA = make_rsrc(in16 + (lin0 * a.in_cs + a.in_choff));
    PADEL_T16_WEIGHTS()

    unsigned s_k = 0;
#define PADEL_T16D_OFF1(K_) (half_tail && (int)(K_) >= nks - 1)
#define PADEL_T16D_REQ1(SR_, K_)                                                                                  \
    PADEL_T16D_DMA(SR_, (K_) * 128u, (K_) * 128u + 64u, (K_) * 128u, (K_) * 128u + 64u, voffA[0], voffA[AP - 1],  \
                   PADEL_T16D_OFF1(K_) ? kOOR : voffA[0], PADEL_T16D_OFF1(K_) ? kOOR : voffA[AP - 1], PADEL_T16D_OFF1(K_))
#define PADEL_T16D_1STEP(J)                                                                                       \
    if ((J) < nb) {                                                                                               \
        wait_vm<NREQ>();                                                                                          \
        __builtin_amdgcn_s_barrier();                                                                             \
        PADEL_T16D_REQ1(((J) + 2) % 3, s_k + (J) + 2);                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PADEL_T16D_COMPUTE((J) % 3);                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    }
    PADEL_T16D_REQ1(0, 0u);
    PADEL_T16D_REQ1(1, 1u);
    for (int k = 0; k < nks; k += 9) {
        const int nb = min(9, nks - k);
        PADEL_T16D_1STEP(0) PADEL_T16D_1STEP(1) PADEL_T16D_1STEP(2) PADEL_T16D_1STEP(3) PADEL_T16D_1STEP(4)
        PADEL_T16D_1STEP(5) PADEL_T16D_1STEP(6) PADEL_T16D_1STEP(7) PADEL_T16D_1STEP(8)
        s_k += 9u;
    }
    wait_vm<0>();
    PADEL_T16_FINISH()
#undef PADEL_T16D_1STEP
#undef PADEL_T16D_REQ1
#undef PADEL_T16D_OFF1
}

template <int WM, int WN, int MF, int NF>
static hipError_t launch_t16d(const ConvArgs& a_in, hipStream_t s) {
    ConvArgs a = a_in;
    constexpr int BM = WM * MF * 16;
    a.n_mtiles = (a.M + BM - 1) / BM;
    a.n_ntiles = (a.n16 + WN * NF - 1) / (WN * NF);
    dim3 grid(8u * (unsigned)((a.n_mtiles + 7) / 8) * (unsigned)a.n_ntiles, 1, 1);
    if (a.ksize == 3) hipLaunchKernelGGL((conv_tap16d_kernel<WM, WN, MF, NF>), grid, dim3(64 * WM * WN), 0, s, a);
    else hipLaunchKernelGGL((conv_tap16d_1_kernel<WM, WN, MF, NF>), grid, dim3(64 * WM * WN), 0, s, a);
    return hipGetLastError();
}

template <int WM, int WN, int MF, int NF>
static hipError_t launch_t16(const ConvArgs& a_in, hipStream_t s) {
    ConvArgs a = a_in;
    constexpr int BM = WM * MF * 16;
    a.n_mtiles = (a.M + BM - 1) / BM;
    a.n_ntiles = (a.n16 + WN * NF - 1) / (WN * NF);
    dim3 grid(8u * (unsigned)((a.n_mtiles + 7) / 8) * (unsigned)a.n_ntiles, 1, 1);
    if (a.ksize == 3) hipLaunchKernelGGL((conv_tap16_kernel<WM, WN, MF, NF>), grid, dim3(64 * WM * WN), 0, s, a);
    else hipLaunchKernelGGL((conv_tap16_1_kernel<WM, WN, MF, NF>), grid, dim3(64 * WM * WN), 0, s, a);
    return hipGetLastError();
}

// tile ids: the fp32 id space + 30.. for the larger per-wave tiles only the fp16 path has
hipError_t launch_conv_t16(const ConvArgs& a, int tile, hipStream_t s) {
    switch (tile) {
        case 6: return launch_t16<2, 2, 2, 4>(a, s);    //  64 x 128
        case 7: return launch_t16<2, 2, 2, 3>(a, s);    //  64 x  96
        case 9: return launch_t16<4, 1, 2, 4>(a, s);    // 128 x  64
        case 11: return launch_t16<4, 1, 2, 2>(a, s);   // 128 x  32
        case 12: return launch_t16<4, 1, 2, 1>(a, s);   // 128 x  16
        case 20: return launch_t16<4, 1, 2, 3>(a, s);   // 128 x  48
        case 30: return launch_t16<2, 2, 4, 4>(a, s);   // 128 x 128, 4 waves of 64 x 64
        case 31: return launch_t16<2, 2, 4, 3>(a, s);   // 128 x  96
        case 32: return launch_t16<2, 2, 4, 2>(a, s);   // 128 x  64
        // + 40: the same tile with 64-channel (double) k-steps
        case 46: return launch_t16d<2, 2, 2, 4>(a, s);  //  64 x 128
        case 47: return launch_t16d<2, 2, 2, 3>(a, s);  //  64 x  96
        case 49: return launch_t16d<4, 1, 2, 4>(a, s);  // 128 x  64
        case 51: return launch_t16d<4, 1, 2, 2>(a, s);  // 128 x  32
        case 60: return launch_t16d<4, 1, 2, 3>(a, s);  // 128 x  48
        case 70: return launch_t16d<2, 2, 4, 4>(a, s);  // 128 x 128
        case 71: return launch_t16d<2, 2, 4, 3>(a, s);  // 128 x  96
        case 72: return launch_t16d<2, 2, 4, 2>(a, s);  // 128 x  64
    }
    return hipErrorNotSupported;
}

}  // namespace padel
