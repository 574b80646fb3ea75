// pa_jpeg_decode on the device (include/padel_hip.h has the specification, mjpeg.decode_host is the numpy twin): three passes.
//   (a) jpeg_entropy_kernel   one wave per restart interval: lane 0 runs the shared decoder (jpeg_entropy.h) block by block into 64
//                             coefficients in LDS, the 64 lanes store the block — int16, zig-zag order, one coalesced 128-byte row.
//                             (Decoding 24 blocks per barrier instead of one was tried and measured the same: the pass is bound by
//                             lane 0's serial work, about 0.5 us per symbol, not by the barriers or the stores.)
//                             Within such an interval the bit stream is serial; intervals are what is parallel.
//       jpeg_entropy_split_kernel   one workgroup per LONG interval (a frame without restart markers is one): its bytes cut into
//                             subsequences, one lane each, a fixed point over their exit states, a write pass, DC scans
//                             (jpeg_entropy_split.h has the algorithm; the same coefficients and status word).  Measured
//                             (profiles/mjpeg_split_bench.txt): 3.1 ms for a 120 KB frame against 73 on one wave; a lane whose
//                             whole wave decodes needs at most 1.6 us per symbol.  The interval's bytes are read from global
//                             memory; staging them through LDS was not tried.
//   (b) jpeg_idct_kernel      one thread per block, as the encoder's DCT: dequantise, inverse DCT, 8 rows of 8 samples into the
//                             padded planes (Y: MCUs x 16, Cb / Cr: MCUs x 8 a side).
//   (c) jpeg_colour_kernel    one thread per 16 pixels of an output row: fancy chroma upsampling (rows r - 1 .. r + 1 of the chroma
//                             planes, which is why this is its own pass), YCbCr -> BGR, three 16-byte stores where width and
//                             destination allow, byte stores otherwise.
#include "jpeg_decode.h"
#include "jpeg_idct.h"

namespace padel {

using namespace jpeg;

static_assert(sizeof(HuffDec) == 896 && offsetof(JpegDecFrame, quant) == 4 * sizeof(HuffDec), "table layout");
static_assert(sizeof(JpegDecFrame) % 16 == 0 && offsetof(JpegDecFrame, quant) % 16 == 0, "quantisers are read 16 bytes at a time");

__global__ void __launch_bounds__(64) jpeg_entropy_kernel(const JpegDecArgs a) {
    __shared__ HuffDec tab[4];               // dc[0], dc[1], ac[0], ac[1] of the interval's frame
    __shared__ int16_t blk[64];
    __shared__ int s_status;
    const int lane = threadIdx.x;
    const int index = a.order[blockIdx.x];
    const JpegDecInterval iv = a.ivls[index];
    const JpegDecFrame* fr = a.frames + iv.frame;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(fr);
        uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
        for (int i = lane; i < (int)(4 * sizeof(HuffDec) / 4); i += 64) dst[i] = src[i];
    }
    if (lane == 0) s_status = 0;
    const HuffDec* dc[3] = {&tab[fr->comp_dc[0] & 1], &tab[fr->comp_dc[1] & 1], &tab[fr->comp_dc[2] & 1]};
    const HuffDec* ac[3] = {&tab[2 + (fr->comp_ac[0] & 1)], &tab[2 + (fr->comp_ac[1] & 1)], &tab[2 + (fr->comp_ac[2] & 1)]};
    BitReader r;
    br_init(&r, a.data, iv.begin, iv.end);
    int pred0 = 0, pred1 = 0, pred2 = 0;
    int16_t* out = a.coef + ((size_t)iv.frame * (size_t)(a.mcus_x * a.mcus_y) + (size_t)iv.first_mcu) * (kBlocksPerMcu * 64);
    const int blocks = iv.mcus * kBlocksPerMcu;
    for (int b = 0, j = 0; b < blocks; ++b, j = j == 5 ? 0 : j + 1) {
        blk[lane] = 0;
        __syncthreads();
        if (lane == 0 && s_status == 0) {
            int st;
            if (j < 4) st = decode_block(&r, dc[0], ac[0], &pred0, blk);
            else if (j == 4) st = decode_block(&r, dc[1], ac[1], &pred1, blk);
            else st = decode_block(&r, dc[2], ac[2], &pred2, blk);
            s_status = st;
        }
        __syncthreads();
        out[(size_t)b * 64 + lane] = s_status ? (int16_t)0 : blk[lane];      // a block that could not be decoded, and all behind it: zeros
    }
    __syncthreads();
    if (lane == 0) a.ivl_status[index] = s_status;
}

// v[0 .. n) in LDS -> v[i] = min(v[0] + .. + v[i - 1], cap), by all threads of the block: every thread sums a run of consecutive
// entries, thread 0 scans the runs' sums in part[0 .. blockDim.x), every thread rewrites its run.  Ends with a barrier.
static __device__ void block_exclusive_scan(uint32_t* v, int n, uint32_t cap, uint32_t* part) {
    const int nt = blockDim.x, tid = threadIdx.x;
    const int run = (n + nt - 1) / nt;
    const int lo = min(tid * run, n), hi = min(lo + run, n);
    uint32_t sum = 0;
    for (int i = lo; i < hi; ++i) sum = min(sum + v[i], cap);
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t before = 0;
        for (int i = 0; i < nt && i * run < n; ++i) {
            const uint32_t s = part[i];
            part[i] = before;
            before = min(before + s, cap);
        }
    }
    __syncthreads();
    sum = part[tid];
    for (int i = lo; i < hi; ++i) {
        const uint32_t s = v[i];
        v[i] = sum;
        sum = min(sum + s, cap);
    }
    __syncthreads();
}

// One workgroup per interval; lanes take the subsequences t, t + blockDim.x, ...  (at most 64 each: blockDim.x >= 64 and at most
// kSplitMaxSub subsequences).  The phases: (1) stuffed bytes per subsequence and the first terminating FF, a scan and a
// min-reduction, which give every subsequence its first bit; (2) the fixed point, one barrier pair per round; (3) first blocks by a
// scan of the finished-block counts; (4) the interval's coefficients zeroed, 16 bytes a store; (5) the write pass; (6) the block that
// could not be decoded zeroed, the DC differences summed per component; (7) status word and rounds.
__global__ void __launch_bounds__(kSplitMaxThreads) jpeg_entropy_split_kernel(const JpegDecArgs a) {
    __shared__ HuffDec tab[6];                           // per component: DC, then AC
    __shared__ uint32_t s_u[kSplitMaxSub + 1];           // stuffed bytes per subsequence -> before it -> its first bit
    __shared__ uint32_t s_first[kSplitMaxSub];           // blocks finished in it -> its first block
    __shared__ SplitState s_exit[kSplitMaxSub], s_ent[kSplitMaxSub];
    __shared__ uint32_t s_part[3 * kSplitMaxThreads];
    __shared__ uint32_t s_term, s_total, s_last, s_bad;
    __shared__ int s_status, s_changed[2];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int index = a.order[a.n_serial + blockIdx.x];
    const JpegDecInterval iv = a.ivls[index];
    const JpegDecFrame* fr = a.frames + iv.frame;
    PA_JUNROLL
    for (int k = 0; k < 3; ++k) {
        constexpr int words = (int)(sizeof(HuffDec) / 4);
        const uint32_t* dc = reinterpret_cast<const uint32_t*>(&fr->dc[fr->comp_dc[k] & 1]);
        const uint32_t* ac = reinterpret_cast<const uint32_t*>(&fr->ac[fr->comp_ac[k] & 1]);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&tab[k]);
        for (int i = tid; i < words; i += nt) {
            dst[i] = dc[i];
            dst[3 * words + i] = ac[i];
        }
    }
    SplitCtx c;
    c.p = a.data + iv.begin;
    c.len = split_len(iv.begin, iv.end);
    c.sub_bytes = split_sub_bytes(c.len, a.sub_bytes);
    c.nsub = split_count(c.len, c.sub_bytes);
    c.blocks = iv.mcus > 0 ? iv.mcus * kBlocksPerMcu : 0;
    c.tab = tab;
    const int T = c.nsub;
    int16_t* out = a.coef + ((size_t)iv.frame * (size_t)(a.mcus_x * a.mcus_y) + (size_t)iv.first_mcu) * (kBlocksPerMcu * 64);
    const SplitState dead = {kSplitDead, 0}, never = {kSplitDead, 1};
    if (tid == 0) {
        s_term = c.len;
        s_last = (uint32_t)(T - 1);
        s_bad = (uint32_t)c.blocks;
        s_status = 0;
        s_changed[0] = s_changed[1] = 0;
        s_u[T] = 0;
    }
    __syncthreads();
    // (1)
    for (int t = tid; t < T; t += nt) {
        uint32_t n, term;
        split_scan_bytes(c.p, c.len, (uint32_t)t * c.sub_bytes, (uint32_t)(t + 1) * c.sub_bytes, &n, &term);
        s_u[t] = n;
        if (term < c.len) atomicMin(&s_term, term);
        s_exit[t] = dead;
        s_ent[t] = never;
        s_first[t] = 0;
    }
    __syncthreads();
    block_exclusive_scan(s_u, T + 1, 0xffffffffu, s_part);
    c.data_end = s_term;
    if (tid == 0) {
        const int td = min((int)(c.data_end / (uint32_t)c.sub_bytes), T);
        uint32_t n = 0, term;
        if (td < T) split_scan_bytes(c.p, c.len, (uint32_t)td * c.sub_bytes, c.data_end, &n, &term);
        s_total = 8u * (c.data_end - s_u[td] - n);
    }
    __syncthreads();
    c.total_bits = s_total;
    for (int t = tid; t <= T; t += nt) s_u[t] = split_first_bit(&c, t, s_u[t]);
    __syncthreads();
    // (2)
    int rounds = 0;
    if (c.blocks)
        for (;;) {
            unsigned long long need = 0;
            for (int t = tid, i = 0; t < T; t += nt, ++i) {
                const SplitState e = split_entry(t, t ? s_exit[t - 1] : dead, s_u[t]);
                if (!split_same(e, s_ent[t])) {
                    s_ent[t] = e;
                    need |= 1ull << i;
                }
            }
            __syncthreads();
            if (tid == 0) s_changed[(rounds + 1) & 1] = 0;
            for (int t = tid, i = 0; t < T; t += nt, ++i) {
                if (!(need >> i & 1)) continue;
                int fin, st, sym = 0;
                const SplitState e = split_run(&c, t, s_ent[t], s_u[t], s_u[t + 1], 0, nullptr, &fin, &st, &sym);
                if (!split_same(e, s_exit[t])) s_changed[rounds & 1] = 1;
                s_exit[t] = e;
                s_first[t] = (uint32_t)fin;
            }
            __syncthreads();
            ++rounds;
            if (!s_changed[(rounds - 1) & 1] || rounds > T) break;      // (round T + 1 can only confirm)
        }
    // (3)
    for (int t = tid; t < T; t += nt)
        if (s_exit[t].pos == kSplitDead) atomicMin(&s_last, (uint32_t)t);
    __syncthreads();
    block_exclusive_scan(s_first, T, (uint32_t)c.blocks, s_part);
    // (4)
    {
        uint4* z = reinterpret_cast<uint4*>(out);
        const size_t n16 = (size_t)c.blocks * 8;
        for (size_t i = tid; i < n16; i += nt) z[i] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    // (5)
    const int last = (int)s_last;
    for (int t = tid; t <= last && c.blocks; t += nt) {
        int fin, st, sym = 0;
        const SplitState e = split_entry(t, t ? s_exit[t - 1] : dead, s_u[t]);
        const int first = (int)s_first[t];
        split_run(&c, t, e, s_u[t], t == T - 1 ? kSplitDead : s_u[t + 1], first, out, &fin, &st, &sym);
        if (st) {
            s_status = st;
            s_bad = (uint32_t)(first + fin);
        }
    }
    __syncthreads();
    // (6)
    const int bad = (int)s_bad;
    if (bad < c.blocks && tid < 64) out[(size_t)bad * 64 + tid] = 0;
    {
        const int mcus = (bad + kBlocksPerMcu - 1) / kBlocksPerMcu;
        const int run = (mcus + nt - 1) / nt;
        const int lo = min(tid * run, mcus), hi = min(lo + run, mcus);
        int32_t sum[3] = {0, 0, 0};
        for (int m = lo; m < hi; ++m) {
            PA_JUNROLL
            for (int j = 0; j < kBlocksPerMcu; ++j) {
                const int b = m * kBlocksPerMcu + j;
                if (b < bad) sum[j < 4 ? 0 : j - 3] += out[(size_t)b * 64];
            }
        }
        PA_JUNROLL
        for (int k = 0; k < 3; ++k) s_part[k * nt + tid] = (uint32_t)sum[k];
        __syncthreads();
        if (tid < 3) {
            uint32_t before = 0;
            for (int i = 0; i < nt && i * run < mcus; ++i) {
                const uint32_t s = s_part[tid * nt + i];
                s_part[tid * nt + i] = before;
                before += s;
            }
        }
        __syncthreads();
        PA_JUNROLL
        for (int k = 0; k < 3; ++k) sum[k] = (int32_t)s_part[k * nt + tid];
        for (int m = lo; m < hi; ++m) {
            PA_JUNROLL
            for (int j = 0; j < kBlocksPerMcu; ++j) {
                const int b = m * kBlocksPerMcu + j;
                if (b < bad) {
                    int32_t& pred = sum[j < 4 ? 0 : j - 3];
                    pred += out[(size_t)b * 64];
                    out[(size_t)b * 64] = (int16_t)pred;
                }
            }
        }
    }
    // (7)
    if (tid == 0) {
        a.ivl_status[index] = s_status;
        a.ivl_status[a.n_ivls + index] = rounds;
    }
}

__global__ void __launch_bounds__(256) jpeg_idct_kernel(const JpegDecArgs a) {
    const size_t per_frame = (size_t)a.mcus_x * a.mcus_y * kBlocksPerMcu;
    const size_t B = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (B >= per_frame * (size_t)a.n) return;
    const int f = (int)(B / per_frame);
    const int rem = (int)(B % per_frame);
    const int mcu = rem / kBlocksPerMcu, k = rem % kBlocksPerMcu;
    const int my = mcu / a.mcus_x, mx = mcu % a.mcus_x;
    const int comp = k < 4 ? 0 : k - 3;
    const uint4* cs = reinterpret_cast<const uint4*>(a.coef + B * 64);
    const uint4* qs = reinterpret_cast<const uint4*>(a.frames[f].quant[comp]);
    int32_t b[64];
    PA_JUNROLL
    for (int i = 0; i < 8; ++i) {
        const uint4 c = cs[i], q = qs[i];
        const uint32_t cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
        PA_JUNROLL
        for (int j = 0; j < 4; ++j) {
            b[kZigzag[8 * i + 2 * j]] = (int32_t)(int16_t)(cw[j] & 0xffffu) * (int32_t)(qw[j] & 0xffffu);
            b[kZigzag[8 * i + 2 * j + 1]] = (int32_t)(int16_t)(cw[j] >> 16) * (int32_t)(qw[j] >> 16);
        }
    }
    idct_block(b);
    const size_t PW = (size_t)a.mcus_x * 16, PH = (size_t)a.mcus_y * 16;
    uint8_t* frame = a.planes + (size_t)f * (PW * PH * 3 / 2);
    uint8_t* p;
    size_t pitch;
    if (k < 4) {
        pitch = PW;
        p = frame + ((size_t)my * 16 + (k >> 1) * 8) * PW + (size_t)mx * 16 + (k & 1) * 8;
    } else {
        pitch = PW / 2;
        p = frame + PW * PH + (k == 5 ? PW * PH / 4 : 0) + (size_t)my * 8 * pitch + (size_t)mx * 8;
    }
    PA_JUNROLL
    for (int r = 0; r < 8; ++r) {
        uint2 v;
        v.x = (uint32_t)sample(b[8 * r]) | (uint32_t)sample(b[8 * r + 1]) << 8 | (uint32_t)sample(b[8 * r + 2]) << 16 | (uint32_t)sample(b[8 * r + 3]) << 24;
        v.y = (uint32_t)sample(b[8 * r + 4]) | (uint32_t)sample(b[8 * r + 5]) << 8 | (uint32_t)sample(b[8 * r + 6]) << 16 | (uint32_t)sample(b[8 * r + 7]) << 24;
        *reinterpret_cast<uint2*>(p + (size_t)r * pitch) = v;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) jpeg_colour_kernel(const JpegDecArgs a) {
    const int groups = (a.w + 15) / 16;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (size_t)groups * a.h * a.n) return;
    const int g = (int)(gid % groups);
    const int y = (int)((gid / groups) % a.h);
    const int f = (int)(gid / ((size_t)groups * a.h));
    const size_t PW = (size_t)a.mcus_x * 16, PH = (size_t)a.mcus_y * 16;
    const uint8_t* Yp = a.planes + (size_t)f * (PW * PH * 3 / 2);
    const uint8_t* Cb = Yp + PW * PH;
    const uint8_t* Cr = Cb + PW * PH / 4;
    const int ch = (a.h + 1) / 2, cw = (a.w + 1) / 2;
    const int r = y >> 1;
    const int rr = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
    const int c0 = g * 8;
    int sb[10], sr[10];
    PA_JUNROLL
    for (int i = 0; i < 10; ++i) {
        const int c = min(max(c0 - 1 + i, 0), cw - 1);
        sb[i] = 3 * Cb[(size_t)r * (PW / 2) + c] + Cb[(size_t)rr * (PW / 2) + c];
        sr[i] = 3 * Cr[(size_t)r * (PW / 2) + c] + Cr[(size_t)rr * (PW / 2) + c];
    }
    const uint4 yv = *reinterpret_cast<const uint4*>(Yp + (size_t)y * PW + (size_t)g * 16);
    const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
    uint8_t px[48];
    PA_JUNROLL
    for (int i = 0; i < 8; ++i) {
        const int y0 = (yw[i >> 1] >> (16 * (i & 1))) & 255, y1 = (yw[i >> 1] >> (16 * (i & 1) + 8)) & 255;
        ycc_to_bgr(y0, chroma_even(sb[i], sb[i + 1]), chroma_even(sr[i], sr[i + 1]), px + 6 * i);
        ycc_to_bgr(y1, chroma_odd(sb[i + 1], sb[i + 2]), chroma_odd(sr[i + 1], sr[i + 2]), px + 6 * i + 3);
    }
    uint8_t* d = a.dst + (((size_t)f * a.h + y) * a.w + (size_t)g * 16) * 3;
    if (VEC) {
        PA_JUNROLL
        for (int j = 0; j < 3; ++j) {
            uint32_t wds[4];
            PA_JUNROLL
            for (int k = 0; k < 4; ++k)
                wds[k] = (uint32_t)px[16 * j + 4 * k] | (uint32_t)px[16 * j + 4 * k + 1] << 8 | (uint32_t)px[16 * j + 4 * k + 2] << 16 |
                         (uint32_t)px[16 * j + 4 * k + 3] << 24;
            reinterpret_cast<uint4*>(d)[j] = make_uint4(wds[0], wds[1], wds[2], wds[3]);
        }
    } else {
        PA_JUNROLL
        for (int i = 0; i < 16; ++i)
            if (g * 16 + i < a.w) {
                d[3 * i] = px[3 * i];
                d[3 * i + 1] = px[3 * i + 1];
                d[3 * i + 2] = px[3 * i + 2];
            }
    }
}

hipError_t launch_jpeg_decode(const JpegDecArgs& a, int* path, hipStream_t s, hipEvent_t* ev) {
    if (ev) hipEventRecord(ev[0], s);
    if (a.n_serial < 0 || a.n_split < 0 || a.n_serial + a.n_split != a.n_ivls) return hipErrorInvalidValue;
    if (a.n_split && (a.split_threads < 64 || a.split_threads > kSplitMaxThreads || a.split_threads % 64)) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (a.n_serial) {
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)a.n_serial), dim3(64), 0, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.n_split) {
        hipLaunchKernelGGL(jpeg_entropy_split_kernel, dim3((unsigned)a.n_split), dim3((unsigned)a.split_threads), 0, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (ev) hipEventRecord(ev[1], s);
    const size_t blocks = (size_t)a.n * a.mcus_x * a.mcus_y * kBlocksPerMcu;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (ev) hipEventRecord(ev[2], s);
    const size_t items = (size_t)a.n * a.h * ((a.w + 15) / 16);
    const bool vec = a.w % 16 == 0 && reinterpret_cast<uintptr_t>(a.dst) % 16 == 0;
    if (vec) hipLaunchKernelGGL(jpeg_colour_kernel<true>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(jpeg_colour_kernel<false>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
    *path = vec ? 1 : 2;
    e = hipGetLastError();
    if (ev && e == hipSuccess) hipEventRecord(ev[3], s);
    return e;
}

}  // namespace padel
