// The second entropy path of the Motion-JPEG reader (include/padel_hip.h, pa_jpeg_decode): one long restart interval — a whole frame
// where the stream has no restart markers — decoded by many lanes at once.  The interval's bytes are cut into subsequences of S raw
// bytes; every lane decodes one from a guessed state, and a fixed point over the subsequences' exit states replaces the guesses by the
// truth ("speculative synchronisation": a Huffman decoder started at a wrong bit falls into step with the right one after some
// symbols).  One definition for host and device, like jpeg_entropy.h, whose reader, tables and status bits it uses: the kernel in
// jpeg_decode.hip runs these functions with lanes over the subsequences, decode_interval_split_host with a loop, and
// tests/jpeg_split_main.cpp compiles the latter with g++ and compares it with decode_interval_host, under the sanitizers too.
//
// Coordinate: the un-stuffed bit index inside the interval (FF 00 counts as 8 bits, the first FF not followed by 00 ends the data, as
// in br_fill).  Subsequence t covers the raw bytes [t S, (t + 1) S); its first bit U[t] follows from the stuffed zero bytes before it;
// one whose first raw byte is the 00 of a pair starts a byte later.  The state between two symbols is (bit position, block in MCU j =
// 0 .. 5, coefficient index k = 0 .. 63); one step takes one whole symbol, code and extra bits, in decode_block's order of checks.
//
// Fixed point (Jacobi): exit[t] = run(t, entry[t]), entry[0] = (0, 0, 0), entry[t] = exit[t - 1] of the round before, and where that
// exit is dead (an undecodable pattern under a wrong guess) the subsequence's own guess (U[t], 0, 0): a dead state handed on would
// serialise the whole iteration.  A subsequence whose entry did not change is not decoded again; rounds run until no exit changes, at
// most one per subsequence, so termination and exactness do not depend on the data.  By induction exit[t] is true for every t up to
// the first dead exit.  Then a prefix sum of the finished-block counts gives every subsequence its first block, each is decoded once
// more from its true entry and writes (block, k) of the zeroed [blocks][64] region, DC as the difference, and one inclusive scan per
// component in int32 turns the differences into what the serial `pred` gives.  From the first block that cannot be decoded on, zeros,
// and that block's reason as the status: decode_interval_host's answer exactly.
//
// Bounded by construction, as jpeg_entropy.h: nothing outside [begin, end) is read; k never passes 63; a block index is checked
// against the caller's block count before every store; at most kSplitMaxSub subsequences per interval (above that S grows).
#pragma once
#include "jpeg_entropy.h"

namespace padel {
namespace jpeg {

constexpr int kSplitMaxSub = 4096;           // subsequences of one interval: what the kernel keeps in LDS
constexpr int kSplitMinSubBytes = 4, kSplitMaxSubBytes = 32768;
constexpr uint32_t kSplitDead = 0xffffffffu; // SplitState::pos of a state nothing can start from
constexpr int kSplitBlockEnd = 0x100;        // split_step: the symbol finished its block

struct SplitState {
    uint32_t pos;                            // un-stuffed bit index inside the interval, or kSplitDead
    uint32_t jk;                             // j | k << 3
};
PA_JHD bool split_same(SplitState a, SplitState b) { return a.pos == b.pos && a.jk == b.jk; }

// What every subsequence of one interval shares.
struct SplitCtx {
    const uint8_t* p;                        // the interval's first byte
    uint32_t len;                            // its raw bytes
    uint32_t data_end;                       // the first FF not followed by 00, or len
    uint32_t total_bits;                     // un-stuffed bits in [0, data_end)
    int sub_bytes, nsub, blocks;
    const HuffDec* tab;                      // per component: its DC table [0 .. 3), its AC table [3 .. 6)
};

// S for an interval of `len` bytes: `want`, or the next multiple of 4 at which kSplitMaxSub subsequences cover it
PA_JHD int split_sub_bytes(uint32_t len, int want) {
    if (want < kSplitMinSubBytes) want = kSplitMinSubBytes;
    const uint32_t need = ((len + kSplitMaxSub - 1) / kSplitMaxSub + 3u) & ~3u;
    return need > (uint32_t)want ? (int)need : want;
}
PA_JHD int split_count(uint32_t len, int sub_bytes) { return len ? (int)((len + (uint32_t)sub_bytes - 1) / (uint32_t)sub_bytes) : 1; }
PA_JHD uint32_t split_len(long long begin, long long end) {
    const long long len = end - begin;
    return len < 0 ? 0u : (len > kMaxFrameBytes ? (uint32_t)kMaxFrameBytes : (uint32_t)len);
}

// raw bytes [lo, hi) of the interval: how many are the 00 of an FF 00 pair, and the first FF that no 00 follows (len: none).  Before
// the data's end every FF is the first of a pair, so the count is that of the stuffed bytes wherever it is used.
PA_JHD void split_scan_bytes(const uint8_t* p, uint32_t len, uint32_t lo, uint32_t hi, uint32_t* stuffed, uint32_t* term) {
    uint32_t n = 0, first = len;
    uint32_t prev = lo > 0 && lo <= len ? p[lo - 1] : 0u;
    for (uint32_t i = lo; i < hi && i < len; ++i) {
        const uint32_t b = p[i];
        if (b == 0 && prev == 0xff) ++n;
        if (b == 0xff && first == len && (i + 1 >= len || p[i + 1] != 0)) first = i;
        prev = b;
    }
    *stuffed = n;
    *term = first;
}
// the first bit of subsequence t, given the stuffed bytes before raw byte t S (t = nsub: the end)
PA_JHD uint32_t split_first_bit(const SplitCtx* c, int t, uint32_t stuffed_before) {
    uint32_t s = (uint32_t)t * (uint32_t)c->sub_bytes;
    if (s >= c->data_end) return c->total_bits;
    if (s > 0 && c->p[s] == 0 && c->p[s - 1] == 0xff) { ++s; ++stuffed_before; }
    return 8u * (s - stuffed_before);
}

// A reader over the interval at bit `pos`, which lies in subsequence t (first bit u_t <= pos) or behind the data
PA_JHD void split_open(BitReader* r, const SplitCtx* c, int t, uint32_t pos, uint32_t u_t) {
    uint32_t s = (uint32_t)t * (uint32_t)c->sub_bytes;
    uint32_t skip = pos - u_t;
    if (s >= c->data_end || pos >= c->total_bits) { s = c->len; skip = 0; }      // behind the data: zeros
    else if (s > 0 && c->p[s] == 0 && c->p[s - 1] == 0xff) ++s;
    r->p = c->p; r->pos = s; r->end = c->len;
    r->acc = 0; r->n = 0; r->fed = 0; r->taken = 0;
    while (skip) {
        const int s16 = skip > 16 ? 16 : (int)skip;
        br_get(r, s16);
        skip -= (uint32_t)s16;
    }
    r->taken = 0;
}

// One symbol from state (base + r->taken, *j, *k).  0: inside the block; kSplitBlockEnd: it finished the block, *j moved on and *k is
// 0; else the kSt* bit of what stopped it.  *at >= 0: coefficient *at of the block is *val (at 0 the DC difference).
PA_JHD int split_step(BitReader* r, const SplitCtx* c, uint32_t base, int* j, int* k, int* at, int* val) {
    const HuffDec* dc = c->tab + (*j < 4 ? 0 : *j - 3);
    const HuffDec* ac = dc + 3;
    *at = -1;
    if (*k == 0) {
        const int s = huff_decode(r, dc);
        if (s < 0) return kStCode;
        if (s > 11) return kStSize;
        *val = s ? extend(br_get(r, s), s) : 0;
        *at = 0;
        *k = 1;
        return 0;
    }
    const int rs = huff_decode(r, ac);
    if (rs < 0) return kStCode;
    const int s = rs & 15;
    int kk = *k;
    if (s == 0) {
        if (rs == 0xf0) {
            kk += 16;
            if (kk < 64) { *k = kk; return 0; }
            if (kk > 64) return kStIndex;
        }
    } else {
        if (s > 10) return kStSize;
        kk += rs >> 4;
        if (kk > 63) return kStIndex;
        *val = extend(br_get(r, s), s);
        *at = kk++;
        if (kk < 64) { *k = kk; return 0; }
    }
    if (base + (uint32_t)r->taken > c->total_bits) { *at = -1; return kStData; }
    *j = *j == 5 ? 0 : *j + 1;
    *k = 0;
    return kSplitBlockEnd;
}

// Subsequence t from state `in` (in.pos >= u_t, its first bit): steps while the position is below `limit` and the block in hand,
// `first` and counting, is below the interval's blocks.  coef: NULL (the fixed point: first = 0) or the interval's [blocks][64]
// region.  The exit state: alive only if the position reached `limit`; dead where a symbol could not be decoded (*status its reason,
// the block in hand first + *finished) and where the blocks ran out (*status 0).
PA_JHD SplitState split_run(const SplitCtx* c, int t, SplitState in, uint32_t u_t, uint32_t limit, int first, int16_t* coef,
                            int* finished, int* status, int* symbols) {
    *finished = 0;
    *status = 0;
    const SplitState dead = {kSplitDead, 0};
    if (in.pos == kSplitDead || in.pos < u_t || first >= c->blocks) return dead;
    if (in.pos >= limit) return in;
    BitReader r;
    split_open(&r, c, t, in.pos, u_t);
    int j = (int)(in.jk & 7u), k = (int)(in.jk >> 3) & 63, b = first, n = 0;
    if (j > 5) j = 0;
    uint32_t pos = in.pos;
    while (pos < limit && b < c->blocks) {
        int at, val;
        const int rc = split_step(&r, c, in.pos, &j, &k, &at, &val);
        ++n;
        if (rc & 0xff) {
            *finished = b - first;
            *status = rc;
            *symbols += n;
            return dead;
        }
        if (coef && at >= 0) coef[(size_t)b * 64 + (size_t)at] = (int16_t)val;
        if (rc == kSplitBlockEnd) ++b;
        pos = in.pos + (uint32_t)r.taken;
    }
    *finished = b - first;
    *symbols += n;
    if (b >= c->blocks) return dead;
    const SplitState out = {pos, (uint32_t)j | (uint32_t)k << 3};
    return out;
}

// The entry of subsequence t in a round: the exit of t - 1, or the guess where that is dead
PA_JHD SplitState split_entry(int t, SplitState before, uint32_t u_t) {
    const SplitState start = {u_t, 0};
    return t == 0 || before.pos == kSplitDead ? start : before;
}

struct SplitStats {
    int sub_bytes, subsequences, rounds;
    long long symbols;           // decoded in all rounds and the write pass
    int restarts;                // entries, behind round 1, that were dead and replaced by the guess
    int passed;                  // subsequences of the true chain that a symbol begun earlier covers whole
    int stuffed_starts;          // subsequences that start on the 00 of an FF 00 pair
    int longest_block;           // subsequences the longest block of the true chain touches
};

// The whole interval on the host, by the steps of the kernel with loops for the lanes: the answer of decode_interval_host.
inline int decode_interval_split_host(const uint8_t* p, long long begin, long long end, int mcus, const HuffDec* dc[3], const HuffDec* ac[3],
                                      int sub_bytes, int16_t* coef, SplitStats* stats) {
    SplitCtx c;
    c.p = p + begin;
    c.len = split_len(begin, end);
    c.sub_bytes = split_sub_bytes(c.len, sub_bytes);
    c.nsub = split_count(c.len, c.sub_bytes);
    c.blocks = mcus > 0 ? mcus * 6 : 0;
    HuffDec* tab = new HuffDec[6];
    for (int i = 0; i < 3; ++i) { tab[i] = *dc[i]; tab[3 + i] = *ac[i]; }
    c.tab = tab;
    const int T = c.nsub;
    const size_t ncoef = (size_t)c.blocks * 64;
    for (size_t i = 0; i < ncoef; ++i) coef[i] = 0;
    SplitStats st = {c.sub_bytes, T, 0, 0, 0, 0, 0, 0};
    // the stuffed bytes before every subsequence, the end of the data
    uint32_t* pre = new uint32_t[(size_t)T + 1];
    uint32_t* U = new uint32_t[(size_t)T + 1];
    SplitState* exit_ = new SplitState[(size_t)T];
    SplitState* ent = new SplitState[(size_t)T];
    SplitState* next = new SplitState[(size_t)T];
    int* fin = new int[(size_t)T];
    c.data_end = c.len;
    pre[0] = 0;
    for (int t = 0; t < T; ++t) {
        uint32_t n, term;
        split_scan_bytes(c.p, c.len, (uint32_t)t * c.sub_bytes, (uint32_t)(t + 1) * c.sub_bytes, &n, &term);
        pre[t + 1] = pre[t] + n;
        if (term < c.data_end) c.data_end = term;
    }
    {
        const int td = (int)(c.data_end / (uint32_t)c.sub_bytes) < T ? (int)(c.data_end / (uint32_t)c.sub_bytes) : T;
        uint32_t n = 0, term;
        if (td < T) split_scan_bytes(c.p, c.len, (uint32_t)td * c.sub_bytes, c.data_end, &n, &term);
        c.total_bits = 8u * (c.data_end - pre[td] - n);
    }
    for (int t = 0; t <= T; ++t) U[t] = split_first_bit(&c, t, pre[t]);
    for (int t = 1; t < T; ++t) {
        const uint32_t s = (uint32_t)t * c.sub_bytes;
        if (s < c.data_end && c.p[s] == 0 && c.p[s - 1] == 0xff) ++st.stuffed_starts;
    }
    int status = 0;
    if (c.blocks) {
        const SplitState dead = {kSplitDead, 0}, never = {kSplitDead, 1};
        for (int t = 0; t < T; ++t) { exit_[t] = dead; ent[t] = never; fin[t] = 0; }
        for (;;) {
            bool changed = false;
            for (int t = 0; t < T; ++t) {
                next[t] = split_entry(t, t ? exit_[t - 1] : dead, U[t]);
                if (st.rounds && t && exit_[t - 1].pos == kSplitDead && !split_same(next[t], ent[t])) ++st.restarts;
            }
            for (int t = 0; t < T; ++t) {
                if (split_same(next[t], ent[t])) continue;
                ent[t] = next[t];
                int rs, sym = 0;
                const SplitState out = split_run(&c, t, ent[t], U[t], U[t + 1], 0, nullptr, &fin[t], &rs, &sym);
                st.symbols += sym;
                if (!split_same(out, exit_[t])) changed = true;
                exit_[t] = out;
            }
            ++st.rounds;
            if (!changed || st.rounds > T) break;        // (round T + 1 can only confirm)
        }
        // the true chain ends at the first dead exit; first blocks by a prefix sum; the write pass
        int last = T - 1;
        for (int t = 0; t < T; ++t)
            if (exit_[t].pos == kSplitDead) { last = t; break; }
        int first = 0, bad = c.blocks, run = 0;          // run: subsequences before t that the block in hand has touched
        for (int t = 0; t <= last; ++t) {
            int done, rs, sym = 0;
            const SplitState in = split_entry(t, t ? exit_[t - 1] : dead, U[t]);
            if (t < T - 1 && in.pos >= U[t + 1]) ++st.passed;
            split_run(&c, t, in, U[t], t == T - 1 ? kSplitDead : U[t + 1], first, coef, &done, &rs, &sym);
            st.symbols += sym;
            if (rs) { status = rs; bad = first + done; }
            const int touched = (in.jk >> 3 ? run : 0) + 1;
            if (touched > st.longest_block && first < c.blocks) st.longest_block = touched;
            run = done ? 1 : touched;
            first = first + done > c.blocks ? c.blocks : first + done;
        }
        // from the block that could not be decoded on: zeros; the DC differences summed per component
        if (bad < c.blocks)
            for (int i = 0; i < 64; ++i) coef[(size_t)bad * 64 + i] = 0;
        int32_t pred[3] = {0, 0, 0};
        for (int b = 0; b < bad; ++b) {
            const int comp = b % 6 < 4 ? 0 : b % 6 - 3;
            pred[comp] += coef[(size_t)b * 64];
            coef[(size_t)b * 64] = (int16_t)pred[comp];
        }
    }
    delete[] tab; delete[] pre; delete[] U; delete[] exit_; delete[] ent; delete[] next; delete[] fin;
    if (stats) *stats = st;
    return status;
}

}  // namespace jpeg
}  // namespace padel
