// The input-patch index math of the fused stem + layer-1 kernel (csrc/conv_index.h: stem_patch_*, stem_lq_*, stem_pair_*) on the
// CPU.  Stages a random u8 NHWC4 frame (the middle one of three, so a read across a frame boundary shows) into a host copy of the
// LDS patch exactly as the kernel's threads do, builds every MFMA operand slot from it the way a lane does (four words, a byte
// permute per slot pair, 0x6400 | byte minus 1024), and compares with the direct per-slot formula: K slot k = 3 tap + colour of
// stem position p of the tile at (oy0, ox0) is byte `colour` of input pixel (4 oy0 - 3 + 2 srow + dy, 4 ox0 - 3 + 2 scol + dx),
// 0 outside the image.  Images 32 x 32 and 64 x 160, every tile (corners, edges, interior, the partial last column), every
// p < 297, every k < 32.  Prints one line per failed check and "<n> checks failed".
#include "conv_index.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace padel;

static int failed = 0;
static long long checked = 0;
#define CHECK(cond_, ...)                                        \
    do {                                                         \
        ++checked;                                               \
        if (!(cond_)) {                                          \
            if (++failed <= 20) { printf(__VA_ARGS__); printf("\n"); } \
        }                                                        \
    } while (0)

// v_perm_b32 D = perm(S0, S1, sel): selector byte 0..3 -> that byte of S1, 4..7 -> of S0, 0x0c -> 0x00
static uint32_t perm_b32(uint32_t s0, uint32_t s1, uint32_t sel) {
    uint32_t d = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = (sel >> (8 * i)) & 255u;
        uint32_t b = 0;
        if (s < 4) b = (s1 >> (8 * s)) & 255u;
        else if (s < 8) b = (s0 >> (8 * (s - 4))) & 255u;
        else if (s != 0x0cu) { b = 0xee; CHECK(false, "selector byte %#x is none of 0..7, 0x0c", s); }
        d |= b << (8 * i);
    }
    return d;
}

// fp16 bits 0x64bb = 1024 + bb; minus 1024: the byte
static int half_minus_1024(uint32_t h) {
    CHECK((h >> 8) == 0x64u, "half %#x is not 0x6400 | byte", h);
    return (int)(h & 255u);
}

static void run(int H, int W, uint32_t seed) {
    const int Ho1 = H / 4, Wo1 = W / 4;
    std::vector<uint32_t> frames((size_t)3 * H * W);
    for (auto& px : frames) { seed = seed * 1664525u + 1013904223u; px = (seed >> 4) | 0x01010101u; }      // no zero byte: a zero is a padding tap
    const uint32_t* img = frames.data() + (size_t)H * W;
    const TileOrigin last = tile_origin<2, 4>(Ho1, Wo1, ((Ho1 + 3) / 4) * ((Wo1 + 15) / 16) - 1);
    CHECK(last.n == 0, "tile count");
    for (int oy0 = 0; oy0 < Ho1; oy0 += 4)
        for (int ox0 = 0; ox0 < Wo1; ox0 += 16) {
            // staging: chunk c by "thread" c
            std::vector<uint32_t> patch(kStemPatchB / 4 + 4, 0xdeadbeefu);
            for (int c = 0; c < 512; ++c) {
                if (c >= kStemPatchChunks) continue;
                const int iy = stem_patch_y0(oy0) + stem_patch_chunk_row(c), ix0 = stem_patch_x0(ox0) + stem_patch_chunk_col(c);
                const bool in = stem_patch_chunk_inside(H, W, iy, ix0);
                int n_in = 0;
                for (int e = 0; e < 4; ++e) n_in += iy >= 0 && iy < H && ix0 + e >= 0 && ix0 + e < W;
                CHECK(n_in == (in ? 4 : 0), "chunk %d of tile (%d, %d): %d of 4 pixels inside, predicate %d", c, oy0, ox0, n_in, (int)in);
                for (int e = 0; e < 4; ++e) patch[(size_t)c * 4 + e] = in ? img[(size_t)iy * W + ix0 + e] : 0u;
            }
            for (int e = 0; e < 4; ++e) CHECK(patch[kStemPatchB / 4 + e] == 0xdeadbeefu, "write past the patch");
            for (int p = 0; p < 297; ++p) {
                const int srow = p / 33, scol = p % 33;
                for (int lq = 0; lq < 4; ++lq) {
                    uint32_t wd[4];
                    for (int i = 0; i < 4; ++i) {
                        const int t = stem_lq_word_tap(lq, i);
                        const int word = stem_patch_tap_word(p, 0, 0) + (t / 3) * kStemPatchRowW + t % 3;
                        CHECK(t >= 0 && t < 9 && word == stem_patch_tap_word(p, t / 3, t % 3) && word >= 0 && word < kStemPatchB / 4,
                              "word %d of lane group %d at p %d: tap %d word %d", i, lq, p, t, word);
                        wd[i] = patch[word];
                    }
                    for (int j = 0; j < 4; ++j) {
                        const int lo = stem_pair_word(j);
                        const uint32_t two = perm_b32(wd[lo + 1], wd[lo], stem_pair_selector(lq, j)) | 0x64006400u;
                        for (int hlf = 0; hlf < 2; ++hlf) {
                            const int k = 8 * lq + 2 * j + hlf;
                            const int got = half_minus_1024((two >> (16 * hlf)) & 0xffffu);
                            int want = 0;
                            if (k < 27) {
                                const int tap = k / 3, col = k % 3, dy = tap / 3, dx = tap % 3;
                                const int sy = 2 * oy0 - 1 + srow, sx = 2 * ox0 - 1 + scol;
                                const int iy = 2 * sy - 1 + dy, ix = 2 * sx - 1 + dx;
                                if (iy >= 0 && iy < H && ix >= 0 && ix < W) want = (int)((img[(size_t)iy * W + ix] >> (8 * col)) & 255u);
                            }
                            CHECK(got == want, "%d x %d tile (%d, %d) p %d k %d: operand %d, direct %d", H, W, oy0, ox0, p, k, got, want);
                        }
                    }
                }
            }
        }
}

int main() {
    static_assert(kStemPatchChunks == 342 && kStemPatchB == 5472, "19 rows x 72 words");
    static_assert(stem_lq_words(0) == 3 && stem_lq_words(1) == 4 && stem_lq_words(2) == 3 && stem_lq_words(3) == 1, "spans per lane group");
    run(32, 32, 1u);
    run(64, 160, 2u);
    printf("%lld checks, %d checks failed\n", checked, failed);
    return failed ? 1 : 0;
}
