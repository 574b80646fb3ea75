// CPU check of csrc/conv_index.h, the index arithmetic every conv kernel shares: the XCD-aware tile map, the tile origin, the
// swizzled LDS slot offsets and fastdiv.  Stand-alone (own main, plain g++; kernels.h only for fill_fastdiv); exit status 0 = all
// checks hold, otherwise one line per failed check.  Driven by tests/test_conv_index_host.py, also under -fsanitize=address,undefined.
#include "conv_index.h"
#include "kernels.h"
#include <cstdio>
#include <vector>

using namespace padel;

static int failures = 0;
#define CHECK(COND, ...)                                                       \
    do {                                                                       \
        if (!(COND)) {                                                         \
            if (++failures <= 20) { std::printf("FAILED %s: ", #COND); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                      \
    } while (0)

// the grid the launchers size: 8 * ceil(nmt / 8) * nnt ids; every (mt, nt) from exactly one valid id, padding ids from none
static void check_tile_map(int nmt, int nnt) {
    const int grid = 8 * ((nmt + 7) / 8) * nnt;
    std::vector<int> owners(nmt * nnt, 0);
    bool padding_seen[8] = {false, false, false, false, false, false, false, false};
    int valid = 0;
    for (int bid = 0; bid < grid; ++bid) {
        const XcdSlot s = xcd_slot(nmt, nnt, bid);
        if (xcd_slot_padding(s)) { padding_seen[bid & 7] = true; continue; }
        CHECK(!padding_seen[bid & 7], "nmt %d nnt %d: id %d is valid behind a padding id of XCD %d", nmt, nnt, bid, bid & 7);
        const int mt = xcd_slot_mtile(s), nt = s.nt;
        CHECK(mt >= 0 && mt < nmt && nt >= 0 && nt < nnt, "nmt %d nnt %d: id %d -> (%d, %d)", nmt, nnt, bid, mt, nt);
        if (mt < 0 || mt >= nmt || nt < 0 || nt >= nnt) continue;
        ++owners[mt * nnt + nt];
        ++valid;
        // the next id of the same XCD: the next channel tile of the same pixel tile, then channel tile 0 of the next pixel tile
        if (bid + 8 < grid) {
            const XcdSlot t = xcd_slot(nmt, nnt, bid + 8);
            if (!xcd_slot_padding(t)) {
                const int mt2 = xcd_slot_mtile(t), nt2 = t.nt;
                const bool same_pixels = nt + 1 < nnt;
                CHECK(mt2 == (same_pixels ? mt : mt + 1) && nt2 == (same_pixels ? nt + 1 : 0),
                      "nmt %d nnt %d: id %d = (%d, %d) is followed on its XCD by (%d, %d)", nmt, nnt, bid, mt, nt, mt2, nt2);
            }
        }
    }
    CHECK(valid == nmt * nnt, "nmt %d nnt %d: %d valid ids", nmt, nnt, valid);
    for (int i = 0; i < nmt * nnt; ++i) CHECK(owners[i] == 1, "nmt %d nnt %d: tile (%d, %d) has %d owners", nmt, nnt, i / nnt, i % nnt, owners[i]);
}

// the tiles of 2^LH x 2^LW pixels cover every output pixel of every image exactly once; n changes at image boundaries only
template <int LH, int LW>
static void check_origin(int B, int Ho, int Wo) {
    constexpr int TH = 1 << LH, TW = 1 << LW;
    const int tpi = ((Ho + TH - 1) / TH) * ((Wo + TW - 1) / TW);
    std::vector<int> hits(B * Ho * Wo, 0);
    for (int mt = 0; mt < B * tpi; ++mt) {
        const TileOrigin o = tile_origin<LH, LW>(Ho, Wo, mt);
        CHECK(o.n == mt / tpi, "%d x %d tiles, %d x %d: tile %d in image %d", TH, TW, Ho, Wo, mt, o.n);
        CHECK(o.y0 >= 0 && o.y0 < Ho && o.x0 >= 0 && o.x0 < Wo && o.y0 % TH == 0 && o.x0 % TW == 0,
              "%d x %d tiles, %d x %d: tile %d at (%d, %d)", TH, TW, Ho, Wo, mt, o.y0, o.x0);
        if (o.n < 0 || o.n >= B || o.y0 < 0 || o.x0 < 0) continue;
        for (int y = o.y0; y < o.y0 + TH && y < Ho; ++y)
            for (int x = o.x0; x < o.x0 + TW && x < Wo; ++x) ++hits[(o.n * Ho + y) * Wo + x];
    }
    for (int i = 0; i < B * Ho * Wo; ++i) CHECK(hits[i] == 1, "%d x %d tiles, %d x %d: pixel %d covered %d times", TH, TW, Ho, Wo, i, hits[i]);
}

// 16-byte aligned, inside the pixel's bytes, and slot -> place a permutation per pixel
static void check_swizzle() {
    for (int p = 0; p < 192; ++p) {
        unsigned seen = 0, seen_tail = 0;
        for (int q = 0; q < 4; ++q) {
            const unsigned o = swz_off(p, q);
            CHECK(o % 16 == 0 && o >= (unsigned)p * 64 && o < (unsigned)p * 64 + 64, "swz_off(%d, %d) = %u", p, q, o);
            seen |= 1u << ((o - (unsigned)p * 64) / 16 % 32);
        }
        CHECK(seen == 0xFu, "swz_off(%d, .) is no permutation of the pixel's four slots (mask %x)", p, seen);
        for (int s = 0; s < 2; ++s) {
            const unsigned o = swz_tail_off(p, s);
            CHECK(o % 16 == 0 && o >= (unsigned)p * 32 && o < (unsigned)p * 32 + 32, "swz_tail_off(%d, %d) = %u", p, s, o);
            seen_tail |= 1u << ((o - (unsigned)p * 32) / 16 % 32);
        }
        CHECK(seen_tail == 0x3u, "swz_tail_off(%d, .) is no permutation of the pixel's two slots (mask %x)", p, seen_tail);
    }
}

static void check_fastdiv(unsigned d) {
    unsigned magic, shift;
    fill_fastdiv(d, &magic, &shift);
    const long long edge[] = {0, 1, (long long)d - 1, d, (long long)d + 1, 2147483647ll};
    for (long long n : edge) CHECK(fastdiv((int)n, magic, shift) == (int)(n / d), "%lld / %u = %d", n, d, fastdiv((int)n, magic, shift));
    unsigned long long x = 0x9E3779B97F4A7C15ull + d;          // splitmix64
    for (int i = 0; i < 4000; ++i) {
        x += 0x9E3779B97F4A7C15ull;
        unsigned long long z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        const int n = (int)((z ^ (z >> 31)) & 0x7FFFFFFFu);
        CHECK(fastdiv(n, magic, shift) == (int)((unsigned)n / d), "%d / %u = %d", n, d, fastdiv(n, magic, shift));
    }
}

int main() {
    for (int nmt : {1, 7, 8, 9, 17, 64})
        for (int nnt : {1, 2, 3}) check_tile_map(nmt, nnt);
    const int sizes[][2] = {{1, 1}, {8, 16}, {9, 17}, {20, 20}};
    for (const auto& hw : sizes) {
        check_origin<3, 4>(2, hw[0], hw[1]);
        check_origin<4, 4>(2, hw[0], hw[1]);
    }
    check_swizzle();
    for (unsigned d : {1u, 2u, 3u, 7u, 18u, 180u, 641u}) check_fastdiv(d);
    static_assert(kPatchW == 18 && kPatchPix == 180 && h2_tap_ky(5) == 2 && h2_tap_kx(5) == 1, "patch geometry, column-major taps");
    std::printf("%d checks failed\n", failures);
    return failures ? 1 : 0;
}
