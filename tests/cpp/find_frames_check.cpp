// Stand-alone program over the host-compilable logic of the frame search
// (csrc/lphy_find_scan.h and find_frames_args of csrc/lphy_ragged_layout.h),
// for a run under the host sanitizers (tests/test_find_frames_cpu.py):
//   - the summary operator find_join, folded left to right and in random
//     bracketings, against a brute-force walk of the burst rule;
//   - find_burst against hand-computed cases;
//   - every row of find_frames_args, in the documented order, and its two
//     overflow-prone sums with values near 2^64;
//   - find_layout: aligned parts that do not overlap.
#include <cstdio>
#include <random>
#include <vector>

#include "lphy_find_scan.h"

using namespace lphy;

#define EXPECT(x)                                               \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

static bool same(const FindSum& a, const FindSum& b) {
    return a.first == b.first && a.last == b.last && a.start == b.start;
}

// the burst rule walked over windows [lo, hi) alone
static FindSum brute(const std::vector<char>& act, uint32_t lo, uint32_t hi, uint32_t max_gap) {
    FindSum s = kFindEmpty;
    for (uint32_t w = lo; w < hi; ++w) {
        if (!act[w]) continue;
        if (s.first == kFindNone) s.first = s.start = w;
        else if (w - s.last - 1 > max_gap) s.start = w;
        s.last = w;
    }
    return s;
}

static FindSum bracket(const std::vector<char>& act, uint32_t lo, uint32_t hi, uint32_t max_gap, std::mt19937& rng) {
    if (hi == lo) return kFindEmpty;
    if (hi - lo == 1) return find_leaf(lo, act[lo]);
    const uint32_t mid = lo + 1 + rng() % (hi - lo - 1);
    return find_join(bracket(act, lo, mid, max_gap, rng), bracket(act, mid, hi, max_gap, rng), max_gap);
}

static int operator_check() {
    std::mt19937 rng(20240611);
    for (uint32_t max_gap : {0u, 1u, 5u, 400u}) {
        for (int trial = 0; trial < 400; ++trial) {
            const uint32_t n = rng() % 301;
            const unsigned p = trial % 4 == 0 ? 2 : (trial % 4 == 1 ? 10 : (trial % 4 == 2 ? 50 : 97));
            std::vector<char> act(n);
            for (auto& a : act) a = rng() % 100 < p;
            // the bursts by a walk: starts[] and ends[]
            std::vector<uint32_t> starts, ends;
            for (uint32_t w = 0; w < n; ++w) {
                if (!act[w]) continue;
                if (ends.empty() || w - ends.back() - 1 > max_gap) starts.push_back(w), ends.push_back(w);
                else ends.back() = w;
            }
            // left to right: every prefix's summary, and the bursts the fold
            // closes (at the start of the next one, and at the end)
            FindSum fold = kFindEmpty;
            std::vector<uint32_t> fstarts, fends;
            for (uint32_t w = 0; w <= n; ++w) {
                EXPECT(same(fold, brute(act, 0, w, max_gap)));
                const bool starts_one = w < n && act[w] && (fold.last == kFindNone || w - fold.last - 1 > max_gap);
                if (fold.last != kFindNone && (starts_one || w == n)) fstarts.push_back(fold.start), fends.push_back(fold.last);
                if (w < n) fold = find_join(fold, find_leaf(w, act[w]), max_gap);
            }
            EXPECT(fstarts == starts && fends == ends);
            // random bracketings of the whole and of random segments
            for (int k = 0; k < 4; ++k) EXPECT(same(bracket(act, 0, n, max_gap, rng), fold));
            for (int k = 0; k < 8 && n; ++k) {
                const uint32_t lo = rng() % n, hi = lo + rng() % (n - lo + 1);
                EXPECT(same(bracket(act, lo, hi, max_gap, rng), brute(act, lo, hi, max_gap)));
            }
        }
    }
    return 0;
}

static int burst_check() {
    // S = 128, hop = S: windows 3 .. 7 are 5 symbols at 3 * 128
    FindGeo g{0, 128, 0, 1 << 20, 128, 0, 1, LPHY_MODE_DECHIRP_LORA_DEMODULATE};
    FindBurst b = find_burst(g, 3, 7);
    EXPECT(b.start == 384 && b.total == 5 && b.out_syms == 4 && b.fate == kFindKept);
    // first and lead move the start; mode 0 and 1 agree from two symbols on
    g.first = 1000, g.lead = 64;
    b = find_burst(g, 3, 7);
    EXPECT(b.start == 1000 + 64 + 384 && b.total == 5);
    g.mode = LPHY_MODE_DEMODULATE;
    EXPECT(find_burst(g, 3, 7).out_syms == 4 && find_burst(g, 3, 3).out_syms == 0);
    g.mode = LPHY_MODE_LORA_DEMODULATE;
    EXPECT(find_burst(g, 3, 3).out_syms == 2 && find_burst(g, 3, 3).total == 1);  // (1 + 1) & ~1
    EXPECT(find_burst(g, 3, 4).out_syms == 0 && find_burst(g, 3, 5).out_syms == 2);
    // hop = S / 4: 9 windows span 9 * 32 = 288 samples = 2 whole symbols
    g = FindGeo{0, 32, 64, 1 << 20, 128, 0, 1, LPHY_MODE_DECHIRP_LORA_DEMODULATE};
    b = find_burst(g, 10, 18);
    EXPECT(b.start == 64 + 320 && b.total == 2 && b.fate == kFindKept);
    // min_symbols
    g.min_symbols = 3;
    EXPECT(find_burst(g, 10, 18).fate == kFindShort);
    EXPECT(find_burst(g, 10, 21).total == 3 && find_burst(g, 10, 21).fate == kFindKept);
    // the clip at total_samples: 5 windows of 128 at 384, the capture ends at 384 + 300
    g = FindGeo{0, 128, 0, 684, 128, 0, 1, LPHY_MODE_DECHIRP_LORA_DEMODULATE};
    b = find_burst(g, 3, 7);
    EXPECT(b.start == 384 && b.total == 2 && b.fate == kFindKept);
    g.total_samples = 384 + 127;  // not one whole symbol left
    EXPECT(find_burst(g, 3, 7).total == 0 && find_burst(g, 3, 7).fate == kFindShort);
    // start >= total_samples: extent 0, no difference formed
    g.total_samples = 384;
    EXPECT(find_burst(g, 3, 7).total == 0 && find_burst(g, 3, 7).fate == kFindShort);
    g.total_samples = 10;
    EXPECT(find_burst(g, 3, 7).total == 0);
    // the 2^31 drop: hop = 2^24, 128 windows are exactly 2^31 samples; 127 are below
    g = FindGeo{0, uint64_t(1) << 24, 0, uint64_t(1) << 40, 128, 0, 1, LPHY_MODE_DECHIRP_LORA_DEMODULATE};
    EXPECT(find_burst(g, 0, 127).total * 128 == (uint64_t(1) << 31) && find_burst(g, 0, 127).fate == kFindLong);
    EXPECT(find_burst(g, 5, 131).fate == kFindKept && find_burst(g, 5, 131).total == (127u << 24) / 128);
    g.min_symbols = 0xffffffffu;  // short is asked first
    EXPECT(find_burst(g, 0, 127).fate == kFindShort);
    // the last window of the largest call: nothing wraps
    g = FindGeo{(uint64_t(1) << 48) - 0xffffffffull, 1, 0, uint64_t(1) << 48, 128, 0, 1, LPHY_MODE_DEMODULATE};
    b = find_burst(g, 0, 0xfffffffeu);
    EXPECT(b.start == g.first && b.total == 0xffffffffull / 128 && b.fate == kFindLong);
    return 0;
}

static int args_check() {
    const RaggedCtx ctx{true, 7, 1}, none{false, 0, 0};
    lphy_find_params p{};
    p.hop = 128, p.total_samples = 1 << 20, p.threshold_db = 10.0f, p.min_symbols = 1;
    const uint64_t S = 128;
    auto call = [&](RaggedCtx c, const lphy_find_params* q, bool ptrs, bool rec, bool work, uint64_t windows, int mode,
                    uint64_t max_frames) { return find_frames_args(c, q, ptrs, rec, work, S, windows, mode, max_frames); };
    EXPECT(call(ctx, &p, true, true, true, 100, 2, 8) == 0);
    EXPECT(call(ctx, &p, true, false, true, 0, 0, 1) == 0);  // no records needed for no windows
    // -EINVAL, row by row (the order that shows is -EINVAL before -ERANGE, below)
    lphy_find_params bad = p;
    EXPECT(call(none, nullptr, false, false, false, uint64_t(1) << 40, 9, 0) == -EINVAL);
    EXPECT(call(none, &p, true, true, true, 100, 2, 8) == -EINVAL);
    EXPECT(call(ctx, nullptr, true, true, true, 100, 2, 8) == -EINVAL);
    EXPECT(call(ctx, &p, false, true, true, 100, 2, 8) == -EINVAL);
    EXPECT(call(ctx, &p, true, false, true, 100, 2, 8) == -EINVAL);
    EXPECT(call(ctx, &p, true, true, false, 100, 2, 8) == -EINVAL);
    bad = p, bad.hop = 0;
    EXPECT(call(ctx, &bad, true, true, true, 100, 2, 8) == -EINVAL);
    bad = p, bad.min_symbols = 0;
    EXPECT(call(ctx, &bad, true, true, true, 100, 2, 8) == -EINVAL);
    EXPECT(call(ctx, &p, true, true, true, 100, 2, 0) == -EINVAL);
    bad = p, bad.threshold_db = __builtin_nanf("");
    EXPECT(call(ctx, &bad, true, true, true, 100, 2, 8) == -EINVAL);
    bad = p, bad.threshold_db = __builtin_inff();  // an infinite threshold is a threshold
    EXPECT(call(ctx, &bad, true, true, true, 100, 2, 8) == 0);
    bad.threshold_db = -__builtin_inff();
    EXPECT(call(ctx, &bad, true, true, true, 100, 2, 8) == 0);
    bad = p, bad.reserved = 1;
    EXPECT(call(ctx, &bad, true, true, true, 100, 2, 8) == -EINVAL);
    EXPECT(call(ctx, &p, true, true, true, 100, -1, 8) == -EINVAL);
    EXPECT(call(ctx, &p, true, true, true, 100, 3, 8) == -EINVAL);
    // every -EINVAL comes before every -ERANGE
    EXPECT(call(ctx, &p, true, true, true, uint64_t(1) << 32, 3, uint64_t(1) << 31) == -EINVAL);
    bad = p, bad.reserved = 1, bad.first = ~uint64_t(0);
    EXPECT(call(ctx, &bad, true, true, true, uint64_t(1) << 32, 2, uint64_t(1) << 31) == -EINVAL);
    // -ERANGE: windows
    lphy_find_params one = p;
    one.hop = 1;
    EXPECT(call(ctx, &one, true, true, true, (uint64_t(1) << 32) - 1, 2, 8) == 0);
    EXPECT(call(ctx, &one, true, true, true, uint64_t(1) << 32, 2, 8) == -ERANGE);
    EXPECT(call(ctx, &one, true, true, true, ~uint64_t(0), 2, 8) == -ERANGE);
    // max_frames
    EXPECT(call(ctx, &p, true, true, true, 100, 2, 0x7fffffff) == 0);
    EXPECT(call(ctx, &p, true, true, true, 100, 2, uint64_t(1) << 31) == -ERANGE);
    EXPECT(call(ctx, &p, true, true, true, 100, 2, ~uint64_t(0)) == -ERANGE);
    // first + lead + windows * hop <= 2^48, none of it wrapping
    const uint64_t top = uint64_t(1) << 48;
    bad = p, bad.hop = 128, bad.first = top - 100 * 128;
    EXPECT(call(ctx, &bad, true, true, true, 100, 2, 8) == 0);
    bad.first += 1;
    EXPECT(call(ctx, &bad, true, true, true, 100, 2, 8) == -ERANGE);
    bad.first -= 1, bad.lead = 1;
    EXPECT(call(ctx, &bad, true, true, true, 100, 2, 8) == -ERANGE);
    bad = p, bad.first = ~uint64_t(0);          // first + anything wraps
    EXPECT(call(ctx, &bad, true, true, true, 1, 2, 8) == -ERANGE);
    bad = p, bad.first = 5, bad.lead = ~uint64_t(0) - 4;  // first + lead wraps to 0
    EXPECT(call(ctx, &bad, true, true, true, 1, 2, 8) == -ERANGE);
    bad = p, bad.lead = top, bad.hop = 1;       // no room for one window
    EXPECT(call(ctx, &bad, true, true, true, 0, 2, 8) == 0);
    EXPECT(call(ctx, &bad, true, true, true, 1, 2, 8) == -ERANGE);
    bad = p, bad.hop = ~uint64_t(0);            // windows * hop wraps to a small number
    EXPECT(call(ctx, &bad, true, true, true, 2, 2, 8) == -ERANGE);
    bad = p, bad.hop = (uint64_t(1) << 63) + 1;
    EXPECT(call(ctx, &bad, true, true, true, 2, 2, 8) == -ERANGE);
    bad = p, bad.hop = uint64_t(1) << 32;       // 2^32 * 2^32 wraps to 0
    EXPECT(call(ctx, &bad, true, true, true, (uint64_t(1) << 32) - 1, 2, 8) == -ERANGE);
    // windows * hop / S < 2^32: 2^39 / 128 = 2^32 is refused, one window less is not
    bad = p, bad.hop = 128;
    EXPECT(call(ctx, &bad, true, true, true, (uint64_t(1) << 32) - 1, 2, 8) == 0);
    bad.hop = 256;
    EXPECT(call(ctx, &bad, true, true, true, uint64_t(1) << 31, 2, 8) == -ERANGE);
    EXPECT(call(ctx, &bad, true, true, true, (uint64_t(1) << 31) - 1, 2, 8) == 0);
    return 0;
}

static int layout_check() {
    for (uint64_t windows : {uint64_t(0), uint64_t(1), uint64_t(1023), uint64_t(1024), uint64_t(1025), uint64_t(40000),
                             (uint64_t(1) << 32) - 1}) {
        const FindLayout l = find_layout(windows);
        EXPECT(l.tiles * kFindTile > windows);  // item `windows` has a tile
        EXPECT((l.tiles - 1) * kFindTile <= windows);
        const size_t at[7] = {l.totals, l.bits, l.sums, l.carry, l.counts, l.prefix, l.bytes};
        const size_t need[6] = {sizeof(FindTotals),
                                (size_t)l.tiles * (kFindTile / 64) * 8,
                                (size_t)l.tiles * sizeof(FindSum),
                                (size_t)l.tiles * 8,
                                (size_t)l.tiles * sizeof(FindTileCount),
                                (size_t)l.tiles * sizeof(FindTilePrefix)};
        for (int i = 0; i < 6; ++i) EXPECT(at[i] % 16 == 0 && at[i] + need[i] <= at[i + 1]);
        EXPECT(l.bytes > 0 && l.bytes % 16 == 0);
    }
    return 0;
}

int main() {
    if (operator_check() || burst_check() || args_check() || layout_check()) return 1;
    std::printf("find_frames_check: ok\n");
    return 0;
}
