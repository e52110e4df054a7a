// codes_plan_check — csrc/lphy_codes_plan.h (the whitening generators of
// lphy_hip_whiten_batch and their reduction by the period) on the CPU, built
// with ASan + UBSan by tests/test_codes_plan_cpu.py.
//
//   codes_plan_check          1. steps every recurrence from every start state
//                             until the state returns and compares the count
//                             with the header's constants; 2. compares the
//                             header's reduced masks with the unreduced walk
//                             the reference helpers do, for every kind, rdd 0-4
//                             and position 0 .. 3 * 510 + 7 under several
//                             splits of the position into bit_ofs + j, and for
//                             every row index of SX1232; 3. for positions around
//                             INT_MAX, held in 64 bits, compares the header's
//                             table positions, step counts and masks with their
//                             direct 64-bit evaluation.
//   codes_plan_check dump     prints the header's masks of 4096 row bytes per
//                             (kind, rdd, bit_ofs), which the driver compares
//                             with the oracle's whitening of zeros.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lphy_codes_plan.h"

using namespace lphy;

static const unsigned long long kSeq[8] = LPHY_WHITEN_SEQ_INIT;
static const int kTaps[8] = LPHY_WHITEN_TAPS_INIT;
static const int kTapsCr1[5] = LPHY_WHITEN_TAPS_CR1_INIT;

static long long g_checked = 0;

#define CHECK(c, ...)                                    \
    do {                                                 \
        ++g_checked;                                     \
        if (!(c)) {                                      \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
            std::printf(__VA_ARGS__);                    \
            std::printf("\n");                           \
            return 1;                                    \
        }                                                \
    } while (0)

static const int* taps_of(unsigned rdd) { return rdd == 1 ? kTapsCr1 : kTaps; }

static unsigned header_mask(int kind, int bit_ofs, unsigned j, unsigned rdd) {
    return whiten_mask(kind, whiten_reduce_ofs(kind, bit_ofs), j, rdd, kSeq, taps_of(rdd));
}

// The masks of positions 0 .. n-1 as the reference helpers produce them: one
// walk from the start, nothing reduced (LoRaCodes.hpp:111-189).
static std::vector<uint8_t> walk(int kind, unsigned rdd, size_t n) {
    std::vector<uint8_t> m(n);
    if (kind == LPHY_WHITEN_SX1232) {
        unsigned s = kWhitenSx1232Seed;
        for (size_t p = 0; p < n; ++p) {
            m[p] = (uint8_t)s;
            for (int k = 0; k < 8; ++k) s = whiten_sx1232_step(s);
        }
    } else if (kind == LPHY_WHITEN_SX1272) {
        const int* taps = taps_of(rdd);
        for (size_t p = 0; p < n; ++p) {
            unsigned x = 0;
            for (unsigned i = 0; i < 4 + rdd; ++i) {
                const long long t = ((long long)taps[i] + (long long)p + 510) % 510;
                x |= (unsigned)((kSeq[t >> 6] >> (t & 63)) & 1ull) << i;
            }
            m[p] = (uint8_t)x;
        }
    } else {
        unsigned long long r[2] = {whiten_lfsr_seed(rdd, 0), whiten_lfsr_seed(rdd, 1)};
        const uint8_t keep = (uint8_t)(0xff >> (4 - rdd));
        for (size_t p = 0; p < n; ++p) {
            m[p] = (uint8_t)(r[p & 1] & keep);
            r[p & 1] = whiten_lfsr64_step(r[p & 1]);
        }
    }
    return m;
}

static int periods() {
    unsigned s = kWhitenSx1232Seed, n = 0;
    do {
        s = whiten_sx1232_step(s);
        ++n;
        CHECK(s < 512 && n <= 512, "SX1232 state %#x after %u steps", s, n);
    } while (s != kWhitenSx1232Seed);
    CHECK(n == kWhitenSx1232Period, "SX1232 period %u, header says %u", n, kWhitenSx1232Period);
    for (unsigned rdd = 0; rdd <= 4; ++rdd)
        for (unsigned odd = 0; odd < 2; ++odd) {
            const unsigned long long seed = whiten_lfsr_seed(rdd, odd);
            unsigned long long r = seed;
            n = 0;
            do {
                r = whiten_lfsr64_step(r);
                ++n;
                CHECK(n <= 100000, "LFSR rdd %u odd %u does not return", rdd, odd);
            } while (r != seed);
            CHECK(n == kWhitenLfsrPeriod, "LFSR rdd %u odd %u period %u, header says %u", rdd, odd, n,
                  kWhitenLfsrPeriod);
        }
    CHECK(kWhitenSeqLen == 2 * kWhitenLfsrPeriod, "two interleaved states");
    // every tap keeps tap + kWhitenSeqLen positive, which whiten_seq_pos relies on
    for (int t : kTaps) CHECK(t >= kWhitenTapMin && t + (int)kWhitenSeqLen > 0, "tap %d", t);
    for (int t : kTapsCr1) CHECK(t >= kWhitenTapMin && t + (int)kWhitenSeqLen > 0, "tap %d", t);
    return 0;
}

static int small_positions() {
    const unsigned top = 3 * 510 + 7;
    for (int kind = 0; kind < 3; ++kind)
        for (unsigned rdd = 0; rdd <= 4; ++rdd) {
            const std::vector<uint8_t> want = walk(kind, rdd, top + 1);
            for (unsigned p = 0; p <= top; ++p) {
                const unsigned splits[] = {0, 1, 3, 254, 255, 509, 510, 511, 1019, 1020, 1021, p / 2, p ? p - 1 : 0, p};
                for (unsigned ofs : splits) {
                    if (ofs > p) continue;
                    // SX1232 ignores bit_ofs: byte j is position j whatever the offset
                    const unsigned j = p - ofs, pos = kind == LPHY_WHITEN_SX1232 ? j : p;
                    const unsigned got = header_mask(kind, (int)ofs, j, rdd);
                    CHECK(got == want[pos], "kind %d rdd %u bit_ofs %u j %u: %#x, walk %#x", kind, rdd, ofs, j, got,
                          want[pos]);
                }
            }
        }
    // SX1232 over every row index the entry point admits (len <= 65535)
    const std::vector<uint8_t> want = walk(LPHY_WHITEN_SX1232, 0, 65535);
    for (unsigned j = 0; j < 65535; ++j) {
        const unsigned got = header_mask(LPHY_WHITEN_SX1232, INT_MAX, j, 7);
        CHECK(got == want[j], "SX1232 j %u: %#x, walk %#x", j, got, want[j]);
    }
    return 0;
}

static int large_positions() {
    const long long lo = (long long)INT_MAX - 65535 - 600, hi = (long long)INT_MAX + 65535;
    for (long long p = lo; p <= hi; p += 9973) {
        // p = bit_ofs + j with bit_ofs <= INT_MAX and j <= 65534: the largest
        // and the smallest bit_ofs that allow it
        long long ofs_hi = p < INT_MAX ? p : INT_MAX, ofs_lo = p - 65534;
        if (ofs_lo > INT_MAX) continue;  // only p = INT_MAX + 65535 itself: no row is that long
        for (long long ofs : {ofs_hi, ofs_lo}) {
            const unsigned j = (unsigned)(p - ofs);
            CHECK(ofs >= 0 && ofs <= INT_MAX && j <= 65534, "split of %lld", p);
            const unsigned r = whiten_reduce_ofs(LPHY_WHITEN_SX1272, (int)ofs);
            CHECK(r == (unsigned)(ofs % 510) && r == whiten_reduce_ofs(LPHY_WHITEN_SX1272_LFSR, (int)ofs),
                  "bit_ofs %lld reduced to %u", ofs, r);
            CHECK(whiten_reduce_ofs(LPHY_WHITEN_SX1232, (int)ofs) == 0, "SX1232 keeps bit_ofs %lld", ofs);
            const WhitenLfsrPlan pl = whiten_lfsr_plan(r, j);
            CHECK(pl.odd == (unsigned)(p & 1) && pl.steps == (unsigned)((p >> 1) % 255),
                  "p %lld: state %u steps %u", p, pl.odd, pl.steps);
            CHECK(whiten_sx1232_steps(j) == (unsigned)((8ll * j) % 511), "SX1232 j %u: %u steps", j,
                  whiten_sx1232_steps(j));
            for (unsigned rdd = 0; rdd <= 4; ++rdd) {
                const int* taps = taps_of(rdd);
                unsigned m1 = 0;
                for (unsigned i = 0; i < 4 + rdd; ++i) {
                    const long long q = ((long long)taps[i] + p + 510) % 510;
                    CHECK(whiten_seq_pos(taps[i], r, j) == (unsigned)q, "p %lld tap %d: %u, direct %lld", p, taps[i],
                          whiten_seq_pos(taps[i], r, j), q);
                    m1 |= (unsigned)((kSeq[q >> 6] >> (q & 63)) & 1ull) << i;
                }
                CHECK(header_mask(LPHY_WHITEN_SX1272, (int)ofs, j, rdd) == (m1 & 0xFF), "p %lld rdd %u table mask", p,
                      rdd);
                unsigned long long s = whiten_lfsr_seed(rdd, (unsigned)(p & 1));
                for (long long k = (p >> 1) % 255; k; --k) s = whiten_lfsr64_step(s);
                CHECK(header_mask(LPHY_WHITEN_SX1272_LFSR, (int)ofs, j, rdd) == (unsigned)(s & (0xffu >> (4 - rdd))),
                      "p %lld rdd %u LFSR mask", p, rdd);
                unsigned t = kWhitenSx1232Seed;
                for (long long k = (8ll * j) % 511; k; --k) t = whiten_sx1232_step(t);
                CHECK(header_mask(LPHY_WHITEN_SX1232, (int)ofs, j, rdd) == (t & 0xFF), "p %lld SX1232 mask", p);
            }
        }
    }
    return 0;
}

static void dump() {
    const int offsets[] = {0, 777};
    for (int kind = 0; kind < 3; ++kind)
        for (unsigned rdd = 0; rdd <= 4; ++rdd)
            for (int ofs : offsets) {
                std::printf("%d %u %d ", kind, rdd, ofs);
                for (unsigned j = 0; j < 4096; ++j) std::printf("%02x", header_mask(kind, ofs, j, rdd));
                std::printf("\n");
            }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "dump")) {
        dump();
        return 0;
    }
    if (periods() || small_positions() || large_positions()) return 1;
    std::printf("codes_plan_check: ok periods=%u,%u,%u checked=%lld\n", kWhitenSx1232Period, kWhitenSeqLen,
                kWhitenLfsrPeriod, g_checked);
    return 0;
}
