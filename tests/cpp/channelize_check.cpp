// Stand-alone program over the host-compilable part of the channeliser
// (csrc/lphy_resample_plan.h), for a run under the host sanitizers
// (tests/test_channelize_cpu.py):
//   - every row of chan_args in the documented order, pairs of bad arguments
//     (the earlier row wins), and the overflow-prone rows with values near
//     2^32, 2^48 and 2^64;
//   - chan_outputs against a brute-force count;
//   - the tile geometry: the tiles' spans cover exactly the samples the
//     outputs read, first to last, for awkward (first, D, T, outputs);
//   - the LDS image: chan_lds_slot is strictly increasing and stays inside
//     chan_lds_slots, the lanes of a half-wave fall on at least 31 slot columns
//     at the decimations the padding is for, and chan_lds_path is the size rule;
//   - res_group.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "lphy_resample_plan.h"
#include "resample_pairs.h"

using namespace lphy;

#define EXPECT(x)                                               \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

static lphy_chan_plan good() {
    lphy_chan_plan p{};
    p.first = 3;
    p.in_samples = 1000;
    p.decim = 4;
    p.taps = 5;
    p.outputs = chan_outputs(p.in_samples, p.first, p.taps, p.decim);
    p.out_stride = p.outputs + 3;
    p.rot_first = (uint64_t(1) << 40) + 3;
    p.channels = 3;
    p.rot_period = 7;
    return p;
}

static int args(const lphy_chan_plan& p) { return chan_args(true, &p, true, true, true, true); }

static int args_check() {
    const uint64_t k32 = uint64_t(1) << 32, k48 = uint64_t(1) << 48;
    lphy_chan_plan p = good();
    EXPECT(p.outputs == 249 && args(p) == 0);
    // the -EINVAL rows, in order
    EXPECT(chan_args(false, &p, true, true, true, true) == -EINVAL);
    EXPECT(chan_args(true, nullptr, true, true, true, true) == -EINVAL);
    EXPECT(chan_args(true, &p, false, true, true, true) == -EINVAL);
    EXPECT(chan_args(true, &p, true, false, true, true) == -EINVAL);
    EXPECT(chan_args(true, &p, true, true, false, true) == -EINVAL);
    EXPECT(chan_args(true, &p, true, true, true, false) == -EINVAL);
    for (int i = 0; i < 2; ++i) {
        p = good(), p.reserved[i] = 1;
        EXPECT(args(p) == -EINVAL);
    }
    p = good(), p.channels = 0;
    EXPECT(args(p) == -EINVAL);
    p = good(), p.taps = 0;
    EXPECT(args(p) == -EINVAL);
    p = good(), p.decim = 0;
    EXPECT(args(p) == -EINVAL);
    p = good(), p.rot_period = 0;
    EXPECT(args(p) == -EINVAL);
    // no output: the sample and output pointers are not asked for, the rest is
    p = good(), p.outputs = 0;
    EXPECT(chan_args(true, &p, true, false, false, true) == 0);
    EXPECT(chan_args(true, &p, false, false, false, true) == -EINVAL);
    p.first = p.in_samples + 1;  // no tap is read, so none lies outside
    EXPECT(args(p) == 0);
    p.channels = 65;
    EXPECT(args(p) == -ERANGE);
    // res_aligned: any of the four off an 8-byte boundary, null pointers pass
    alignas(16) static char buf[32];
    EXPECT(res_aligned(buf, buf + 8, buf + 16, nullptr));
    EXPECT(!res_aligned(buf + 4, buf, buf, buf) && !res_aligned(buf, buf + 4, buf, buf));
    EXPECT(!res_aligned(buf, buf, buf + 2, buf) && !res_aligned(buf, buf, buf, buf + 1));

    // the -ERANGE rows, each at its edge
    p = good(), p.channels = 64, p.out_stride = p.outputs;
    EXPECT(args(p) == 0);
    p.channels = 65;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.taps = 4096, p.in_samples = 100000, p.outputs = 2, p.out_stride = 2;
    EXPECT(args(p) == 0);
    p.taps = 4097;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.decim = 65536, p.in_samples = 3 + 65536 + 5, p.outputs = 2;
    EXPECT(args(p) == 0);  // decim > taps is legal
    p.decim = 65537;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.rot_period = 65536;
    EXPECT(args(p) == 0);
    p.rot_period = 65537;
    EXPECT(args(p) == -ERANGE);
    // outputs < 2^32: the largest legal count, D = 1 and T = 1
    p = good(), p.decim = 1, p.taps = 1, p.first = 0, p.in_samples = k32, p.outputs = k32 - 1, p.out_stride = k32 - 1;
    EXPECT(args(p) == 0);
    p.outputs = k32, p.out_stride = k32;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.out_stride = p.outputs;
    EXPECT(args(p) == 0);
    p.out_stride = p.outputs - 1;
    EXPECT(args(p) == -ERANGE);
    // in_samples <= 2^48
    p = good(), p.in_samples = k48;
    EXPECT(args(p) == 0);
    p.first = k48 - 1000 + 3, p.out_stride = p.outputs;
    EXPECT(args(p) == 0);  // the last tap is sample 2^48 - 1
    p.first += 1;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.in_samples = k48 + 1;
    EXPECT(args(p) == -ERANGE);
    // a tap outside the capture: exact at the edge, and no wrap for a huge first
    p = good();  // 3 + 248 * 4 + 5 = 1000
    p.in_samples = 999;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.first = 4;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.first = ~uint64_t(0);
    EXPECT(args(p) == -ERANGE);
    p = good(), p.first = ~uint64_t(0) - 996;  // first + span wraps to 0
    EXPECT(args(p) == -ERANGE);
    p = good(), p.first = 1001;
    EXPECT(args(p) == -ERANGE);
    return 0;
}

// the largest product (outputs - 1) * decim the earlier rows let through, and
// the product channels * out_stride
static int args_big_product() {
    const uint64_t k32 = uint64_t(1) << 32, k48 = uint64_t(1) << 48;
    lphy_chan_plan p = good();
    p.decim = 65536, p.channels = 1, p.in_samples = k48, p.first = 0, p.taps = 1;
    // outputs = 2^32 - 1 reads up to (2^32 - 2) * 2^16 + 1 = 2^48 - 2^17 + 1 samples: inside
    p.outputs = p.out_stride = k32 - 1;
    EXPECT(args(p) == 0);
    EXPECT(chan_outputs(k48, 0, 1, 65536) == k32);  // one more would fit the capture, not the call
    p.first = (uint64_t(1) << 17) - 1;
    EXPECT(args(p) == 0);
    p.first += 1;
    EXPECT(args(p) == -ERANGE);
    // channels * out_stride <= 2^48
    p = good(), p.channels = 64, p.out_stride = k48 / 64;
    EXPECT(args(p) == 0);
    p.out_stride += 1;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.channels = 3, p.out_stride = k48 / 3;  // 3 * floor(2^48 / 3) = 2^48 - 1
    EXPECT(args(p) == 0);
    p.out_stride += 1;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.out_stride = ~uint64_t(0);  // the product would wrap
    EXPECT(args(p) == -ERANGE);
    return 0;
}

// pairs of bad arguments: the row that stands first in the header's order wins
static int args_pairs() {
    lphy_chan_plan p = good();
    p.channels = 65;  // -ERANGE alone
    EXPECT(args(p) == -ERANGE);
    EXPECT(chan_args(true, &p, true, true, true, false) == -EINVAL);
    EXPECT(chan_args(true, &p, true, true, false, true) == -EINVAL);
    p.reserved[1] = 7;
    EXPECT(args(p) == -EINVAL);
    p = good(), p.taps = 5000, p.decim = 0;
    EXPECT(args(p) == -EINVAL);
    p = good(), p.out_stride = 1, p.rot_period = 0;
    EXPECT(args(p) == -EINVAL);
    p = good(), p.in_samples = 10, p.channels = 0;
    EXPECT(args(p) == -EINVAL);
    // among the -EINVAL rows only the code is visible; among -ERANGE rows too.  Null in front of alignment:
    EXPECT(chan_args(false, nullptr, false, false, false, false) == -EINVAL);
    return 0;
}

static int outputs_check() {
    for (uint64_t n = 0; n <= 40; ++n)
        for (uint64_t first = 0; first <= 42; ++first)
            for (uint32_t T = 0; T <= 9; ++T)
                for (uint32_t D = 0; D <= 9; ++D) {
                    uint64_t brute = 0;
                    if (T && D)
                        while (first + brute * D + T <= n) ++brute;
                    EXPECT(chan_outputs(n, first, T, D) == brute);
                }
    EXPECT(chan_outputs(~uint64_t(0), ~uint64_t(0), 1, 1) == 0);
    EXPECT(chan_outputs(~uint64_t(0), ~uint64_t(0) - 1, 1, 1) == 1);
    EXPECT(chan_outputs(10, ~uint64_t(0), 4096, 65536) == 0);
    return 0;
}

static int geometry_check() {
    const uint64_t K = kChanTile;
    for (uint64_t first : {uint64_t(0), uint64_t(1), uint64_t(5), (uint64_t(1) << 40) + 7})
        for (uint32_t D : {1u, 3u, 4u, 7u, 16u, 65536u})
            for (uint32_t T : {1u, 2u, 5u, 67u, 4096u})
                for (uint64_t outputs : {uint64_t(1), K - 1, K, K + 1, 3 * K + 5}) {
                    const uint64_t tiles = res_tiles(outputs);
                    EXPECT(tiles == (outputs + K - 1) / K);
                    uint64_t seen = 0;
                    for (uint64_t t = 0; t < tiles; ++t) {
                        const ChanSpan s = chan_tile_span(first, D, T, outputs, t);
                        EXPECT(s.nout >= 1 && s.nout <= K && (t + 1 < tiles ? s.nout == K : seen + s.nout == outputs));
                        // first sample of the tile's first output, last of its last
                        const uint64_t m0 = t * K, m1 = m0 + s.nout - 1;
                        EXPECT(s.begin == first + m0 * D);
                        EXPECT(s.begin + s.samples - 1 == first + m1 * D + T - 1);
                        // lane l's taps are samples l * D + k of the span
                        for (unsigned l : {0u, s.nout - 1})
                            EXPECT((uint64_t)l * D + T - 1 < s.samples);
                        EXPECT(s.samples - 1 < (uint64_t)(K - 1) * D + T);
                        seen += s.nout;
                    }
                    EXPECT(seen == outputs);
                    // the last tap of the last output is the last sample any tile reads
                    const ChanSpan last = chan_tile_span(first, D, T, outputs, tiles - 1);
                    EXPECT(last.begin + last.samples == first + (outputs - 1) * D + T);
                }
    return 0;
}

static int lds_check() {
    for (uint32_t i = 0; i < 20000; ++i) EXPECT(chan_lds_slot(i + 1) > chan_lds_slot(i));
    EXPECT(chan_lds_slot(0) == 0 && chan_lds_slot(31) == 31 && chan_lds_slot(32) == 33);
    for (uint32_t D : {1u, 2u, 3u, 4u, 8u, 16u, 32u})
        for (uint32_t T : {1u, 5u, 129u}) {
            const uint64_t n = (uint64_t)(kChanTile - 1) * D + T;  // a full tile's span
            EXPECT(chan_lds_slots(D, T) == (uint64_t)chan_lds_slot((uint32_t)n - 1) + 1);
        }
    // 32 consecutive lanes reading sample l * D + k with one 8-byte read: the
    // slot columns (slot mod 32) they touch
    for (uint32_t D : {8u, 16u, 32u})
        for (uint32_t k = 0; k < 70; ++k)
            for (uint32_t l0 : {0u, 32u, 224u}) {
                int col[32] = {}, used = 0;
                for (uint32_t l = l0; l < l0 + 32; ++l) used += col[chan_lds_slot(l * D + k) & 31]++ == 0;
                EXPECT(used >= 31 && (k >= D || used == 32));  // unpadded: 32 / D of them
            }
    // the size rule at its edge: slots * 8 <= kResLdsBytes
    EXPECT(chan_lds_path(16, 129) && chan_lds_path(8, 65) && chan_lds_path(1, 4096) && chan_lds_path(8, 4096));
    EXPECT(!chan_lds_path(64, 4096) && !chan_lds_path(65536, 1));
    for (uint32_t D = 1; D <= 64; ++D)
        for (uint32_t T : {1u, 64u, 4096u})
            EXPECT(chan_lds_path(D, T) == (chan_lds_slots(D, T) * 8 <= kResLdsBytes));
    uint32_t Tedge = 1;
    while (chan_lds_path(24, Tedge + 1)) ++Tedge;
    EXPECT(chan_lds_slots(24, Tedge) * 8 <= kResLdsBytes && chan_lds_slots(24, Tedge + 1) * 8 > kResLdsBytes);
    // no wrap at the largest plan
    EXPECT(chan_lds_slots(65536, 4096) > (uint64_t(1) << 24));
    return 0;
}

static int group_check() {
    const unsigned want[] = {0, 1, 2, 4, 4, 8, 8, 8, 8, 8};
    for (unsigned c = 1; c < 10; ++c) EXPECT(res_group(c) == want[c]);
    EXPECT(res_group(64) == 8);
    return 0;
}

// two violations at once, one row per adjacent pair of chan_args's tests and some across the two codes
static const Pair kChanPairs[] = {
    {V_CTX, V_PLAN, -EINVAL}, {V_PLAN, V_TABLES, -EINVAL}, {V_TABLES, V_IN, -EINVAL}, {V_IN, V_OUT, -EINVAL},
    {V_OUT, V_ALIGN, -EINVAL}, {V_ALIGN, V_RES0, -EINVAL}, {V_RES0, V_RES1, -EINVAL}, {V_RES1, V_CH0, -EINVAL},
    {V_CH0, V_T0, -EINVAL}, {V_T0, V_STEP0, -EINVAL}, {V_STEP0, V_R0, -EINVAL}, {V_R0, V_CHMAX, -EINVAL},
    {V_CHMAX, V_TMAX, -ERANGE}, {V_TMAX, V_STEPMAX, -ERANGE}, {V_STEPMAX, V_RMAX, -ERANGE},
    {V_RMAX, V_OUTMAX, -ERANGE}, {V_OUTMAX, V_STRIDE_SMALL, -ERANGE}, {V_STRIDE_SMALL, V_INMAX, -ERANGE},
    {V_INMAX, V_FIRST, -ERANGE}, {V_FIRST, V_STRIDE_BIG, -ERANGE}, {V_CHMAX, V_RES0, -EINVAL},
    {V_INMAX, V_STRIDE_SMALL, -ERANGE}, {V_CHMAX, V_ALIGN, -EINVAL}, {V_OUTMAX, V_RES1, -EINVAL},
    {V_STRIDE_BIG, V_R0, -EINVAL}, {V_INMAX, V_OUT, -EINVAL}, {V_FIRST, V_CTX, -EINVAL}, {V_STEPMAX, V_T0, -EINVAL},
    {V_STRIDE_BIG, V_TABLES, -EINVAL}, {V_RMAX, V_IN, -EINVAL}, {V_FIRST, V_STEP0, -EINVAL}, {V_TMAX, V_CH0, -EINVAL},
    {V_STRIDE_SMALL, V_PLAN, -EINVAL}, {V_OUTMAX, V_IN, -EINVAL},
};

int main() {
    if (args_check() || args_big_product() || args_pairs() || outputs_check() || geometry_check() || lds_check() ||
        group_check() || pairs_check(kChanPairs, good(), chan_args, &lphy_chan_plan::decim, &lphy_chan_plan::out_stride))
        return 1;
    std::printf("channelize_check: ok kChanTile=%u sizeof(lphy_chan_plan)=%zu\n", kChanTile, sizeof(lphy_chan_plan));
    return 0;
}
