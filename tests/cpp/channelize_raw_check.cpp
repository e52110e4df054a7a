// Stand-alone program over the host-compilable part of lphy_hip_channelize_raw
// (csrc/lphy_resample_plan.h, csrc/lphy_stage_plan.h), for a run under the host
// sanitizers (tests/test_channelize_raw_cpu.py):
//   - chan_stage_split, the split of a tile's span into head samples, 16-byte
//     loads and tail samples: for both sample sizes, every address offset and
//     every span length 0..40 the parts add up to the span, every load is
//     16-byte aligned, and every sample of the span is named exactly once and
//     none outside it;
//   - chan_sample_bytes for the four formats and for what is none;
//   - the two rows the call adds to chan_args, the format's and the per-format
//     alignment of d_in, and their place in the order;
//   - the host form's staging: the samples go up at the format's bytes each.
#include <cstdio>
#include <vector>

#include "lphy_resample_plan.h"
#include "lphy_stage_plan.h"

using namespace lphy;

#define EXPECT(x)                                               \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

static int split_check() {
    for (uint32_t B : {4u, 2u}) {
        const uint32_t V = 16 / B;
        for (uint32_t off = 0; off < 32; off += B)
            for (uint32_t n = 0; n <= 40; ++n) {
                const uintptr_t addr = 0x10000 + off;
                const ChanStage s = chan_stage_split(addr, n, B);
                EXPECT(s.head + V * s.vectors + s.tail == n);
                EXPECT(s.head == (n < ((16 - off % 16) % 16) / B ? n : ((16 - off % 16) % 16) / B));
                EXPECT(s.head < V && s.tail < V);
                // the kernel's walk: head sample i, vector v's samples head + V*v + j, tail sample head + V*vectors + i
                std::vector<int> named(n, 0);
                for (uint32_t i = 0; i < s.head; ++i) {
                    EXPECT(i < n);
                    ++named[i];
                }
                for (uint32_t v = 0; v < s.vectors; ++v) {
                    const uint32_t i = s.head + V * v;
                    EXPECT((addr + (uintptr_t)i * B) % 16 == 0);
                    for (uint32_t j = 0; j < V; ++j) {
                        EXPECT(i + j < n);
                        ++named[i + j];
                    }
                }
                for (uint32_t t = 0; t < s.tail; ++t) {
                    const uint32_t i = s.head + V * s.vectors + t;
                    EXPECT(i < n);
                    ++named[i];
                }
                for (uint32_t i = 0; i < n; ++i) EXPECT(named[i] == 1);
            }
    }
    // the span shorter than its head: one SC16 sample 4 bytes past a boundary
    const ChanStage s = chan_stage_split(0x1004, 1, 4);
    EXPECT(s.head == 1 && s.vectors == 0 && s.tail == 0);
    // a high address, and the longest span of the LDS path
    const ChanStage big = chan_stage_split(~uintptr_t(0) - 13, (1u << 24) - 1, 2);  // address ends in ...2
    EXPECT(big.head == 7 && big.head + 8 * big.vectors + big.tail == (1u << 24) - 1);
    return 0;
}

static int bytes_check() {
    EXPECT(chan_sample_bytes(LPHY_FMT_CF32) == 8 && chan_sample_bytes(LPHY_FMT_SC16) == 4);
    EXPECT(chan_sample_bytes(LPHY_FMT_SC8) == 2 && chan_sample_bytes(LPHY_FMT_CU8) == 2);
    EXPECT(chan_sample_bytes(-1) == 0 && chan_sample_bytes(4) == 0 && chan_sample_bytes(1 << 30) == 0);
    return 0;
}

static lphy_chan_plan good() {
    lphy_chan_plan p{};
    p.first = 3;
    p.in_samples = 1000;
    p.decim = 4;
    p.taps = 5;
    p.outputs = chan_outputs(p.in_samples, p.first, p.taps, p.decim);
    p.out_stride = p.outputs + 3;
    p.channels = 3;
    p.rot_period = 7;
    return p;
}

alignas(16) static char buf[64];

// the call's argument check as lphy_hip_channelize_raw puts it together
static int raw(const void* in, int format, const lphy_chan_plan* p, const void* taps = buf, const void* rot = buf,
               const void* out = buf, bool ctx = true) {
    return chan_args(ctx, p, taps && rot, in != nullptr, out != nullptr, chan_raw_aligned(in, format, taps, rot, out));
}

static int args_check() {
    const int formats[] = {LPHY_FMT_CF32, LPHY_FMT_SC16, LPHY_FMT_SC8, LPHY_FMT_CU8};
    lphy_chan_plan p = good();
    for (int f : formats) EXPECT(raw(buf, f, &p) == 0);
    // a format that is none of the four
    for (int f : {-1, 4, 255, 1 << 30}) EXPECT(raw(buf, f, &p) == -EINVAL);
    // ... stands in front of a misaligned pointer (both -EINVAL) and in front of every -ERANGE
    EXPECT(raw(buf + 1, 4, &p) == -EINVAL && raw(buf, 4, &p, buf + 4) == -EINVAL);
    const uint64_t k32 = uint64_t(1) << 32, k48 = uint64_t(1) << 48;
    lphy_chan_plan bad[9];
    for (lphy_chan_plan& q : bad) q = good();
    bad[0].channels = 65;
    bad[1].taps = 4097;
    bad[2].decim = 65537;
    bad[3].rot_period = 65537;
    bad[4].outputs = bad[4].out_stride = k32;
    bad[5].out_stride = bad[5].outputs - 1;
    bad[6].in_samples = k48 + 1;
    bad[7].first = 4;
    bad[8].out_stride = k48 / 3 + 1;
    for (const lphy_chan_plan& q : bad) {
        EXPECT(raw(buf, LPHY_FMT_SC16, &q) == -ERANGE && raw(buf, LPHY_FMT_CU8, &q) == -ERANGE);
        EXPECT(raw(buf, 4, &q) == -EINVAL && raw(buf, -1, &q) == -EINVAL);
    }
    // ... and behind the null-pointer rows: with the format bad as well these still refuse, and
    // with outputs == 0, where d_in and d_out are not asked for, the format still is
    EXPECT(raw(buf, 4, &p, buf, buf, buf, false) == -EINVAL && raw(buf, 4, nullptr) == -EINVAL);
    EXPECT(raw(nullptr, LPHY_FMT_SC16, &p) == -EINVAL && raw(buf, LPHY_FMT_SC16, &p, buf, buf, nullptr) == -EINVAL);
    EXPECT(raw(buf, LPHY_FMT_SC16, &p, nullptr) == -EINVAL && raw(buf, LPHY_FMT_SC16, &p, buf, nullptr) == -EINVAL);
    lphy_chan_plan none = good();
    none.outputs = 0;
    EXPECT(raw(nullptr, LPHY_FMT_SC8, &none, buf, buf, nullptr) == 0);
    EXPECT(raw(nullptr, 4, &none, buf, buf, nullptr) == -EINVAL);
    // d_in's alignment is its sample's bytes: 2 bytes off is legal for the 8-bit formats alone,
    // 4 bytes off for SC16 too, 8 bytes off for all; 1 byte off for none
    EXPECT(raw(buf + 2, LPHY_FMT_SC8, &p) == 0 && raw(buf + 2, LPHY_FMT_CU8, &p) == 0);
    EXPECT(raw(buf + 2, LPHY_FMT_SC16, &p) == -EINVAL && raw(buf + 2, LPHY_FMT_CF32, &p) == -EINVAL);
    EXPECT(raw(buf + 4, LPHY_FMT_SC16, &p) == 0 && raw(buf + 4, LPHY_FMT_CF32, &p) == -EINVAL);
    EXPECT(raw(buf + 6, LPHY_FMT_SC16, &p) == -EINVAL && raw(buf + 6, LPHY_FMT_SC8, &p) == 0);
    for (int f : formats) EXPECT(raw(buf + 8, f, &p) == 0 && raw(buf + 1, f, &p) == -EINVAL);
    // the other three pointers are asked for 8 bytes whatever the format
    for (int f : formats) {
        EXPECT(raw(buf, f, &p, buf + 4) == -EINVAL && raw(buf, f, &p, buf, buf + 2) == -EINVAL);
        EXPECT(raw(buf, f, &p, buf, buf, buf + 4) == -EINVAL && raw(buf, f, &p, buf + 8, buf + 16, buf + 24) == 0);
    }
    // the alignment row is in front of the rows behind it: reserved, a zero count, -ERANGE
    lphy_chan_plan q = good();
    q.reserved[0] = 1;
    EXPECT(raw(buf, LPHY_FMT_SC16, &q) == -EINVAL);
    q = good(), q.decim = 0;
    EXPECT(raw(buf, LPHY_FMT_SC8, &q) == -EINVAL);
    EXPECT(raw(buf + 2, LPHY_FMT_SC16, &bad[0]) == -EINVAL && raw(buf + 2, LPHY_FMT_SC8, &bad[0]) == -ERANGE);
    // LPHY_FMT_CF32 is lphy_hip_channelize's own alignment rule
    for (int a = 0; a < 16; ++a)
        EXPECT(chan_raw_aligned(buf + a, LPHY_FMT_CF32, buf, buf, buf) == res_aligned(buf + a, buf, buf, buf));
    return 0;
}

// the host form stages the span at the format's bytes a sample; the tables and the output as chan_plan
static int stage_check() {
    const lphy_chan_plan p = good();
    const size_t span = (size_t)((p.outputs - 1) * p.decim + p.taps);
    const StagePlan f = chan_plan(span, p.channels, p.taps, p.rot_period, p.out_stride);
    for (int fmt : {LPHY_FMT_CF32, LPHY_FMT_SC16, LPHY_FMT_SC8, LPHY_FMT_CU8}) {
        const size_t B = chan_sample_bytes(fmt);
        const StagePlan s = chan_raw_plan(span * B, p.channels, p.taps, p.rot_period, p.out_stride);
        EXPECT(s.n == 4 && s.s[0].size == B * span && s.s[0].role == kStageIn && s.s[0].off == 0);
        for (int i = 1; i < 4; ++i) EXPECT(s.s[i].size == f.s[i].size && s.s[i].role == f.s[i].role);
        EXPECT(s.s[1].off == align_up(B * span) && s.s[1].off % 256 == 0);
        EXPECT(s.up.begin == 0 && s.up.end == s.end && s.down.begin == s.s[3].off && s.down.end == s.end);
        if (fmt == LPHY_FMT_CF32) EXPECT(s.end == f.end);
        else EXPECT(f.end - s.end == align_up(8 * span) - align_up(B * span));
    }
    EXPECT(f.s[0].size == 8 * span);
    return 0;
}

int main() {
    if (split_check() || bytes_check() || args_check() || stage_check()) return 1;
    std::printf("channelize_raw_check: ok CF32=%d SC16=%d SC8=%d CU8=%d\n", (int)LPHY_FMT_CF32, (int)LPHY_FMT_SC16,
                (int)LPHY_FMT_SC8, (int)LPHY_FMT_CU8);
    return 0;
}
