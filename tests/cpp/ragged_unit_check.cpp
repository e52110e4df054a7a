// Host-only test library over csrc/lphy_ragged_unit.h: ragged_unit<false> as
// the kernels compile it, for every unit of a caller's table
// (tests/test_ragged_unit_cpu.py loads it through ctypes), and
// lphy_hip_ragged_layout's table builder beside it.  With -DRAGGED_UNIT_MAIN it
// is a stand-alone program over the same helpers, for a run under the host
// sanitizers.
#include "lphy_ragged_layout.h"
#include "lphy_ragged_unit.h"

using namespace lphy;

extern "C" int ru_layout_check(uint64_t step, const uint64_t* h_samples, size_t frames, lphy_ragged_desc* h_desc) {
    return ragged_layout(step, h_samples, frames, LPHY_MODE_LORA_DEMODULATE, h_desc);
}

// out[4 q .. 4 q + 3] = {frame, s, live, the record read was record `frame`} for u = first + q
extern "C" void ru_units_check(const lphy_ragged_desc* desc, unsigned frames, uint64_t units, uint64_t first,
                               size_t queries, uint64_t* out) {
    for (size_t q = 0; q < queries; ++q) {
        const RaggedUnit r = ragged_unit<false>(desc, frames, units, first + q);
        const lphy_ragged_desc& d = desc[r.frame];
        out[4 * q] = r.frame;
        out[4 * q + 1] = r.s;
        out[4 * q + 2] = r.live;
        out[4 * q + 3] = r.d.iq_offset == d.iq_offset && r.d.samples == d.samples && r.d.sym_offset == d.sym_offset &&
                         r.d.unit_offset == d.unit_offset;
    }
}

#ifdef RAGGED_UNIT_MAIN
#include <cstdio>

#define EXPECT(x)                                               \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

// every u in [0, units + 2) of a heap table of exactly frames + 1 records, so
// that a read past either end is the sanitizer's to see
static int walk(const std::vector<lphy_ragged_desc>& t, bool sound) {
    const unsigned frames = (unsigned)t.size() - 1;
    const uint64_t units = t[frames].unit_offset;
    for (uint64_t u = 0; u < units + 2; ++u) {
        const RaggedUnit r = ragged_unit<false>(t.data(), frames, units, u);
        EXPECT(r.frame < frames);
        if (u >= units) EXPECT(!r.live && r.frame == 0 && r.d.iq_offset == t[0].iq_offset);
        if (r.live) EXPECT(r.d.unit_offset <= u && r.s == u - r.d.unit_offset);
        if (sound && u < units) {
            unsigned want = 0;  // the last record whose unit_offset is <= u
            for (unsigned f = 0; f < frames; ++f)
                if (t[f].unit_offset <= u) want = f;
            EXPECT(r.live && r.frame == want);
        }
    }
    return 0;
}

int main() {
    const uint64_t step = 128;
    const uint64_t pat[8] = {0, 0, 0, 1, 2, 3, 4, 5};
    for (size_t frames : {size_t(1), size_t(2), size_t(3), size_t(8), size_t(601)}) {
        std::vector<uint64_t> samples(frames);
        for (size_t f = 0; f < frames; ++f) samples[f] = pat[f % 8] * step + (f % 3);
        std::vector<lphy_ragged_desc> t(frames + 1);
        EXPECT(ragged_layout(step, samples.data(), frames, LPHY_MODE_LORA_DEMODULATE, t.data()) == 0);
        if (walk(t, true)) return 1;
        if (frames < 3) continue;
        // forged: a non-monotone prefix, a first record past 0, a total past the sum
        std::vector<lphy_ragged_desc> bad = t;
        bad[frames / 2].unit_offset = t[frames].unit_offset + 7;
        if (walk(bad, false)) return 1;
        bad = t;
        bad[0].unit_offset = 3;
        if (walk(bad, false)) return 1;
        bad = t;
        bad[frames].unit_offset += 9;
        if (walk(bad, false)) return 1;
    }
    std::printf("ragged_unit_check: ok\n");
    return 0;
}
#endif
