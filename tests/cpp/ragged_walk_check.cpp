// Host-only test library over csrc/lphy_ragged_layout.h: the one walk over a
// caller's table as each *_host form calls it, and the ragged entry points'
// argument checks (tests/test_ragged_walk_cpu.py loads it through ctypes).
// With -DRAGGED_WALK_MAIN it is a stand-alone program over the same two, on
// heap tables of exactly frames + 1 records, for a run under the host
// sanitizers.
#include "lphy_ragged_layout.h"

using namespace lphy;

enum { kDemod, kDetect, kEstimate, kTx, kCompensate };  // kTx: modulate_ragged and both tx_ragged forms

// The table check of caller `who`'s host form.  out (written when 0 is
// returned): demod iq_samples, out_syms; detect iq_samples, units; estimate
// iq_samples; tx iq_samples, out_syms, in_bytes, iq_gaps, sym_gaps.
extern "C" int rw_walk(int who, uint64_t step, const lphy_ragged_desc* desc, size_t frames, int mode, uint64_t* out) {
    if (who == kDemod) return ragged_extent(step, desc, frames, mode, &out[0], &out[1]);
    if (who == kDetect) return detect_ragged_extent(step, desc, frames, &out[0], &out[1]);
    if (who == kEstimate) return estimate_ragged_extent(desc, frames, &out[0]);
    TxExtent t;
    const int rc = who == kTx ? tx_extent(step, desc, frames, &t) : -1;
    if (rc) return rc;
    const uint64_t v[5] = {t.iq_samples, t.out_syms, t.in_bytes, t.iq_gaps, t.sym_gaps};
    for (int i = 0; i < 5; ++i) out[i] = v[i];
    return 0;
}

// a: ctx (0: null), sf, osr, frames, ptrs (0: a required pointer is null), mode,
// flags, phase, bytes (0: null).  1 (nothing to do) comes back as the entry point's 0.
extern "C" int rw_args(int who, const uint64_t* a) {
    const RaggedCtx c{a[0] != 0, (unsigned)a[1], (unsigned)a[2]};
    const size_t frames = a[3];
    const bool ptrs = a[4] != 0;
    int rc = -1;
    switch (who) {
        case kDemod: rc = demod_ragged_args(c, ptrs, (int)a[5], (unsigned)a[6], a[8] != 0, frames); break;
        case kDetect: rc = detect_ragged_args(c, frames, ptrs, (unsigned)a[7], (unsigned)a[6]); break;
        case kEstimate:
        case kTx: rc = ragged_args(c, frames, ptrs); break;
        case kCompensate: rc = ragged_args(c, frames, ptrs, 0); break;
    }
    return rc > 0 ? 0 : rc;
}

#ifdef RAGGED_WALK_MAIN
#include <cstdio>

#define EXPECT(x)                                               \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

using Table = std::vector<lphy_ragged_desc>;
constexpr uint64_t kStep = 128, kBig = kRaggedMaxSamples - kStep;  // 2^24 - 1 symbols
constexpr uint64_t kUntouched = 0xABABABABABABABABull;

static Table packed(const std::vector<uint64_t>& samples) {
    Table t(samples.size() + 1);
    uint64_t iq = 0, sym = 0, unit = 0;  // (ragged_layout refuses 2^32 units: laid out here)
    for (size_t f = 0; f < samples.size(); ++f) {
        t[f] = lphy_ragged_desc{iq, samples[f], sym, unit};
        iq += samples[f];
        sym += (ragged_out_syms(samples[f] / kStep, LPHY_MODE_LORA_DEMODULATE) + 1) & ~uint64_t(1);
        unit += samples[f] / kStep;
    }
    t[samples.size()] = lphy_ragged_desc{iq, 0, sym, unit};
    return t;
}

enum Fault { kSamples, kPrefix, kIq, kSym, kFaults };

static void forge(Table& t, int fault, size_t f) {
    if (fault == kSamples) t[f].samples = kRaggedMaxSamples;
    if (fault == kPrefix) t[f].unit_offset += 1;
    if (fault == kIq) t[f].iq_offset = kRaggedMaxOffset + 1;
    if (fault == kSym) t[f].sym_offset = kRaggedMaxOffset + 1;
}

// what a single fault costs caller `who` (0: the caller does not read the field)
static int code(int who, int fault) {
    if (fault == kFaults) return 0;  // (none)
    if (fault == kPrefix) return who == kEstimate ? 0 : -EINVAL;
    if (fault == kSym) return who == kDemod || who == kTx ? -ERANGE : 0;
    return -ERANGE;
}

// every caller on table t, forged with faults a and b (kFaults: none): the
// code is one of theirs, and a refused table leaves the outputs alone
static int run(const Table& t, int a, int b) {
    for (int who = kDemod; who <= kTx; ++who) {
        uint64_t out[5] = {kUntouched, kUntouched, kUntouched, kUntouched, kUntouched};
        const int rc = rw_walk(who, kStep, t.data(), t.size() - 1, LPHY_MODE_LORA_DEMODULATE, out);
        const int ca = code(who, a), cb = code(who, b);
        if (ca || cb) EXPECT(rc != 0 && (rc == ca || rc == cb));
        else EXPECT(rc == 0 || (who == kTx && rc == -EINVAL));
        if (rc) EXPECT(out[0] == kUntouched && out[4] == kUntouched);
        else EXPECT(out[0] != kUntouched);
    }
    return 0;
}

int main() {
    const std::vector<uint64_t> base = {4 * kStep, 0,         2 * kStep, 6 * kStep + 5, 37,
                                        66 * kStep, 3 * kStep, kStep,     2 * kStep};
    const size_t n = base.size();
    const Table sound = packed(base);
    if (run(sound, kFaults, kFaults)) return 1;
    for (int a = 0; a < kFaults; ++a)
        for (size_t f : {size_t(0), n / 2, n - 1, n}) {
            if (f == n && a != kPrefix) continue;  // record [frames]: the total alone is read
            Table t = sound;
            forge(t, a, f);
            if (run(t, a, kFaults)) return 1;
            for (int b = 0; b < kFaults; ++b)
                for (size_t g : {size_t(0), n / 2, n - 1}) {
                    if (b == a || g == f) continue;
                    Table u = t;
                    forge(u, b, g);
                    if (run(u, a, b)) return 1;
                }
        }
    // 2^32 whole symbols, reached in the table's last frame, alone and behind another fault
    std::vector<uint64_t> many = base;
    many.insert(many.end(), 257, kBig);
    const Table full = packed(many);
    for (int who = kDemod; who <= kTx; ++who) {
        uint64_t out[5];
        const int mode = LPHY_MODE_LORA_DEMODULATE;
        EXPECT(rw_walk(who, kStep, full.data(), many.size(), mode, out) == (who == kEstimate ? 0 : -ERANGE));
        // (one frame fewer stays below, and the next record's prefix is that total: base's odd frames are tx's alone)
        EXPECT(rw_walk(who, kStep, full.data(), many.size() - 1, mode, out) == (who == kTx ? -EINVAL : 0));
    }
    for (int a = 0; a < kFaults; ++a)
        for (int who = kDemod; who <= kTx; ++who) {
            Table t = full;
            forge(t, a, 1);
            uint64_t out[5];
            const int rc = rw_walk(who, kStep, t.data(), many.size(), LPHY_MODE_LORA_DEMODULATE, out);
            EXPECT(rc == (code(who, a) ? code(who, a) : who == kEstimate ? 0 : -ERANGE));
        }
    // the checks: every entry point over a grid of plain values, codes in range
    for (int who = kDemod; who <= kCompensate; ++who)
        for (uint64_t bits = 0; bits < 512; ++bits) {
            const uint64_t frames = bits & 8 ? 0 : (bits & 16 ? kRaggedMaxFrames + 1 : 3);
            const uint64_t a[9] = {bits & 1, bits & 2 ? 6u : 7u, bits & 4 ? 2u : 1u, frames, (bits >> 5) & 1,
                                   bits & 64 ? 3u : 1u, bits & 128 ? 0x100u : LPHY_F_DECODE, bits & 4 ? 2u : 0u,
                                   (bits >> 8) & 1};
            const int rc = rw_args(who, a);
            EXPECT(rc == 0 || rc == -EINVAL || rc == -ERANGE || rc == -ENOTSUP);
            if (!(bits & 1)) EXPECT(rc == -EINVAL);
        }
    std::printf("ragged_walk_check: ok\n");
    return 0;
}
#endif
