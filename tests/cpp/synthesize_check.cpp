// Stand-alone program over the host-compilable part of the synthesiser
// (csrc/lphy_resample_plan.h), for a run under the host sanitizers
// (tests/test_synthesize_cpu.py):
//   - every row of synth_args in the documented order, pairs of bad arguments
//     (the earlier row wins), and the overflow-prone rows at 2^32, 2^48, 2^64;
//   - synth_outputs against its formula and a brute-force reach;
//   - the tile geometry: for a grid of (U, T, first, outputs, in_samples), for
//     every output of every tile, every j the definition reads lies inside the
//     staged span, at a slot below synth_lds_slots, the lane's 32-bit q and p
//     are the definition's 64-bit ones, and the slot is staged (synth_stage,
//     synth_slot_sample) as sample j when 0 <= j < in_samples and as zero
//     otherwise;
//   - res_group, synth_lds_bytes and synth_lds_path.
// Prints the tile, sizeof(lphy_synth_plan) and its members' offsets.
#include <cstdio>
#include <initializer_list>

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

static lphy_synth_plan good() {
    lphy_synth_plan p{};
    p.first = 3;
    p.in_samples = 100;
    p.in_stride = 103;
    p.interp = 4;
    p.taps = 5;
    p.outputs = synth_outputs(p.in_samples, p.first, p.taps, p.interp);
    p.rot_first = (uint64_t(1) << 40) + 3;
    p.channels = 3;
    p.rot_period = 7;
    return p;
}

static int args(const lphy_synth_plan& p) { return synth_args(true, &p, true, true, true, true); }

static int args_check() {
    const uint64_t k32 = uint64_t(1) << 32, k48 = uint64_t(1) << 48;
    lphy_synth_plan p = good();
    EXPECT(p.outputs == 99 * 4 + 5 - 3 && args(p) == 0);
    // the -EINVAL rows, in order
    EXPECT(synth_args(false, &p, true, true, true, true) == -EINVAL);
    EXPECT(synth_args(true, nullptr, true, true, true, true) == -EINVAL);
    EXPECT(synth_args(true, &p, false, true, true, true) == -EINVAL);
    EXPECT(synth_args(true, &p, true, true, false, true) == -EINVAL);  // out
    EXPECT(synth_args(true, &p, true, false, true, true) == -EINVAL);  // in
    EXPECT(synth_args(true, &p, true, true, true, false) == -EINVAL);  // alignment
    for (int i = 0; i < 2; ++i) {
        p = good(), p.reserved[i] = 1;
        EXPECT(args(p) == -EINVAL);
    }
    p = good(), p.channels = 0;
    EXPECT(args(p) == -EINVAL);
    p = good(), p.taps = 0;
    EXPECT(args(p) == -EINVAL);
    p = good(), p.interp = 0;
    EXPECT(args(p) == -EINVAL);
    p = good(), p.rot_period = 0;
    EXPECT(args(p) == -EINVAL);
    // the earlier row wins: a zero field and a limit, a bad pointer and a zero field
    p = good(), p.taps = 0, p.channels = 65;
    EXPECT(args(p) == -EINVAL);
    p = good(), p.channels = 65, p.outputs = k32;
    EXPECT(synth_args(true, &p, true, true, false, true) == -EINVAL);
    // no input sample: d_in is not asked for, d_out is; no output: neither
    p = good(), p.in_samples = 0;
    EXPECT(synth_args(true, &p, true, false, true, true) == 0);
    EXPECT(synth_args(true, &p, true, false, false, true) == -EINVAL);
    p = good(), p.outputs = 0;
    EXPECT(synth_args(true, &p, true, false, false, true) == 0);
    EXPECT(synth_args(true, &p, false, false, false, true) == -EINVAL);
    p.channels = 65;
    EXPECT(synth_args(true, &p, true, false, false, true) == -ERANGE);
    // res_aligned: any of the four off an 8-byte boundary, null pointers pass
    alignas(16) static char buf[32];
    EXPECT(res_aligned(buf, buf + 8, buf + 16, nullptr) && res_aligned(nullptr, buf, buf, buf + 24));
    EXPECT(!res_aligned(buf + 4, buf, buf, buf) && !res_aligned(buf, buf + 4, buf, buf));
    EXPECT(!res_aligned(buf, buf, buf + 2, buf) && !res_aligned(buf, buf, buf, buf + 1));

    // the -ERANGE rows, each at its edge, in order
    p = good(), p.channels = 64;
    EXPECT(args(p) == 0);
    p.channels = 65;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.taps = 4096;
    EXPECT(args(p) == 0);
    p.taps = 4097;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.interp = 65536;
    EXPECT(args(p) == 0);
    p.interp = 65537;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.rot_period = 65536;
    EXPECT(args(p) == 0);
    p.rot_period = 65537;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.outputs = k32 - 1;  // a tail past what the input reaches is legal
    EXPECT(args(p) == 0);
    p.outputs = k32;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.in_stride = p.in_samples;
    EXPECT(args(p) == 0);
    p.in_stride = p.in_samples - 1;
    EXPECT(args(p) == -ERANGE);
    // in_samples <= 2^48 (one channel, or the next row speaks first)
    p = good(), p.channels = 1, p.in_samples = k48, p.in_stride = k48;
    EXPECT(args(p) == 0);
    p.in_samples = k48 + 1, p.in_stride = k48 + 1;
    EXPECT(args(p) == -ERANGE);
    p.in_samples = ~uint64_t(0), p.in_stride = ~uint64_t(0);
    EXPECT(args(p) == -ERANGE);
    // channels * in_stride <= 2^48, without the product
    p = good(), p.channels = 64, p.in_stride = k48 / 64;
    EXPECT(args(p) == 0);
    p.in_stride = k48 / 64 + 1;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.channels = 3, p.in_stride = k48 / 3;
    EXPECT(args(p) == 0);
    p.in_stride = k48 / 3 + 1;
    EXPECT(args(p) == -ERANGE);
    p.in_stride = ~uint64_t(0) / 3 + 2;  // 3 * in_stride wraps to a small number
    EXPECT(args(p) == -ERANGE);
    // first + outputs <= 2^48, without the sum
    p = good(), p.outputs = 1000, p.first = k48 - 1000;
    EXPECT(args(p) == 0);
    p.first = k48 - 999;
    EXPECT(args(p) == -ERANGE);
    p.first = ~uint64_t(0) - 10;  // first + outputs wraps
    EXPECT(args(p) == -ERANGE);
    p = good(), p.outputs = 0, p.first = k48;
    EXPECT(args(p) == 0);
    p.first = k48 + 1;
    EXPECT(args(p) == -ERANGE);
    p = good(), p.first = 0, p.outputs = k32 - 1;
    EXPECT(args(p) == 0);
    // order among the -ERANGE rows: the earlier one is the one that speaks (all return
    // the same code, so this checks only that two bad rows do not cancel)
    p = good(), p.channels = 65, p.in_stride = 0;
    EXPECT(args(p) == -ERANGE);
    return 0;
}

static int outputs_check() {
    EXPECT(synth_outputs(0, 0, 5, 4) == 0 && synth_outputs(10, 0, 0, 4) == 0 && synth_outputs(10, 0, 5, 0) == 0);
    EXPECT(synth_outputs(1, 0, 5, 4) == 5 && synth_outputs(1, 4, 5, 4) == 1 && synth_outputs(1, 5, 5, 4) == 0);
    EXPECT(synth_outputs(1, 6, 5, 4) == 0 && synth_outputs(1, ~uint64_t(0), 5, 4) == 0);
    EXPECT(synth_outputs(100, 3, 5, 4) == 99 * 4 + 5 - 3);
    // the limits' corner does not wrap: (2^48 - 1) * 65536 + 4096 < 2^64
    const uint64_t k48 = uint64_t(1) << 48;
    EXPECT(synth_outputs(k48, 0, 4096, 65536) == (k48 - 1) * 65536 + 4096);
    EXPECT(synth_outputs(k48, 1000, 1, 1) == k48 - 1000);
    // past the limits it saturates
    EXPECT(synth_outputs(~uint64_t(0), 0, 4096, 65536) == ~uint64_t(0));
    EXPECT(synth_outputs(~uint64_t(0), 10, 1, 2) == ~uint64_t(0) - 10);
    // brute force: the last output any input sample reaches, from the definition
    for (uint32_t U : {1u, 2u, 3u, 7u, 16u})
        for (uint32_t T : {1u, 2u, 5u, 16u, 17u, 40u})
            for (uint64_t n_in : {1ull, 2ull, 9ull})
                for (uint64_t first : {0ull, 1ull, 13ull, 200ull}) {
                    uint64_t reach = 0;  // one past the last w with a (j, k) pair in range
                    for (uint64_t w = 0; w < n_in * U + T + 4; ++w)
                        for (uint64_t i = 0; i * U + w % U < T; ++i)
                            if (w / U >= i && w / U - i < n_in) reach = w + 1;
                    EXPECT(synth_outputs(n_in, first, T, U) == (reach > first ? reach - first : 0));
                }
    return 0;
}

static int geometry_check() {
    EXPECT(res_tiles(0) == 0 && res_tiles(1) == 1 && res_tiles(kSynthTile) == 1);
    EXPECT(res_tiles(kSynthTile + 1) == 2 && res_tiles((uint64_t(1) << 32) - 1) == (uint64_t(1) << 32) / kSynthTile);
    EXPECT(synth_chain(1, 1) == 1 && synth_chain(5, 4) == 2 && synth_chain(4, 4) == 1 && synth_chain(3, 300) == 1);
    EXPECT(synth_chain(4096, 1) == 4096 && synth_chain(129, 16) == 9);
    unsigned long long reads = 0;
    for (uint32_t U : {1u, 2u, 3u, 8u, 16u, 255u, 256u, 257u, 300u, 1000u, 65536u})
        for (uint32_t T : {1u, 2u, 5u, 129u, 257u, 700u, 4096u}) {
            const uint32_t S = synth_lds_slots(U, T), chain = synth_chain(T, U);
            EXPECT(S == kSynthTile / U + (T + U - 1) / U + 1);
            for (uint64_t first : {uint64_t(0), uint64_t(1), uint64_t(U - 1), uint64_t(5) * U + 3, uint64_t(7) * U,
                                   (uint64_t(1) << 48) - 1000})
                for (uint64_t outputs : {uint64_t(1), uint64_t(kSynthTile - 1), uint64_t(kSynthTile),
                                         uint64_t(kSynthTile + 1), uint64_t(2 * kSynthTile + 77)}) {
                    for (uint64_t tile = 0; tile < res_tiles(outputs); ++tile) {
                        const SynthSpan sp = synth_tile_span(first, U, T, outputs, tile);
                        const SynthStage stg = synth_stage(sp);
                        EXPECT(stg.zeros <= sp.samples && (stg.zeros == 0 || stg.j0 == 0));
                        // streams that end in front of, inside and behind the span, and none at all
                        const uint64_t q_last = (first + tile * kSynthTile + sp.nout - 1) / U;
                        const uint64_t ins[] = {0, 1, q_last > 3 ? q_last - 3 : 2, q_last + 1, q_last + 1000,
                                                sp.begin > 0 ? (uint64_t)sp.begin : 5, uint64_t(1) << 48};
                        for (uint32_t slot = 0; slot < sp.samples; ++slot)
                            for (uint64_t n_in : ins) {
                                const int64_t j = sp.begin + (int64_t)slot;
                                uint64_t got = 0;
                                const bool have = synth_slot_sample(stg, slot, n_in, &got);
                                EXPECT(have == (j >= 0 && (uint64_t)j < n_in));
                                if (have) EXPECT(got == (uint64_t)j);
                            }
                        EXPECT(sp.nout >= 1 && sp.nout <= kSynthTile);
                        EXPECT(tile * kSynthTile + sp.nout == (tile + 1 == res_tiles(outputs) ? outputs : (tile + 1) * kSynthTile));
                        EXPECT(sp.samples >= 1 && sp.samples <= S);
                        const uint64_t w0 = first + tile * kSynthTile;
                        EXPECT(sp.q0 == w0 / U && sp.p0 == w0 % U);
                        int64_t lo = INT64_MAX, hi = INT64_MIN;
                        for (unsigned n = 0; n < sp.nout; ++n) {
                            const uint64_t w = w0 + n, q = w / U, p = w % U;
                            // the lane's 32-bit arithmetic
                            const uint32_t t = sp.p0 + n, dq = t / U, lp = t % U;
                            EXPECT(sp.q0 + dq == q && lp == p);
                            const uint32_t ni = lp < T ? (T - 1 - lp) / U + 1 : 0;
                            uint32_t count = 0;
                            for (uint64_t i = 0; i * U + p < T; ++i) {
                                ++count;
                                const int64_t j = (int64_t)q - (int64_t)i;
                                const int64_t slot = j - sp.begin;
                                EXPECT(slot >= 0 && slot < (int64_t)sp.samples && slot < (int64_t)S);
                                EXPECT(slot == (int64_t)(chain - 1 + dq - i));  // the kernel's expression
                                lo = j < lo ? j : lo, hi = j > hi ? j : hi;
                                ++reads;
                            }
                            EXPECT(count == ni && ni <= chain);
                        }
                        // the span starts no earlier than one chain behind the tile's first q
                        // and ends at its last q
                        if (lo <= hi) EXPECT(sp.begin <= lo && hi <= sp.begin + (int64_t)sp.samples - 1);
                        EXPECT(sp.begin == (int64_t)sp.q0 - (int64_t)(chain - 1));
                        EXPECT(sp.begin + (int64_t)sp.samples - 1 == (int64_t)((w0 + sp.nout - 1) / U));
                    }
                }
        }
    EXPECT(reads > 1000000);
    // a span in front of the stream: begin < 0, the first -begin slots are zeros,
    // all of them when the span ends before sample 0 cannot happen (its last
    // slot is the tile's last q >= 0), and a stream shorter than the span
    {
        const SynthSpan sp = synth_tile_span(0, 4, 17, 10, 0);  // chain 5: begin = -4
        EXPECT(sp.begin == -4 && sp.samples == (0 + 9) / 4 + 1 + 4);
        const SynthStage stg = synth_stage(sp);
        EXPECT(stg.j0 == 0 && stg.zeros == 4);
        uint64_t j = 99;
        EXPECT(!synth_slot_sample(stg, 3, 10, &j) && synth_slot_sample(stg, 4, 10, &j) && j == 0);
        EXPECT(synth_slot_sample(stg, 6, 3, &j) && j == 2 && !synth_slot_sample(stg, 6, 2, &j));
        EXPECT(!synth_slot_sample(stg, 4, 0, &j));
        // the clamp of synth_stage, on a span made by hand
        const SynthStage far = synth_stage(SynthSpan{-100, 0, 0, 7, 1});
        EXPECT(far.j0 == 0 && far.zeros == 7);
    }
    return 0;
}

static int group_check() {
    EXPECT(res_group(1) == 1 && res_group(2) == 2 && res_group(3) == 4 && res_group(4) == 4);
    EXPECT(res_group(5) == 8 && res_group(8) == 8 && res_group(9) == 8 && res_group(64) == 8);
    EXPECT(synth_lds_bytes(1, 16, 129) == (16 + 9 + 1) * 8 && synth_lds_bytes(9, 16, 129) == 8 * (16 + 9 + 1) * 8);
    // the size rule: one channel always fits, eight channels do up to S = 1024
    EXPECT(synth_lds_path(1, 1, 4096) && synth_lds_bytes(1, 1, 4096) == (256 + 4096 + 1) * 8);
    EXPECT(synth_lds_path(8, 1, 767) && synth_lds_bytes(8, 1, 767) == kResLdsBytes);
    EXPECT(!synth_lds_path(8, 1, 768) && !synth_lds_path(64, 1, 1025) && synth_lds_path(4, 1, 1025));
    EXPECT(synth_lds_path(64, 2, 1025) && !synth_lds_path(2, 1, 4096) && synth_lds_path(64, 16, 4096));
    return 0;
}

// two violations at once, one row per adjacent pair of synth_args's tests and some across the two codes
static const Pair kSynthPairs[] = {
    {V_CTX, V_PLAN, -EINVAL}, {V_PLAN, V_TABLES, -EINVAL}, {V_TABLES, V_OUT, -EINVAL}, {V_OUT, V_IN, -EINVAL},
    {V_IN, V_ALIGN, -EINVAL}, {V_ALIGN, V_RES0, -EINVAL}, {V_RES0, V_RES1, -EINVAL}, {V_RES1, V_CH0, -EINVAL},
    {V_CH0, V_T0, -EINVAL}, {V_T0, V_STEP0, -EINVAL}, {V_STEP0, V_R0, -EINVAL}, {V_R0, V_CHMAX, -EINVAL},
    {V_CHMAX, V_TMAX, -ERANGE}, {V_TMAX, V_STEPMAX, -ERANGE}, {V_STEPMAX, V_RMAX, -ERANGE},
    {V_RMAX, V_OUTMAX, -ERANGE}, {V_OUTMAX, V_STRIDE_SMALL, -ERANGE}, {V_STRIDE_SMALL, V_INMAX, -ERANGE},
    {V_INMAX, V_STRIDE_BIG, -ERANGE}, {V_STRIDE_BIG, V_FIRST, -ERANGE}, {V_CHMAX, V_RES0, -EINVAL},
    {V_INMAX, V_STRIDE_SMALL, -ERANGE}, {V_CHMAX, V_ALIGN, -EINVAL}, {V_OUTMAX, V_RES1, -EINVAL},
    {V_STRIDE_BIG, V_R0, -EINVAL}, {V_INMAX, V_OUT, -EINVAL}, {V_FIRST, V_CTX, -EINVAL}, {V_STEPMAX, V_T0, -EINVAL},
    {V_STRIDE_BIG, V_TABLES, -EINVAL}, {V_RMAX, V_IN, -EINVAL}, {V_FIRST, V_STEP0, -EINVAL}, {V_TMAX, V_CH0, -EINVAL},
    {V_STRIDE_SMALL, V_PLAN, -EINVAL}, {V_OUTMAX, V_IN, -EINVAL},
};

int main() {
    if (args_check() || outputs_check() || geometry_check() || group_check() ||
        pairs_check(kSynthPairs, good(), synth_args, &lphy_synth_plan::interp, &lphy_synth_plan::in_stride))
        return 1;
    static_assert(sizeof(lphy_synth_plan) == 64, "lphy_synth_plan is 64 bytes");
    std::printf("synthesize_check: ok kSynthTile=%u sizeof(lphy_synth_plan)=%zu offsets=%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu\n",
                kSynthTile, sizeof(lphy_synth_plan), offsetof(lphy_synth_plan, first),
                offsetof(lphy_synth_plan, in_samples), offsetof(lphy_synth_plan, in_stride),
                offsetof(lphy_synth_plan, outputs), offsetof(lphy_synth_plan, rot_first),
                offsetof(lphy_synth_plan, channels), offsetof(lphy_synth_plan, taps), offsetof(lphy_synth_plan, interp),
                offsetof(lphy_synth_plan, rot_period), offsetof(lphy_synth_plan, reserved));
    return 0;
}
