// lphy_codes_plan.h — what the whitening kernel (k_whiten, lphy_codes.hip)
// computes that is a function of plain values: the recurrences of the three
// generators, their periods, and the reduction that takes (kind, bit_ofs, j)
// to a table position or to a start state and a number of steps below one
// period.  Plain C++ with LPHY_HD in front of what the kernel calls too, no
// HIP: the kernel, the entry point and a CPU test
// (tests/cpp/codes_plan_check.cpp, which derives the periods again by
// stepping the recurrences until the state returns) share it.
#pragma once
#include <cstdint>

#include "../../include/lphy_hip.h"
#include "lphy_hd.h"

// The stored 510-bit sequence of Sx1272ComputeWhitening and the sequence
// positions its codeword bits tap (LoRaCodes.hpp:147-167), as initialisers:
// the kernel keeps them in constant memory, the CPU test in a plain array.
#define LPHY_WHITEN_SEQ_INIT                                                                           \
    {0x0102291EA751AAFFull, 0xD24B050A8D643A17ull, 0x5B279B671120B8F4ull, 0x032B37B9F6FB55A2ull,       \
     0x994E0F87E95E2D16ull, 0x7CBCFC7631984C26ull, 0x281C8E4F0DAEF7F9ull, 0x1741886EB7733B15ull}
#define LPHY_WHITEN_TAPS_INIT {6, 4, 2, 0, -112, -114, -302, -34}
#define LPHY_WHITEN_TAPS_CR1_INIT {6, 4, 2, 0, -360}

namespace lphy {

// Positions after which each generator's output repeats.
constexpr unsigned kWhitenSx1232Period = 511;  // steps of the 9-bit LFSR from 0x1FF
constexpr unsigned kWhitenSeqLen = 510;        // the stored SX1272 sequence, by definition
constexpr unsigned kWhitenLfsrPeriod = 255;    // steps of each 64-bit state; two interleaved: 510 positions
constexpr int kWhitenTapMin = -360;            // the most negative tap: tap + kWhitenSeqLen > 0

constexpr unsigned kWhitenSx1232Seed = 0x1FF;

// SX1232RadioComputeWhitening (LoRaCodes.hpp:111-137): x^9 + x^5 + 1, one bit
LPHY_HD unsigned whiten_sx1232_step(unsigned s) { return (s >> 1) | (((s ^ (s >> 5)) & 1u) << 8); }

// Sx1272ComputeWhiteningLfsr (:176-189): one codeword, poly 0x1D on every bit lane
LPHY_HD unsigned long long whiten_lfsr64_step(unsigned long long r) {
    return (r >> 8) | (((r >> 32) ^ (r >> 24) ^ (r >> 16) ^ r) << 56);
}

// the state that even (odd = 0) and odd codeword positions start from
LPHY_HD unsigned long long whiten_lfsr_seed(unsigned rdd, unsigned odd) {
    return rdd == 1 ? (odd ? 0xF8ECFEEFEFEFEFEFull : 0x05121100F8ECFEEFull)
                    : (odd ? 0xE85C2EFFFFFFFFFFull : 0x6572D100E85C2EFFull);
}

// What the entry point hands the kernel for a bit_ofs >= 0: the two SX1272
// kinds repeat every kWhitenSeqLen positions, SX1232 ignores it.
LPHY_HD unsigned whiten_reduce_ofs(int kind, int bit_ofs) {
    return kind == LPHY_WHITEN_SX1232 ? 0u : (unsigned)bit_ofs % kWhitenSeqLen;
}

// Below, ofs = whiten_reduce_ofs(...) < kWhitenSeqLen and j < 65536 is the
// byte's index in its row, so ofs + j and 8 * j are far from 32 bits.

// SX1232: steps from kWhitenSx1232Seed to the state whose low byte masks byte j
LPHY_HD unsigned whiten_sx1232_steps(unsigned j) { return (8u * j) % kWhitenSx1232Period; }

// SX1272: position in the stored sequence of a codeword bit with tap `tap`
LPHY_HD unsigned whiten_seq_pos(int tap, unsigned ofs, unsigned j) {
    return ((unsigned)(tap + (int)kWhitenSeqLen) + ofs + j) % kWhitenSeqLen;
}

// SX1272 LFSR: codeword position p = ofs + j takes state p & 1 after p >> 1
// steps, which repeat every kWhitenLfsrPeriod
struct WhitenLfsrPlan {
    unsigned odd, steps;
};
LPHY_HD WhitenLfsrPlan whiten_lfsr_plan(unsigned ofs, unsigned j) {
    const unsigned p = ofs + j;
    return WhitenLfsrPlan{p & 1u, (p >> 1) % kWhitenLfsrPeriod};
}

// The byte XORed into byte j of a row.  seq: the 8 words of
// LPHY_WHITEN_SEQ_INIT; taps: LPHY_WHITEN_TAPS_CR1_INIT for rdd 1,
// LPHY_WHITEN_TAPS_INIT otherwise (both read by LPHY_WHITEN_SX1272 only).
LPHY_HD unsigned whiten_mask(int kind, unsigned ofs, unsigned j, unsigned rdd, const unsigned long long* seq,
                                const int* taps) {
    if (kind == LPHY_WHITEN_SX1232) {
        unsigned s = kWhitenSx1232Seed;
        for (unsigned k = whiten_sx1232_steps(j); k; --k) s = whiten_sx1232_step(s);
        return s & 0xFFu;
    }
    if (kind == LPHY_WHITEN_SX1272) {
        unsigned mask = 0;
        for (unsigned i = 0; i < 4 + rdd; ++i) {
            const unsigned q = whiten_seq_pos(taps[i], ofs, j);
            mask |= (unsigned)((seq[q >> 6] >> (q & 63)) & 1ull) << i;
        }
        return mask & 0xFFu;
    }
    const WhitenLfsrPlan pl = whiten_lfsr_plan(ofs, j);
    unsigned long long r = whiten_lfsr_seed(rdd, pl.odd);
    for (unsigned k = pl.steps; k; --k) r = whiten_lfsr64_step(r);
    return (unsigned)(r & (0xffu >> (4 - rdd)));
}

}  // namespace lphy
