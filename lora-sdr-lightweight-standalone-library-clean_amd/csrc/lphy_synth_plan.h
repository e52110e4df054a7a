// lphy_synth_plan.h — everything of the synthesiser (lphy_hip_synthesize,
// kernel in lphy_synth.h) that is a function of plain values: the output
// count, the tile geometry (which narrow samples of a channel a workgroup
// stages, and where in its LDS), which plans take the LDS path, the channel
// grouping, and the argument check.  Plain C++ with LPHY_CH_HD in front of what
// the kernel calls too, no HIP: the device form, the host form and a CPU test
// (tests/cpp/synthesize_check.cpp) share it.
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdint>

#include "../../include/lphy_hip.h"

#ifndef LPHY_CH_HD
#if defined(__HIPCC__)
#define LPHY_CH_HD __host__ __device__ __forceinline__
#else
#define LPHY_CH_HD inline
#endif
#endif

namespace lphy {

constexpr unsigned kSynthTile = 256;  // wideband outputs per workgroup, one per thread
constexpr uint32_t kSynthMaxChannels = 64, kSynthMaxTaps = 4096, kSynthMaxInterp = 65536, kSynthMaxRot = 65536;
constexpr uint64_t kSynthMaxOutputs = uint64_t(1) << 32;  // exclusive
constexpr uint64_t kSynthMaxSamples = uint64_t(1) << 48;  // in_samples, channels * in_stride, first + outputs: inclusive
constexpr unsigned kSynthGroupMax = 8;                    // channels a lane accumulates at a time
constexpr uint64_t kSynthLdsBytes = 64 * 1024;            // the LDS path's staging, at most

// lphy_hip_synthesize_outputs: the outputs up to the last one an input sample
// reaches, (in_samples - 1) * U + T - first.  Past the call's limits the
// product saturates at 2^64 - 1 instead of wrapping.
LPHY_CH_HD uint64_t synth_outputs(uint64_t in_samples, uint64_t first, uint32_t taps, uint32_t interp) {
    if (taps == 0 || interp == 0 || in_samples == 0) return 0;
    const uint64_t top = ~uint64_t(0) - taps;
    const uint64_t end = in_samples - 1 > top / interp ? ~uint64_t(0) : (in_samples - 1) * interp + taps;
    return end > first ? end - first : 0;
}

LPHY_CH_HD uint64_t synth_tiles(uint64_t outputs) { return (outputs + kSynthTile - 1) / kSynthTile; }

// taps a lane can meet in one chain, ceil(T / U): i = 0 .. synth_chain - 1
LPHY_CH_HD uint32_t synth_chain(uint32_t taps, uint32_t interp) { return (taps - 1) / interp + 1; }

// The narrow samples tile `tile` stages per channel: `samples` consecutive ones
// from index `begin`, which is signed (the first tiles reach in front of the
// stream) and may end past in_samples; what lies outside 0 .. in_samples-1 is
// staged as (+0, +0).  Output n of the tile, w = first + tile * kSynthTile + n,
// reads j = w / U - i for i < synth_chain, that is slot j - begin.  `q0` and
// `p0` are w / U and w % U of the tile's first output, so that a lane needs
// 32-bit arithmetic only: with t = p0 + n, its q is q0 + t / U and its p is
// t % U.  tile < synth_tiles(outputs).
struct SynthSpan {
    int64_t begin;
    uint64_t q0;
    uint32_t p0, samples;
    unsigned nout;
};
LPHY_CH_HD SynthSpan synth_tile_span(uint64_t first, uint32_t interp, uint32_t taps, uint64_t outputs, uint64_t tile) {
    const uint64_t n0 = tile * kSynthTile, left = outputs - n0;
    const unsigned nout = left < kSynthTile ? (unsigned)left : kSynthTile;
    const uint64_t w0 = first + n0, q0 = w0 / interp;
    const uint32_t p0 = (uint32_t)(w0 % interp);
    const uint32_t back = synth_chain(taps, interp) - 1;  // the oldest sample of a chain lies this far behind q
    return SynthSpan{(int64_t)q0 - (int64_t)back, q0, p0, (p0 + nout - 1) / interp + 1 + back, nout};
}

// Which slots of a span hold a sample of the stream: slot s does iff zeros <=
// s and j0 + (s - zeros) < in_samples, and then it is narrow sample j0 + (s -
// zeros); every other slot is staged as (+0, +0).  j0 = max(begin, 0) is the
// first staged sample that can exist and `zeros` its slot (all of the span
// when it ends in front of the stream), so the kernel needs one 64-bit
// remainder for j0's rotation index and 32-bit arithmetic from there.
struct SynthStage {
    uint64_t j0;
    uint32_t zeros;
};
LPHY_CH_HD SynthStage synth_stage(const SynthSpan& sp) {
    if (sp.begin >= 0) return SynthStage{(uint64_t)sp.begin, 0u};
    const uint64_t front = (uint64_t)(-sp.begin);
    return SynthStage{0, front < sp.samples ? (uint32_t)front : sp.samples};
}
LPHY_CH_HD bool synth_slot_sample(const SynthStage& st, uint32_t s, uint64_t in_samples, uint64_t* j) {
    *j = st.j0 + (s - st.zeros);  // read only where s >= zeros
    return s >= st.zeros && *j < in_samples;
}

// slots of one channel in a workgroup's LDS image, 8 bytes each: the most
// synth_tile_span().samples can be, kSynthTile / U + ceil(T / U) + 1.  The image
// is channel-major, slot = channel_in_group * synth_lds_slots + (j - begin),
// and is not padded: the lanes of one read take slots that fall by 0 or 1 from
// lane to lane (q grows by at most 1 from an output to the next), so the
// distinct addresses of a wave are consecutive 8-byte words, which lie on
// different banks; lanes with the same address are served by a broadcast.
LPHY_CH_HD uint32_t synth_lds_slots(uint32_t interp, uint32_t taps) {
    return kSynthTile / interp + synth_chain(taps, interp) + 1;
}

// channels a lane accumulates at a time: the least of 1, 2, 4, 8 that holds
// them all, else 8 (a last group past `channels` stages the last channel again
// and adds nothing for it)
LPHY_CH_HD unsigned synth_group(uint32_t channels) {
    unsigned g = 1;
    while (g < kSynthGroupMax && g < channels) g *= 2;
    return g;
}

LPHY_CH_HD uint64_t synth_lds_bytes(uint32_t channels, uint32_t interp, uint32_t taps) {
    return (uint64_t)synth_group(channels) * synth_lds_slots(interp, taps) * 8;
}

// The LDS path takes a plan iff the image of one channel group fits
// kSynthLdsBytes; every other plan (long filters at a small U with many
// channels) reads and rotates its samples from global memory.
LPHY_CH_HD bool synth_lds_path(uint32_t channels, uint32_t interp, uint32_t taps) {
    return synth_lds_bytes(channels, interp, taps) <= kSynthLdsBytes;
}

// lphy_hip_synthesize's argument check, in the header's order.  ctx, tables
// (both), in, out: the pointer is there; aligned: none of the four that is
// there is off an 8-byte boundary.
inline int synth_args(bool ctx, const lphy_synth_plan* p, bool tables, bool in, bool out, bool aligned) {
    if (!ctx || !p || !tables) return -EINVAL;
    if (p->outputs > 0 && !out) return -EINVAL;
    if (p->outputs > 0 && p->in_samples > 0 && !in) return -EINVAL;
    if (!aligned) return -EINVAL;
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return -EINVAL;
    if (p->channels == 0 || p->taps == 0 || p->interp == 0 || p->rot_period == 0) return -EINVAL;
    if (p->channels > kSynthMaxChannels) return -ERANGE;
    if (p->taps > kSynthMaxTaps) return -ERANGE;
    if (p->interp > kSynthMaxInterp) return -ERANGE;
    if (p->rot_period > kSynthMaxRot) return -ERANGE;
    if (p->outputs >= kSynthMaxOutputs) return -ERANGE;
    if (p->in_stride < p->in_samples) return -ERANGE;
    if (p->in_samples > kSynthMaxSamples) return -ERANGE;
    if (p->in_stride > kSynthMaxSamples / p->channels) return -ERANGE;
    if (p->first > kSynthMaxSamples || p->outputs > kSynthMaxSamples - p->first) return -ERANGE;
    return 0;
}

inline bool synth_aligned(const void* a, const void* b, const void* c, const void* d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 7) == 0;
}

}  // namespace lphy
