// lphy_resample_plan.h — everything of the channeliser (lphy_hip_channelize,
// kernel in lphy_chan.h) and of its mirror the synthesiser
// (lphy_hip_synthesize, kernel in lphy_synth.h) that is a function of plain
// values: what the two share (the limits, the tile, the channel grouping and
// the head of the argument check), then each one's output count, tile
// geometry (which samples a workgroup stages, and where in its LDS), LDS-path
// rule and argument check, and for the channeliser on integer captures
// (lphy_hip_channelize_raw) the sample sizes, the two rows it adds to the check
// and the split of a span into 16-byte loads.  Plain C++ with LPHY_HD in front
// of what the kernels call too, no HIP: the device forms, the host forms and
// the CPU tests (tests/cpp/channelize_check.cpp, channelize_raw_check.cpp,
// synthesize_check.cpp) share it.
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdint>

#include "../../include/lphy_hip.h"
#include "lphy_hd.h"

namespace lphy {

// ---- shared ------------------------------------------------------------------
constexpr unsigned kResTile = 256;  // outputs (of every channel) per workgroup, one per thread
constexpr unsigned kChanTile = kResTile, kSynthTile = kResTile;
constexpr uint32_t kResMaxChannels = 64, kResMaxTaps = 4096, kResMaxStep = 65536, kResMaxRot = 65536;  // step: decim, interp
constexpr uint64_t kResMaxOutputs = uint64_t(1) << 32;  // exclusive
constexpr uint64_t kResMaxSamples = uint64_t(1) << 48;  // sample counts, channels * stride, first + outputs: inclusive
constexpr unsigned kResGroupMax = 8;                    // channels a lane accumulates at a time
constexpr uint64_t kResLdsBytes = 64 * 1024;            // the LDS paths' staging, at most

LPHY_HD uint64_t res_tiles(uint64_t outputs) { return (outputs + kResTile - 1) / kResTile; }

// channels a lane accumulates at a time: the least of 1, 2, 4, 8 that holds
// them all, else 8 (a last group past `channels` repeats the last channel and
// stores or adds nothing for it)
LPHY_HD unsigned res_group(uint32_t channels) {
    unsigned g = 1;
    while (g < kResGroupMax && g < channels) g *= 2;
    return g;
}

inline bool res_aligned(const void* a, const void* b, const void* c, const void* d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 7) == 0;
}

// The rows chan_args and synth_args begin with, in the header's order.  ctx,
// tables (both): the pointer is there; `pointers`: the plan's own rule for in
// and out, asked once the plan is known to be there; aligned: none of the four
// pointers that is there is off an 8-byte boundary; `step`: decim or interp.
template <class Plan, class Pointers>
inline int res_args(bool ctx, const Plan* p, bool tables, Pointers pointers, bool aligned, uint32_t Plan::*step) {
    if (!ctx || !p || !tables) return -EINVAL;
    if (!pointers(*p)) return -EINVAL;
    if (!aligned) return -EINVAL;
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return -EINVAL;
    if (p->channels == 0 || p->taps == 0 || p->*step == 0 || p->rot_period == 0) return -EINVAL;
    if (p->channels > kResMaxChannels) return -ERANGE;
    if (p->taps > kResMaxTaps) return -ERANGE;
    if (p->*step > kResMaxStep) return -ERANGE;
    if (p->rot_period > kResMaxRot) return -ERANGE;
    if (p->outputs >= kResMaxOutputs) return -ERANGE;
    return 0;
}

// ---- the channeliser ---------------------------------------------------------
// lphy_hip_channelize_outputs
LPHY_HD uint64_t chan_outputs(uint64_t in_samples, uint64_t first, uint32_t taps, uint32_t decim) {
    if (taps == 0 || decim == 0 || first > in_samples || in_samples - first < taps) return 0;
    return (in_samples - first - taps) / decim + 1;
}

// The samples tile `tile` reads: `samples` of them from `begin`, for its
// `nout` outputs (kChanTile but for the last tile).  tile < res_tiles(outputs).
struct ChanSpan {
    uint64_t begin, samples;
    unsigned nout;
};
LPHY_HD ChanSpan chan_tile_span(uint64_t first, uint32_t decim, uint32_t taps, uint64_t outputs, uint64_t tile) {
    const uint64_t m0 = tile * kChanTile, left = outputs - m0;
    const unsigned nout = left < kChanTile ? (unsigned)left : kChanTile;
    return ChanSpan{first + m0 * decim, (uint64_t)(nout - 1) * decim + taps, nout};
}

// Where sample i of a tile's span lies in the workgroup's LDS, in 8-byte
// slots: one slot of padding after every 32 samples.  Lane l reads sample
// l * D + k, so at D = 8, 16 or 32 an unpadded image puts the 32 lanes of an
// 8-byte read on 4, 2 or 1 of the 32 slot columns; with the padding they take
// at least 31 different ones.
LPHY_HD uint32_t chan_lds_slot(uint32_t i) { return i + (i >> 5); }

// slots of a full tile's span (64-bit: D * kChanTile alone reaches 2^24)
LPHY_HD uint64_t chan_lds_slots(uint32_t decim, uint32_t taps) {
    const uint64_t last = (uint64_t)(kChanTile - 1) * decim + taps - 1;
    return last + (last >> 5) + 1;
}

// The LDS path takes a plan iff a full tile's padded span fits kResLdsBytes;
// every other plan reads its samples from global memory.
LPHY_HD bool chan_lds_path(uint32_t decim, uint32_t taps) { return chan_lds_slots(decim, taps) * 8 <= kResLdsBytes; }

// lphy_hip_channelize's argument check, in the header's order.  in, out: the
// pointer is there; the rest as res_args.
inline int chan_args(bool ctx, const lphy_chan_plan* p, bool tables, bool in, bool out, bool aligned) {
    const auto pointers = [=](const lphy_chan_plan& q) { return q.outputs == 0 || (in && out); };
    if (int rc = res_args(ctx, p, tables, pointers, aligned, &lphy_chan_plan::decim)) return rc;
    if (p->out_stride < p->outputs) return -ERANGE;
    if (p->in_samples > kResMaxSamples) return -ERANGE;
    // first + (outputs - 1) * decim + taps <= in_samples; the product is below 2^48 here
    if (p->outputs > 0 &&
        (p->first > p->in_samples || (p->outputs - 1) * p->decim + p->taps > p->in_samples - p->first))
        return -ERANGE;
    if (p->out_stride > kResMaxSamples / p->channels) return -ERANGE;
    return 0;
}

// ---- the channeliser on integer captures (lphy_hip_channelize_raw) ------------
// lphy_hip_sample_bytes: one I/Q pair of `format`, 0 for no format
LPHY_HD size_t chan_sample_bytes(int format) {
    switch (format) {
        case LPHY_FMT_CF32: return 8;
        case LPHY_FMT_SC16: return 4;
        case LPHY_FMT_SC8:
        case LPHY_FMT_CU8: return 2;
        default: return 0;
    }
}

// The format's row and the alignment row of lphy_hip_channelize_raw, which
// stand together directly behind the null-pointer rows and both give -EINVAL:
// `format` is one of the four, `in` lies on a multiple of its sample's bytes
// and the other three on 8.  chan_args takes the answer as its `aligned`; with
// LPHY_FMT_CF32 it is res_aligned's.
inline bool chan_raw_aligned(const void* in, int format, const void* taps, const void* rot, const void* out) {
    const size_t b = chan_sample_bytes(format);
    return b != 0 && ((uintptr_t)in & (b - 1)) == 0 && res_aligned(nullptr, taps, rot, out);
}

// How a workgroup stages the `n` samples of `bytes` each (4 or 2) that begin at
// address `addr` (a multiple of `bytes`) with 16-byte loads: `head` single
// samples up to the first 16-byte boundary, `vectors` loads of 16 / bytes
// samples each, `tail` single samples.  Unlike the float path's head of at most
// one sample, which a span of n >= 1 always holds, this head can be longer
// than the span: then it is the whole span.  Sample i of the span is head
// sample i, sample i - head - (16 / bytes) * vectors of the tail, or in vector
// (i - head) / (16 / bytes).
struct ChanStage {
    uint32_t head, vectors, tail;
};
LPHY_HD ChanStage chan_stage_split(uintptr_t addr, uint32_t n, uint32_t bytes) {
    const uint32_t per = 16 / bytes;
    const uint32_t front = (uint32_t)((16 - (addr & 15)) & 15) / bytes;
    const uint32_t head = n < front ? n : front;
    return ChanStage{head, (n - head) / per, (n - head) % per};
}

// ---- the synthesiser ---------------------------------------------------------
// lphy_hip_synthesize_outputs: the outputs up to the last one an input sample
// reaches, (in_samples - 1) * U + T - first.  Past the call's limits the
// product saturates at 2^64 - 1 instead of wrapping.
LPHY_HD uint64_t synth_outputs(uint64_t in_samples, uint64_t first, uint32_t taps, uint32_t interp) {
    if (taps == 0 || interp == 0 || in_samples == 0) return 0;
    const uint64_t top = ~uint64_t(0) - taps;
    const uint64_t end = in_samples - 1 > top / interp ? ~uint64_t(0) : (in_samples - 1) * interp + taps;
    return end > first ? end - first : 0;
}

// taps a lane can meet in one chain, ceil(T / U): i = 0 .. synth_chain - 1
LPHY_HD uint32_t synth_chain(uint32_t taps, uint32_t interp) { return (taps - 1) / interp + 1; }

// The narrow samples tile `tile` stages per channel: `samples` consecutive ones
// from index `begin`, which is signed (the first tiles reach in front of the
// stream) and may end past in_samples; what lies outside 0 .. in_samples-1 is
// staged as (+0, +0).  Output n of the tile, w = first + tile * kSynthTile + n,
// reads j = w / U - i for i < synth_chain, that is slot j - begin.  `q0` and
// `p0` are w / U and w % U of the tile's first output, so that a lane needs
// 32-bit arithmetic only: with t = p0 + n, its q is q0 + t / U and its p is
// t % U.  tile < res_tiles(outputs).
struct SynthSpan {
    int64_t begin;
    uint64_t q0;
    uint32_t p0, samples;
    unsigned nout;
};
LPHY_HD SynthSpan synth_tile_span(uint64_t first, uint32_t interp, uint32_t taps, uint64_t outputs, uint64_t tile) {
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
LPHY_HD SynthStage synth_stage(const SynthSpan& sp) {
    if (sp.begin >= 0) return SynthStage{(uint64_t)sp.begin, 0u};
    const uint64_t front = (uint64_t)(-sp.begin);
    return SynthStage{0, front < sp.samples ? (uint32_t)front : sp.samples};
}
LPHY_HD bool synth_slot_sample(const SynthStage& st, uint32_t s, uint64_t in_samples, uint64_t* j) {
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
LPHY_HD uint32_t synth_lds_slots(uint32_t interp, uint32_t taps) {
    return kSynthTile / interp + synth_chain(taps, interp) + 1;
}

LPHY_HD uint64_t synth_lds_bytes(uint32_t channels, uint32_t interp, uint32_t taps) {
    return (uint64_t)res_group(channels) * synth_lds_slots(interp, taps) * 8;
}

// The LDS path takes a plan iff the image of one channel group fits
// kResLdsBytes; every other plan (long filters at a small U with many
// channels) reads and rotates its samples from global memory.
LPHY_HD bool synth_lds_path(uint32_t channels, uint32_t interp, uint32_t taps) {
    return synth_lds_bytes(channels, interp, taps) <= kResLdsBytes;
}

// lphy_hip_synthesize's argument check, in the header's order.  in, out: the
// pointer is there; the rest as res_args.
inline int synth_args(bool ctx, const lphy_synth_plan* p, bool tables, bool in, bool out, bool aligned) {
    const auto pointers = [=](const lphy_synth_plan& q) { return q.outputs == 0 || (out && (in || q.in_samples == 0)); };
    if (int rc = res_args(ctx, p, tables, pointers, aligned, &lphy_synth_plan::interp)) return rc;
    if (p->in_stride < p->in_samples) return -ERANGE;
    if (p->in_samples > kResMaxSamples) return -ERANGE;
    if (p->in_stride > kResMaxSamples / p->channels) return -ERANGE;
    if (p->first > kResMaxSamples || p->outputs > kResMaxSamples - p->first) return -ERANGE;
    return 0;
}

}  // namespace lphy
