// lphy_chan_plan.h — everything of the channeliser (lphy_hip_channelize,
// kernel in lphy_chan.h) that is a function of plain values: the output count,
// the tile geometry (which samples a workgroup stages, and where in its LDS),
// which plans take the LDS path, and the argument check.  Plain C++ with
// LPHY_CH_HD in front of what the kernel calls too, no HIP: the device form,
// the host form and a CPU test (tests/cpp/channelize_check.cpp) share it.
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdint>

#include "../../include/lphy_hip.h"

#if defined(__HIPCC__)
#define LPHY_CH_HD __host__ __device__ __forceinline__
#else
#define LPHY_CH_HD inline
#endif

namespace lphy {

constexpr unsigned kChanTile = 256;  // outputs of every channel per workgroup, one per thread
constexpr uint32_t kChanMaxChannels = 64, kChanMaxTaps = 4096, kChanMaxDecim = 65536, kChanMaxRot = 65536;
constexpr uint64_t kChanMaxOutputs = uint64_t(1) << 32;  // exclusive
constexpr uint64_t kChanMaxSamples = uint64_t(1) << 48;  // in_samples and channels * out_stride, inclusive
constexpr unsigned kChanGroupMax = 8;                    // channels a lane accumulates at a time
constexpr uint64_t kChanLdsBytes = 64 * 1024;            // the LDS path's staging, at most

// lphy_hip_channelize_outputs
LPHY_CH_HD uint64_t chan_outputs(uint64_t in_samples, uint64_t first, uint32_t taps, uint32_t decim) {
    if (taps == 0 || decim == 0 || first > in_samples || in_samples - first < taps) return 0;
    return (in_samples - first - taps) / decim + 1;
}

LPHY_CH_HD uint64_t chan_tiles(uint64_t outputs) { return (outputs + kChanTile - 1) / kChanTile; }

// The samples tile `tile` reads: `samples` of them from `begin`, for its
// `nout` outputs (kChanTile but for the last tile).  tile < chan_tiles(outputs).
struct ChanSpan {
    uint64_t begin, samples;
    unsigned nout;
};
LPHY_CH_HD ChanSpan chan_tile_span(uint64_t first, uint32_t decim, uint32_t taps, uint64_t outputs, uint64_t tile) {
    const uint64_t m0 = tile * kChanTile, left = outputs - m0;
    const unsigned nout = left < kChanTile ? (unsigned)left : kChanTile;
    return ChanSpan{first + m0 * decim, (uint64_t)(nout - 1) * decim + taps, nout};
}

// Where sample i of a tile's span lies in the workgroup's LDS, in 8-byte
// slots: one slot of padding after every 32 samples.  Lane l reads sample
// l * D + k, so at D = 8, 16 or 32 an unpadded image puts the 32 lanes of an
// 8-byte read on 4, 2 or 1 of the 32 slot columns; with the padding they take
// at least 31 different ones.
LPHY_CH_HD uint32_t chan_lds_slot(uint32_t i) { return i + (i >> 5); }

// slots of a full tile's span (64-bit: D * kChanTile alone reaches 2^24)
LPHY_CH_HD uint64_t chan_lds_slots(uint32_t decim, uint32_t taps) {
    const uint64_t last = (uint64_t)(kChanTile - 1) * decim + taps - 1;
    return last + (last >> 5) + 1;
}

// The LDS path takes a plan iff a full tile's padded span fits kChanLdsBytes;
// every other plan reads its samples from global memory.
LPHY_CH_HD bool chan_lds_path(uint32_t decim, uint32_t taps) { return chan_lds_slots(decim, taps) * 8 <= kChanLdsBytes; }

// channels a lane accumulates at a time: the least of 1, 2, 4, 8 that holds
// them all, else 8 (a last group past `channels` repeats the last channel and
// stores nothing for it)
LPHY_CH_HD unsigned chan_group(uint32_t channels) {
    unsigned g = 1;
    while (g < kChanGroupMax && g < channels) g *= 2;
    return g;
}

// lphy_hip_channelize's argument check, in the header's order.  ctx, tables
// (both), in, out: the pointer is there; aligned: none of the four that is
// there is off an 8-byte boundary.
inline int chan_args(bool ctx, const lphy_chan_plan* p, bool tables, bool in, bool out, bool aligned) {
    if (!ctx || !p || !tables) return -EINVAL;
    if (p->outputs > 0 && !(in && out)) return -EINVAL;
    if (!aligned) return -EINVAL;
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return -EINVAL;
    if (p->channels == 0 || p->taps == 0 || p->decim == 0 || p->rot_period == 0) return -EINVAL;
    if (p->channels > kChanMaxChannels) return -ERANGE;
    if (p->taps > kChanMaxTaps) return -ERANGE;
    if (p->decim > kChanMaxDecim) return -ERANGE;
    if (p->rot_period > kChanMaxRot) return -ERANGE;
    if (p->outputs >= kChanMaxOutputs) return -ERANGE;
    if (p->out_stride < p->outputs) return -ERANGE;
    if (p->in_samples > kChanMaxSamples) return -ERANGE;
    // first + (outputs - 1) * decim + taps <= in_samples; the product is below 2^48 here
    if (p->outputs > 0 &&
        (p->first > p->in_samples || (p->outputs - 1) * p->decim + p->taps > p->in_samples - p->first))
        return -ERANGE;
    if (p->out_stride > kChanMaxSamples / p->channels) return -ERANGE;
    return 0;
}

inline bool chan_aligned(const void* a, const void* b, const void* c, const void* d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 7) == 0;
}

}  // namespace lphy
