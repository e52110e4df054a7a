// lphy_stage_plan.h — where the buffers of one *_host call lie in the
// context's staging (lphy_host.h): an ordered list of slices, the bytes the
// call needs, and the spans the pinned mirror moves in one copy each way.
// Plain host arithmetic, no HIP: the CPU tests compile it alone
// (tests/cpp/stage_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "lphy_ragged_layout.h"

namespace lphy {

// every slice starts on this alignment and occupies at least one unit of it,
// so the slices of a call are distinct and non-null even when empty
constexpr size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

enum StageRole : unsigned {
    kStageIn = 1,       // host -> device before the kernels
    kStageOut = 2,      // device -> host after them
    kStageInOut = 3,
    kStageZero = 4,     // device memory zeroed before the kernels
    kStageZeroOut = 6,
    kStageScratch = 8,  // lent to the kernels, never copied; after every other slice
};

struct StageSlice {
    size_t off = 0, size = 0;
    unsigned role = 0;
};

struct StageSpan {  // [begin, end); begin == end: nothing to move
    size_t begin = 0, end = 0;
    void cover(size_t b, size_t e) {
        if (begin == end) begin = b;
        end = e;
    }
};

struct StagePlan {
    static constexpr int kMaxSlices = 5;
    StageSlice s[kMaxSlices];
    int n = 0;
    size_t end = 0;         // bytes of staging the call needs
    size_t copied_end = 0;  // end of the last slice that is not scratch
    StageSpan up, down;     // the non-empty slices uploaded or zeroed / downloaded

    StagePlan& add(size_t size, unsigned role) {
        s[n++] = StageSlice{end, size, role};
        const size_t off = end;
        end += align_up(std::max<size_t>(1, size));
        if (role == kStageScratch) return *this;
        copied_end = end;
        if (size && (role & (kStageIn | kStageZero))) up.cover(off, end);
        if (size && (role & kStageOut)) down.cover(off, end);
        return *this;
    }
};

constexpr size_t kIqBytes = 2 * sizeof(float);  // one complex sample
constexpr size_t kMetaBytes = sizeof(lphy_frame_meta);

// The plans of the eleven *_host entry points, slices in the order named.

// iq | syms | bytes | meta | spec (the SF 11-12 speculation records); `per`:
// lphy_hip_syms_per_frame
inline StagePlan demod_plan(size_t frames, size_t frame_samples, size_t per) {
    return StagePlan()
        .add(frames * frame_samples * kIqBytes, kStageIn)
        .add(frames * per * sizeof(uint16_t), kStageOut)
        .add(frames * (per / 2), kStageOut)
        .add(frames * kMetaBytes, kStageZeroOut)
        .add(frames * 16, kStageScratch);
}

// iq | desc | syms | bytes | meta; the caller's output slots go in as well
// (slots no frame owns come back as they went)
inline StagePlan ragged_plan(size_t iq_samples, size_t frames, size_t out_syms) {
    return StagePlan()
        .add(iq_samples * kIqBytes, kStageIn)
        .add((frames + 1) * sizeof(lphy_ragged_desc), kStageIn)
        .add(out_syms * sizeof(uint16_t), kStageInOut)
        .add((out_syms + 1) / 2, kStageInOut)
        .add(frames * kMetaBytes, kStageZeroOut);
}

// iq (the samples the windows span) | records
inline StagePlan detect_plan(size_t span, size_t windows) {
    return StagePlan().add(span * kIqBytes, kStageIn).add(windows * sizeof(lphy_detect_rec), kStageOut);
}

// syms | bytes | meta
inline StagePlan decode_plan(size_t count) {
    return StagePlan().add(count * sizeof(uint16_t), kStageIn).add(count / 2, kStageOut).add(kMetaBytes, kStageZeroOut);
}

// iq | meta
inline StagePlan estimate_plan(size_t count) {
    return StagePlan().add(count * kIqBytes, kStageIn).add(kMetaBytes, kStageInOut);
}

// iq | the time shift's buffer
inline StagePlan compensate_plan(size_t count) {
    return StagePlan().add(count * kIqBytes, kStageInOut).add(count * kIqBytes, kStageScratch);
}

// iq | meta
inline StagePlan compensate_batch_plan(size_t frames, size_t frame_samples) {
    return StagePlan().add(frames * frame_samples * kIqBytes, kStageInOut).add(frames * kMetaBytes, kStageIn);
}

// syms | iq | the modulator's scratch (mod_scratch_bytes for one frame of nsyms); step = N * osr
inline StagePlan modulate_plan(size_t step, size_t nsyms, size_t scratch) {
    return StagePlan()
        .add(nsyms * sizeof(uint16_t), kStageIn)
        .add((nsyms + 2) * step * kIqBytes, kStageOut)
        .add(scratch, kStageScratch);
}

// bytes | desc | iq | syms (lphy_hip_tx_ragged_host).  The IQ and the symbols
// are outputs; where the frames leave gaps in them the caller's values go in
// first, so that the gaps come back as they went.  out_syms = 0: no h_syms_out.
inline StagePlan tx_plan(size_t in_bytes, size_t frames, size_t iq_samples, size_t out_syms, bool iq_gaps,
                         bool sym_gaps) {
    return StagePlan()
        .add(in_bytes, kStageIn)
        .add((frames + 1) * sizeof(lphy_ragged_desc), kStageIn)
        .add(iq_samples * kIqBytes, iq_gaps ? kStageInOut : kStageOut)
        .add(out_syms * sizeof(uint16_t), sym_gaps ? kStageInOut : kStageOut);
}

// iq | desc (the frames' records; record [frames] is not read) | meta
// (lphy_hip_estimate_ragged_host).  The caller's records go in, so that a
// frame the call leaves alone comes back as it went.
inline StagePlan estimate_ragged_plan(size_t iq_samples, size_t frames) {
    return StagePlan()
        .add(iq_samples * kIqBytes, kStageIn)
        .add(frames * sizeof(lphy_ragged_desc), kStageIn)
        .add(frames * kMetaBytes, kStageInOut);
}

// iq | desc (frames + 1 records) | records, one per whole symbol
// (lphy_hip_detect_ragged_host).  With a checked table every record has
// exactly one owner, so the records only come back.
inline StagePlan detect_ragged_plan(size_t iq_samples, size_t frames, size_t units) {
    return StagePlan()
        .add(iq_samples * kIqBytes, kStageIn)
        .add((frames + 1) * sizeof(lphy_ragged_desc), kStageIn)
        .add(units * sizeof(lphy_detect_rec), kStageOut);
}

// records | desc (max_frames + 1 records) | info | the search's workspace
// (find_layout's bytes, lphy_find_scan.h) - lphy_hip_find_frames_host.  Not
// among the plans lphy_hip_ctx_reserve sizes for: a capture's windows and the
// table's capacity are not a frame shape, so a call past the reservation grows
// the staging once, like any other.
inline StagePlan find_plan(size_t windows, size_t max_frames, size_t work_bytes) {
    return StagePlan()
        .add(windows * sizeof(lphy_detect_rec), kStageIn)
        .add((max_frames + 1) * sizeof(lphy_ragged_desc), kStageOut)
        .add(sizeof(lphy_find_info), kStageOut)
        .add(work_bytes, kStageScratch);
}

// samples (those the outputs read) | taps | rot | out (all channels' strides;
// the caller's values go in, so that the slots past `outputs` come back as they
// went) - lphy_hip_channelize_host.  Like find_plan not among the plans
// lphy_hip_ctx_reserve sizes for: a wideband capture is not a frame shape.
// chan_raw_plan: the same for lphy_hip_channelize_raw_host, whose samples are
// of the capture's format: `in_bytes` = samples * lphy_hip_sample_bytes.
inline StagePlan chan_raw_plan(size_t in_bytes, size_t channels, size_t taps, size_t rot_period, size_t out_stride) {
    return StagePlan()
        .add(in_bytes, kStageIn)
        .add(channels * taps * kIqBytes, kStageIn)
        .add(channels * rot_period * kIqBytes, kStageIn)
        .add(channels * out_stride * kIqBytes, kStageInOut);
}
inline StagePlan chan_plan(size_t samples, size_t channels, size_t taps, size_t rot_period, size_t out_stride) {
    return chan_raw_plan(samples * kIqBytes, channels, taps, rot_period, out_stride);
}

// in (the channels' streams, first sample of the first to last sample of the
// last) | taps | rot | out (`outputs` samples, every one written) -
// lphy_hip_synthesize_host.  Beside chan_plan, and like it not among the plans
// lphy_hip_ctx_reserve sizes for.
inline StagePlan synth_plan(size_t in_samples, size_t channels, size_t taps, size_t rot_period, size_t outputs) {
    return StagePlan()
        .add(in_samples * kIqBytes, kStageIn)
        .add(channels * taps * kIqBytes, kStageIn)
        .add(channels * rot_period * kIqBytes, kStageIn)
        .add(outputs * kIqBytes, kStageOut);
}

// Staging every *_host entry point needs for calls of up to `frames` frames
// of `frame_samples` samples, or one buffer of frames * frame_samples: the
// largest of the eleven plans at that shape (the ragged estimate's slices are
// among the ragged demodulator's, so it never sets the size).  Demodulation in modes 1/2, which
// give no fewer symbols than mode 0; ragged frames of frame_samples each; one
// detector window per N samples of the buffer; one ragged detector record per
// whole symbol of the buffer (16 B a symbol: more than the ragged
// demodulator's outputs); all the frames' symbols in one
// decode; ragged transmit frames of frame_samples each, gaps or not (the
// ragged plan's slices less the records, so it never sets the size); one frame's symbols in one modulate (mod_scratch: its
// mod_scratch_bytes).  A call past that grows the staging.
inline size_t host_stage_bytes(size_t N, size_t osr, size_t frames, size_t frame_samples, size_t mod_scratch) {
    const size_t step = N * osr, n = frames * frame_samples, total = frame_samples / step;
    const size_t per = ragged_out_syms(total, LPHY_MODE_LORA_DEMODULATE);
    return std::max({demod_plan(frames, frame_samples, per).end,
                     ragged_plan(n, frames, frames * ((per + 1) & ~size_t(1))).end,
                     detect_plan(n, n / N).end,
                     detect_ragged_plan(n, frames, n / step).end,
                     decode_plan(frames * (total + 2)).end,
                     estimate_plan(n).end,
                     estimate_ragged_plan(n, frames).end,
                     compensate_plan(n).end,
                     compensate_batch_plan(frames, frame_samples).end,
                     modulate_plan(step, total, mod_scratch).end,
                     tx_plan(frames * (per / 2), frames, n, frames * ((per + 1) & ~size_t(1)), true, true).end});
}

}  // namespace lphy
