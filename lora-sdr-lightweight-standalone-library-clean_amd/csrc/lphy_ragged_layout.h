// lphy_ragged_layout.h — everything the calls on a ragged descriptor table
// (lphy_ragged_desc) share that is not a kernel: the frame geometry and the
// limits (host and device), the table builders (lphy_hip_ragged_layout,
// lphy_hip_tx_layout), the one walk over a caller's table that the *_host
// forms check it with, and the entry points' argument checks.  Plain C++ with
// LPHY_RG_HD in front of what the kernels call too, no HIP: the CPU tests
// compile it alone (tests/cpp/ragged_layout_check.cpp, ragged_walk_check.cpp,
// tx_layout_check.cpp, find_frames_check.cpp).
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/lphy_hip.h"

// not lphy_hd.h's LPHY_HD: this one stands before `constexpr` and `inline`, here and in lphy_lorawan_ragged.h
#if defined(__HIPCC__)
#define LPHY_RG_HD __host__ __device__
#else
#define LPHY_RG_HD
#endif

namespace lphy {

constexpr uint64_t kRaggedMaxSamples = uint64_t(1) << 31;  // per frame, exclusive
constexpr uint64_t kRaggedMaxUnits = uint64_t(1) << 32;    // whole symbols per call, exclusive
constexpr uint64_t kRaggedMaxFrames = 0x7fffffff;          // frames (records, jobs) per call, inclusive
constexpr uint64_t kRaggedMaxOffset = uint64_t(1) << 48;   // iq_offset and sym_offset, inclusive

// lphy_hip_syms_per_frame for `total` whole symbols
LPHY_RG_HD constexpr uint64_t ragged_out_syms(uint64_t total, int mode) {
    return total >= 2 ? total - 2 : (mode == LPHY_MODE_DEMODULATE ? 0 : total);
}

// the symbols the demodulator's estimate takes (LoRaDemod.cpp:80 / phy.cpp:196)
LPHY_RG_HD constexpr uint64_t ragged_est_syms(uint64_t total, int mode) {
    return mode == LPHY_MODE_DEMODULATE ? 2 : (total < 2 ? total : 2);
}

// h_desc[frames + 1] from h_samples[frames]: frames back to back in the IQ,
// output symbols packed by ragged_out_syms with every sym_offset even (frame
// f's bytes start at sym_offset / 2), unit_offset the exclusive prefix of
// whole symbols; record [frames] holds the totals.  step = N * osr.
inline int ragged_layout(uint64_t step, const uint64_t* h_samples, size_t frames, int mode,
                         lphy_ragged_desc* h_desc) {
    if (!h_desc || (frames && !h_samples) || step == 0) return -EINVAL;
    if (mode < 0 || mode > 2) return -EINVAL;
    uint64_t iq = 0, sym = 0, unit = 0;
    for (size_t f = 0; f < frames; ++f) {
        const uint64_t n = h_samples[f];
        if (n >= kRaggedMaxSamples) return -ERANGE;
        const uint64_t total = n / step;
        h_desc[f] = lphy_ragged_desc{iq, n, sym, unit};
        iq += n;
        sym += (ragged_out_syms(total, mode) + 1) & ~uint64_t(1);
        unit += total;
        if (unit >= kRaggedMaxUnits) return -ERANGE;
    }
    h_desc[frames] = lphy_ragged_desc{iq, 0, sym, unit};
    return 0;
}

// ragged_walk's per-frame hook when the caller has none
struct NoFrame {
    void operator()(const lphy_ragged_desc&, uint64_t) const {}
};

// A caller's table (host copy), for every *_host form: the limits, the
// unit_offset prefix (record [frames] included) and the extents of the IQ, of
// the output symbols and of the whole symbols it names, written when 0 is
// returned and not otherwise.  A null out_syms / units: the call does not
// read sym_offset / unit_offset, and that field's checks and sums are not
// made.  step = N * osr.  frame(d, total) sees every frame the checks passed,
// in record order.
template <class F = NoFrame>
int ragged_walk(uint64_t step, const lphy_ragged_desc* h_desc, size_t frames, int mode, uint64_t* iq_samples,
                uint64_t* out_syms, uint64_t* units, F&& frame = F{}) {
    uint64_t iq = 0, sym = 0, unit = 0;
    for (size_t f = 0; f < frames; ++f) {
        const lphy_ragged_desc& d = h_desc[f];
        if (d.samples >= kRaggedMaxSamples) return -ERANGE;
        if (units && d.unit_offset != unit) return -EINVAL;
        if (d.iq_offset > kRaggedMaxOffset || (out_syms && d.sym_offset > kRaggedMaxOffset)) return -ERANGE;
        const uint64_t total = d.samples / step;
        if (units) unit += total;
        if (unit >= kRaggedMaxUnits) return -ERANGE;
        if (d.iq_offset + d.samples > iq) iq = d.iq_offset + d.samples;
        const uint64_t end = out_syms ? d.sym_offset + ragged_out_syms(total, mode) : 0;
        if (end > sym) sym = end;
        frame(d, total);
    }
    if (units && h_desc[frames].unit_offset != unit) return -EINVAL;
    *iq_samples = iq;
    if (out_syms) *out_syms = sym;
    if (units) *units = unit;
    return 0;
}

// The walk as lphy_hip_demod_ragged_host makes it (the units are checked, the
// caller takes them from record [frames]) ...
inline int ragged_extent(uint64_t step, const lphy_ragged_desc* h_desc, size_t frames, int mode,
                         uint64_t* iq_samples, uint64_t* out_syms) {
    uint64_t units = 0;
    return ragged_walk(step, h_desc, frames, mode, iq_samples, out_syms, &units);
}
// ... lphy_hip_estimate_ragged_host (iq_offset and samples alone: no symbol is
// counted, so the step and the mode are not used; 1 keeps the division defined) ...
inline int estimate_ragged_extent(const lphy_ragged_desc* h_desc, size_t frames, uint64_t* iq_samples) {
    return ragged_walk(1, h_desc, frames, LPHY_MODE_DEMODULATE, iq_samples, nullptr, nullptr);
}
// ... and lphy_hip_detect_ragged_host (no sym_offset, so no mode)
inline int detect_ragged_extent(uint64_t step, const lphy_ragged_desc* h_desc, size_t frames, uint64_t* iq_samples,
                                uint64_t* units) {
    return ragged_walk(step, h_desc, frames, LPHY_MODE_DEMODULATE, iq_samples, nullptr, units);
}

// lphy_hip_tx_layout: the table of frames that carry h_len_bytes[f] payload
// bytes each, (2 len + 2) symbols of `step` samples, as ragged_layout packs
// them in mode 1 - so sym_offset / 2 is the exclusive prefix of len and the
// same table demodulates the IQ back into bytes at the same offsets.
inline int tx_layout(uint64_t step, const uint64_t* h_len_bytes, size_t frames, lphy_ragged_desc* h_desc) {
    if (!h_desc || (frames && !h_len_bytes) || step == 0) return -EINVAL;
    std::vector<uint64_t> samples;
    try {
        samples.resize(frames);
    } catch (const std::bad_alloc&) {
        return -ENOMEM;
    }
    for (size_t f = 0; f < frames; ++f) {
        // (2 len + 2) * step < 2^31 without overflow
        if (h_len_bytes[f] >= kRaggedMaxSamples) return -ERANGE;
        const uint64_t syms = 2 * h_len_bytes[f] + 2;
        if (syms > (kRaggedMaxSamples - 1) / step) return -ERANGE;
        samples[f] = syms * step;
    }
    return ragged_layout(step, samples.data(), frames, LPHY_MODE_LORA_DEMODULATE, h_desc);
}

// A caller's table for lphy_hip_tx_ragged_host: ragged_walk's checks first,
// whichever frame fails them; then every frame must be whole symbols, at
// least the two sync symbols, and an even number of data symbols (-EINVAL
// otherwise).  Besides the walk's extents: the bytes the frames read (the
// largest sym_offset / 2 + nsyms / 2) and whether the frames cover their IQ /
// symbol extent without a gap (frames must not overlap, so the sums say so).
// *x is written when 0 is returned and not otherwise.
struct TxExtent {
    uint64_t iq_samples = 0, out_syms = 0, in_bytes = 0;
    bool iq_gaps = false, sym_gaps = false;
};

inline int tx_extent(uint64_t step, const lphy_ragged_desc* h_desc, size_t frames, TxExtent* x) {
    TxExtent t;
    uint64_t iq_sum = 0, sym_sum = 0, units = 0;
    bool whole = true;
    auto frame = [&](const lphy_ragged_desc& d, uint64_t total) {
        if (d.samples % step || total < 2 || (total & 1)) whole = false;
        const uint64_t nsyms = ragged_out_syms(total, LPHY_MODE_LORA_DEMODULATE);
        iq_sum += d.samples;
        sym_sum += nsyms;
        if (d.sym_offset / 2 + nsyms / 2 > t.in_bytes) t.in_bytes = d.sym_offset / 2 + nsyms / 2;
    };
    const int rc =
        ragged_walk(step, h_desc, frames, LPHY_MODE_LORA_DEMODULATE, &t.iq_samples, &t.out_syms, &units, frame);
    if (rc) return rc;
    if (!whole) return -EINVAL;
    t.iq_gaps = iq_sum != t.iq_samples;
    t.sym_gaps = sym_sum != t.out_syms;
    *x = t;
    return 0;
}

// ---- the entry points' argument checks, device and host forms alike, in the
// order include/lphy_hip.h documents (before any device call): 0 to go on, 1
// when there is nothing to do, or the error.

// what the checks read of a context; ok: the context is not null
struct RaggedCtx {
    bool ok;
    unsigned sf, osr;
};

// estimate, modulate / tx, detect, compensate.  valid: every required pointer
// is there (detect: and no unknown flag bit, and phase < osr); min_sf: 7, and 0
// for compensate, which has no transform.
constexpr int ragged_args(RaggedCtx c, size_t frames, bool valid, unsigned min_sf = 7) {
    if (!c.ok) return -EINVAL;
    if (frames == 0) return 1;
    if (!valid) return -EINVAL;
    if (frames > kRaggedMaxFrames) return -ERANGE;
    if (c.sf < min_sf) return -ENOTSUP;
    return 0;
}

constexpr int detect_ragged_args(RaggedCtx c, size_t frames, bool ptrs, unsigned phase, unsigned flags) {
    return ragged_args(c, frames, ptrs && !(flags & ~(unsigned)LPHY_DET_DECHIRP) && phase < c.osr);
}

// demod: the context among the pointers, frames == 0 last of what needs no table
constexpr int demod_ragged_args(RaggedCtx c, bool ptrs, int mode, unsigned flags, bool bytes, size_t frames) {
    if (!c.ok || !ptrs) return -EINVAL;
    if (mode < 0 || mode > 2) return -EINVAL;
    if (flags & ~(unsigned)(LPHY_F_DECODE | LPHY_F_NO_SCRATCH)) return -ENOTSUP;
    if (c.osr != 1 || c.sf < 7) return -ENOTSUP;
    if ((flags & LPHY_F_DECODE) && !bytes) return -EINVAL;
    if (frames == 0) return 1;
    if (frames > kRaggedMaxFrames) return -ERANGE;
    return 0;
}

// find_frames.  ptrs: the table and the info are there; rec: the records are
// (asked for with windows > 0 only); work: the workspace is there and 16-byte
// aligned (the host form lends its own: true); step = N * osr, of a context
// that is not null.  windows == 0 goes on: the call writes the padding.  The
// two sums are bounded by division, so neither wraps.
inline int find_frames_args(RaggedCtx c, const lphy_find_params* p, bool ptrs, bool rec, bool work, uint64_t step,
                            uint64_t windows, int mode, uint64_t max_frames) {
    if (!c.ok || !p || !ptrs) return -EINVAL;
    if (windows > 0 && !rec) return -EINVAL;
    if (!work) return -EINVAL;
    if (p->hop == 0 || p->min_symbols == 0 || max_frames == 0) return -EINVAL;
    if (p->threshold_db != p->threshold_db) return -EINVAL;
    if (p->reserved != 0) return -EINVAL;
    if (mode < 0 || mode > 2) return -EINVAL;
    if (windows >= kRaggedMaxUnits) return -ERANGE;
    if (max_frames > kRaggedMaxFrames) return -ERANGE;
    // first + lead + windows * hop <= 2^48
    if (p->first > kRaggedMaxOffset || p->lead > kRaggedMaxOffset - p->first) return -ERANGE;
    const uint64_t room = kRaggedMaxOffset - p->first - p->lead;
    if (windows && p->hop > room / windows) return -ERANGE;
    // windows * hop / step < 2^32 (the product is at most 2^48 here)
    if (windows * p->hop / step >= kRaggedMaxUnits) return -ERANGE;
    return 0;
}

}  // namespace lphy
