// lphy_ragged_layout.h — the descriptors of a ragged batch packed back to
// back (lphy_hip_ragged_layout) and the checks of a descriptor table the host
// can read (lphy_hip_demod_ragged_host), and the same two for the transmit
// direction (lphy_hip_tx_layout, lphy_hip_tx_ragged_host).  Plain host C++, no
// HIP: the CPU tests compile it alone (tests/cpp/ragged_layout_check.cpp,
// tests/cpp/tx_layout_check.cpp).
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/lphy_hip.h"

namespace lphy {

constexpr uint64_t kRaggedMaxSamples = uint64_t(1) << 31;  // per frame, exclusive
constexpr uint64_t kRaggedMaxUnits = uint64_t(1) << 32;    // whole symbols per call, exclusive

// lphy_hip_syms_per_frame for `total` whole symbols
constexpr uint64_t ragged_out_syms(uint64_t total, int mode) {
    if (mode == LPHY_MODE_DEMODULATE) return total >= 2 ? total - 2 : 0;
    return total >= 2 ? total - 2 : total;
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

// A caller's table (host copy): the limits, the unit_offset prefix, and the
// extents of the IQ and of the output symbols it names.
inline int ragged_extent(uint64_t step, const lphy_ragged_desc* h_desc, size_t frames, int mode,
                         uint64_t* iq_samples, uint64_t* out_syms) {
    uint64_t iq = 0, sym = 0, unit = 0;
    for (size_t f = 0; f < frames; ++f) {
        const lphy_ragged_desc& d = h_desc[f];
        if (d.samples >= kRaggedMaxSamples) return -ERANGE;
        if (d.unit_offset != unit) return -EINVAL;
        if (d.iq_offset > (uint64_t(1) << 48) || d.sym_offset > (uint64_t(1) << 48)) return -ERANGE;
        const uint64_t total = d.samples / step;
        unit += total;
        if (unit >= kRaggedMaxUnits) return -ERANGE;
        if (d.iq_offset + d.samples > iq) iq = d.iq_offset + d.samples;
        const uint64_t end = d.sym_offset + ragged_out_syms(total, mode);
        if (end > sym) sym = end;
    }
    if (h_desc[frames].unit_offset != unit) return -EINVAL;
    *iq_samples = iq;
    *out_syms = sym;
    return 0;
}

// A caller's table for lphy_hip_estimate_ragged_host: the limits of
// ragged_extent on the two fields that call reads (iq_offset, samples) and the
// extent of the IQ they name.  No prefix check: unit_offset is not read.
inline int estimate_ragged_extent(const lphy_ragged_desc* h_desc, size_t frames, uint64_t* iq_samples) {
    uint64_t iq = 0;
    for (size_t f = 0; f < frames; ++f) {
        const lphy_ragged_desc& d = h_desc[f];
        if (d.samples >= kRaggedMaxSamples) return -ERANGE;
        if (d.iq_offset > (uint64_t(1) << 48)) return -ERANGE;
        if (d.iq_offset + d.samples > iq) iq = d.iq_offset + d.samples;
    }
    *iq_samples = iq;
    return 0;
}

// A caller's table for lphy_hip_detect_ragged_host: ragged_extent's limits
// and prefix check on the three fields that call reads (iq_offset, samples,
// unit_offset; step = N * osr), the extent of the IQ they name and the whole
// symbols, one record each.  sym_offset is not read.
inline int detect_ragged_extent(uint64_t step, const lphy_ragged_desc* h_desc, size_t frames, uint64_t* iq_samples,
                                uint64_t* units) {
    uint64_t iq = 0, unit = 0;
    for (size_t f = 0; f < frames; ++f) {
        const lphy_ragged_desc& d = h_desc[f];
        if (d.samples >= kRaggedMaxSamples) return -ERANGE;
        if (d.unit_offset != unit) return -EINVAL;
        if (d.iq_offset > (uint64_t(1) << 48)) return -ERANGE;
        unit += d.samples / step;
        if (unit >= kRaggedMaxUnits) return -ERANGE;
        if (d.iq_offset + d.samples > iq) iq = d.iq_offset + d.samples;
    }
    if (h_desc[frames].unit_offset != unit) return -EINVAL;
    *iq_samples = iq;
    *units = unit;
    return 0;
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

// A caller's table for lphy_hip_tx_ragged_host: ragged_extent's checks, then
// every frame must be whole symbols, at least the two sync symbols, and an
// even number of data symbols (-EINVAL otherwise).  Besides the extents of
// the IQ and of the symbols: the bytes the frames read (the largest
// sym_offset / 2 + nsyms / 2) and whether the frames cover their IQ / symbol
// extent without a gap (frames must not overlap, so the sums say so).
struct TxExtent {
    uint64_t iq_samples = 0, out_syms = 0, in_bytes = 0;
    bool iq_gaps = false, sym_gaps = false;
};

inline int tx_extent(uint64_t step, const lphy_ragged_desc* h_desc, size_t frames, TxExtent* x) {
    if (int rc = ragged_extent(step, h_desc, frames, LPHY_MODE_LORA_DEMODULATE, &x->iq_samples, &x->out_syms))
        return rc;
    uint64_t iq_sum = 0, sym_sum = 0;
    x->in_bytes = 0;
    for (size_t f = 0; f < frames; ++f) {
        const lphy_ragged_desc& d = h_desc[f];
        const uint64_t total = d.samples / step;
        if (d.samples % step || total < 2 || (total & 1)) return -EINVAL;
        const uint64_t nsyms = total - 2;
        iq_sum += d.samples;
        sym_sum += nsyms;
        if (d.sym_offset / 2 + nsyms / 2 > x->in_bytes) x->in_bytes = d.sym_offset / 2 + nsyms / 2;
    }
    x->iq_gaps = iq_sum != x->iq_samples;
    x->sym_gaps = sym_sum != x->out_syms;
    return 0;
}

}  // namespace lphy
