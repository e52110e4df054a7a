// lphy_ragged_layout.h — the descriptors of a ragged batch packed back to
// back (lphy_hip_ragged_layout) and the checks of a descriptor table the host
// can read (lphy_hip_demod_ragged_host).  Plain host C++, no HIP: the CPU
// tests compile it alone (tests/cpp/ragged_layout_check.cpp).
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdint>

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

}  // namespace lphy
