// lphy_ragged_unit.h — "unit u of a ragged table" for the persistent kernels
// over a lphy_ragged_desc table (k_rg_demod, k_detect over DetRagged,
// k_tx_samples): everything between knowing the unit and the kernel's own
// per-frame limit.  Integer logic that a host compiler takes too
// (tests/cpp/ragged_unit_check.cpp); the wave-uniform step is device-only.
#pragma once
#include <cstdint>

#include "../../include/lphy_hip.h"
#include "lphy_hd.h"

namespace lphy {

// Frame of unit u in a ragged table (lphy_ragged_desc, frames + 1 records):
// the last record whose unit_offset is <= u, for u below the table's total
// (whatever the table holds, a frame below nframes).
LPHY_HD unsigned unit_frame(const lphy_ragged_desc* __restrict__ desc, unsigned nframes, unsigned long long u) {
    // unit_offset[lo] <= u < unit_offset[hi] throughout
    unsigned lo = 0, hi = nframes;
    while (hi - lo > 1) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (desc[mid].unit_offset <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct RaggedUnit {
    lphy_ragged_desc d;    // the frame's record (record 0 for a unit past the table)
    unsigned frame;
    unsigned long long s;  // the unit within the frame (meaningful when live)
    bool live;
};

// Unit u of a table of `units` units (record [nframes]'s unit_offset).
// UNIFORM: u is the same in every lane of the wavefront, so the search runs
// on scalar values.  live: u is below the total and not below the record's
// own offset, so a table whose prefix is wrong cannot lead outside the frame
// once the caller has checked s against the frame's own count.
template <bool UNIFORM>
LPHY_HD RaggedUnit ragged_unit(const lphy_ragged_desc* __restrict__ desc, unsigned nframes,
                                  unsigned long long units, unsigned long long u) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (UNIFORM) {
        const unsigned lo32 = __builtin_amdgcn_readfirstlane((unsigned)u);
        const unsigned hi32 = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
        u = ((unsigned long long)hi32 << 32) | lo32;
    }
#endif
    RaggedUnit r;
    r.live = u < units;
    r.frame = r.live ? unit_frame(desc, nframes, u) : 0u;
    r.d = desc[r.frame];
    r.s = u - r.d.unit_offset;
    r.live = r.live && r.d.unit_offset <= u;
    return r;
}

}  // namespace lphy
