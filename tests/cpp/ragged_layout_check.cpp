// Host-only test library over csrc/lphy_ragged_layout.h: the function
// lphy_hip_ragged_layout runs for a context of (sf, osr), without a device
// (tests/test_ragged_layout_cpu.py loads it through ctypes).
#include "lphy_ragged_layout.h"

extern "C" int ragged_layout_check(unsigned sf, unsigned osr, const uint64_t* h_samples, size_t frames, int mode,
                                   lphy_ragged_desc* h_desc) {
    return lphy::ragged_layout((uint64_t(1) << sf) * osr, h_samples, frames, mode, h_desc);
}

extern "C" int ragged_extent_check(unsigned sf, const lphy_ragged_desc* h_desc, size_t frames, int mode,
                                   uint64_t* iq_samples, uint64_t* out_syms) {
    return lphy::ragged_extent(uint64_t(1) << sf, h_desc, frames, mode, iq_samples, out_syms);
}

extern "C" size_t ragged_desc_size(void) { return sizeof(lphy_ragged_desc); }
