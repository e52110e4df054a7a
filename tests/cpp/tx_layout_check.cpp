// Host-only test library over the ragged transmit path's host arithmetic:
// csrc/lphy_ragged_layout.h (tx_layout: what lphy_hip_tx_layout runs for a
// context of (sf, osr); tx_extent: the table checks of
// lphy_hip_tx_ragged_host) and csrc/lphy_stage_plan.h (tx_plan), without a
// device (tests/test_tx_layout_cpu.py loads it through ctypes).
#include "plan_dump.h"

using namespace lphy;

extern "C" int tx_layout_check(unsigned sf, unsigned osr, const uint64_t* h_len_bytes, size_t frames,
                               lphy_ragged_desc* h_desc) {
    return tx_layout((uint64_t(1) << sf) * osr, h_len_bytes, frames, h_desc);
}

extern "C" int tx_ragged_layout_check(unsigned sf, unsigned osr, const uint64_t* h_samples, size_t frames,
                                      lphy_ragged_desc* h_desc) {
    return ragged_layout((uint64_t(1) << sf) * osr, h_samples, frames, LPHY_MODE_LORA_DEMODULATE, h_desc);
}

// out: iq_samples, out_syms, in_bytes, iq_gaps, sym_gaps
extern "C" int tx_extent_check(unsigned sf, unsigned osr, const lphy_ragged_desc* h_desc, size_t frames,
                               uint64_t* out) {
    TxExtent x;
    const int rc = tx_extent((uint64_t(1) << sf) * osr, h_desc, frames, &x);
    if (rc) return rc;
    out[0] = x.iq_samples;
    out[1] = x.out_syms;
    out[2] = x.in_bytes;
    out[3] = x.iq_gaps;
    out[4] = x.sym_gaps;
    return 0;
}

// a: in_bytes, frames, iq_samples, out_syms, iq_gaps, sym_gaps.  out: plan_dump's.
extern "C" int tx_plan_check(const uint64_t* a, uint64_t* out) {
    return plan_dump(tx_plan(a[0], a[1], a[2], a[3], a[4] != 0, a[5] != 0), out);
}

extern "C" uint64_t tx_reserve_check(uint64_t N, uint64_t osr, uint64_t frames, uint64_t frame_samples,
                                     uint64_t mod_scratch) {
    return host_stage_bytes(N, osr, frames, frame_samples, mod_scratch);
}

extern "C" int tx_max_slices(void) { return StagePlan::kMaxSlices; }
