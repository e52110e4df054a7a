// Host-only test library over csrc/lphy_stage_plan.h and
// csrc/lphy_ragged_layout.h for lphy_hip_estimate_ragged_host: its staging
// plan, the reservation and the table check it makes before any device call
// (tests/test_estimate_ragged_cpu.py loads it through ctypes).
#include "plan_dump.h"

using namespace lphy;

// out: plan_dump's
extern "C" int estimate_ragged_plan_check(uint64_t iq_samples, uint64_t frames, uint64_t* out) {
    return plan_dump(estimate_ragged_plan(iq_samples, frames), out);
}

extern "C" uint64_t estimate_ragged_reserve_check(uint64_t N, uint64_t osr, uint64_t frames, uint64_t frame_samples,
                                                  uint64_t mod_scratch) {
    return host_stage_bytes(N, osr, frames, frame_samples, mod_scratch);
}

// desc: frames records of four uint64 (lphy_ragged_desc)
extern "C" int estimate_ragged_extent_check(const uint64_t* desc, uint64_t frames, uint64_t* iq_samples) {
    return estimate_ragged_extent(reinterpret_cast<const lphy_ragged_desc*>(desc), frames, iq_samples);
}
