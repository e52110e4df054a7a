// Host-only test library over csrc/lphy_stage_plan.h and
// csrc/lphy_ragged_layout.h for lphy_hip_detect_ragged_host: its staging
// plan, the reservation and the table check it makes before any device call
// (tests/test_detect_ragged_plan_cpu.py loads it through ctypes).
#include "plan_dump.h"

using namespace lphy;

// out: plan_dump's
extern "C" int detect_ragged_plan_check(uint64_t iq_samples, uint64_t frames, uint64_t units, uint64_t* out) {
    return plan_dump(detect_ragged_plan(iq_samples, frames, units), out);
}

extern "C" uint64_t detect_ragged_reserve_check(uint64_t N, uint64_t osr, uint64_t frames, uint64_t frame_samples,
                                                uint64_t mod_scratch) {
    return host_stage_bytes(N, osr, frames, frame_samples, mod_scratch);
}

// desc: frames + 1 records of four uint64 (lphy_ragged_desc); out: IQ samples, units
extern "C" int detect_ragged_extent_check(uint64_t step, const uint64_t* desc, uint64_t frames, uint64_t* out) {
    return detect_ragged_extent(step, reinterpret_cast<const lphy_ragged_desc*>(desc), frames, &out[0], &out[1]);
}

// the same table through the ragged demodulator's check (mode 0)
extern "C" int demod_ragged_extent_check(uint64_t step, const uint64_t* desc, uint64_t frames) {
    uint64_t iq = 0, syms = 0;
    return ragged_extent(step, reinterpret_cast<const lphy_ragged_desc*>(desc), frames, LPHY_MODE_DEMODULATE, &iq,
                         &syms);
}
