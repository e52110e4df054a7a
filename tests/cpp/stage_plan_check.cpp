// Host-only test library over csrc/lphy_stage_plan.h: the staging plans the
// *_host entry points build and the reservation lphy_hip_ctx_reserve sizes,
// without a device (tests/test_stage_plan_cpu.py loads it through ctypes).
#include "plan_dump.h"

using namespace lphy;

// out: plan_dump's.  which / a: the plan function and its arguments in the
// header's order.  Returns the number of values written, 0 for a bad `which`.
extern "C" int stage_plan_check(int which, const uint64_t* a, uint64_t* out) {
    switch (which) {
        case 0: return plan_dump(demod_plan(a[0], a[1], a[2]), out);
        case 1: return plan_dump(ragged_plan(a[0], a[1], a[2]), out);
        case 2: return plan_dump(detect_plan(a[0], a[1]), out);
        case 3: return plan_dump(decode_plan(a[0]), out);
        case 4: return plan_dump(estimate_plan(a[0]), out);
        case 5: return plan_dump(compensate_plan(a[0]), out);
        case 6: return plan_dump(compensate_batch_plan(a[0], a[1]), out);
        case 7: return plan_dump(modulate_plan(a[0], a[1], a[2]), out);
        default: return 0;
    }
}

extern "C" uint64_t stage_reserve_check(uint64_t N, uint64_t osr, uint64_t frames, uint64_t frame_samples,
                                        uint64_t mod_scratch) {
    return host_stage_bytes(N, osr, frames, frame_samples, mod_scratch);
}

extern "C" int stage_max_slices(void) { return StagePlan::kMaxSlices; }
