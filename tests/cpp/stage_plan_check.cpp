// Host-only test library over csrc/lphy_stage_plan.h: the staging plans the
// *_host entry points build and the reservation lphy_hip_ctx_reserve sizes,
// without a device (tests/test_stage_plan_cpu.py loads it through ctypes).
#include "lphy_stage_plan.h"

using namespace lphy;

// out: n, end, copied_end, up.begin, up.end, down.begin, down.end, then
// (off, size, role) per slice.  which / a: the plan function and its arguments
// in the header's order.  Returns the number of values written, 0 for a bad `which`.
extern "C" int stage_plan_check(int which, const uint64_t* a, uint64_t* out) {
    StagePlan p;
    switch (which) {
        case 0: p = demod_plan(a[0], a[1], a[2]); break;
        case 1: p = ragged_plan(a[0], a[1], a[2]); break;
        case 2: p = detect_plan(a[0], a[1]); break;
        case 3: p = decode_plan(a[0]); break;
        case 4: p = estimate_plan(a[0]); break;
        case 5: p = compensate_plan(a[0]); break;
        case 6: p = compensate_batch_plan(a[0], a[1]); break;
        case 7: p = modulate_plan(a[0], a[1], a[2]); break;
        default: return 0;
    }
    const uint64_t head[7] = {(uint64_t)p.n, p.end, p.copied_end, p.up.begin, p.up.end, p.down.begin, p.down.end};
    int k = 0;
    for (uint64_t v : head) out[k++] = v;
    for (int i = 0; i < p.n; ++i) {
        out[k++] = p.s[i].off;
        out[k++] = p.s[i].size;
        out[k++] = p.s[i].role;
    }
    return k;
}

extern "C" uint64_t stage_reserve_check(uint64_t N, uint64_t osr, uint64_t frames, uint64_t frame_samples,
                                        uint64_t mod_scratch) {
    return host_stage_bytes(N, osr, frames, frame_samples, mod_scratch);
}

extern "C" int stage_max_slices(void) { return StagePlan::kMaxSlices; }
