// A StagePlan as the CPU tests read it: n, end, copied_end, up.begin, up.end,
// down.begin, down.end, then (off, size, role) per slice.  Returns the number
// of values written.
#pragma once
#include "lphy_stage_plan.h"

inline int plan_dump(const lphy::StagePlan& p, uint64_t* out) {
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
