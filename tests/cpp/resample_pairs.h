// Two violations at once for chan_args and synth_args (channelize_check.cpp,
// synthesize_check.cpp): the rows' expected codes are literals recorded from
// the argument checks as they stood before the two shared one head, so the
// order of the tests, which callers see as the first failing code, is pinned
// for every adjacent pair of tests and for pairs across the two codes.
#pragma once
#include <cstdint>
#include <cstdio>

// one way to fail each test, in the order of the shared head; the four behind
// V_OUTMAX come in each check's own order
enum V { V_CTX, V_PLAN, V_TABLES, V_IN, V_OUT, V_ALIGN, V_RES0, V_RES1, V_CH0, V_T0, V_STEP0, V_R0, V_CHMAX, V_TMAX,
         V_STEPMAX, V_RMAX, V_OUTMAX, V_STRIDE_SMALL, V_INMAX, V_FIRST, V_STRIDE_BIG };
struct Pair { V a, b; int want; };
struct Call { bool ctx = true, plan = true, tables = true, in = true, out = true, aligned = true; };

template <class P>
void violate(V v, Call& c, P& p, uint32_t P::*step, uint64_t P::*stride) {
    const uint64_t k48 = uint64_t(1) << 48;
    switch (v) {
        case V_CTX: c.ctx = false; break;
        case V_PLAN: c.plan = false; break;
        case V_TABLES: c.tables = false; break;
        case V_IN: c.in = false; break;
        case V_OUT: c.out = false; break;
        case V_ALIGN: c.aligned = false; break;
        case V_RES0: p.reserved[0] = 1; break;
        case V_RES1: p.reserved[1] = 1; break;
        case V_CH0: p.channels = 0; break;
        case V_T0: p.taps = 0; break;
        case V_STEP0: p.*step = 0; break;
        case V_R0: p.rot_period = 0; break;
        case V_CHMAX: p.channels = 65; break;
        case V_TMAX: p.taps = 4097; break;
        case V_STEPMAX: p.*step = 65537; break;
        case V_RMAX: p.rot_period = 65537; break;
        case V_OUTMAX: p.outputs = uint64_t(1) << 32; break;
        case V_STRIDE_SMALL: p.*stride = 0; break;
        case V_INMAX: p.in_samples = p.*stride = k48 + 1; break;
        case V_FIRST: p.first = ~uint64_t(0); break;
        case V_STRIDE_BIG: p.*stride = k48; break;
    }
}

template <class P, size_t N>
int pairs_check(const Pair (&rows)[N], const P& good, int (*args)(bool, const P*, bool, bool, bool, bool),
                uint32_t P::*step, uint64_t P::*stride) {
    for (const Pair& r : rows) {
        Call c;
        P p = good;
        violate(r.a, c, p, step, stride);
        violate(r.b, c, p, step, stride);
        const int rc = args(c.ctx, c.plan ? &p : nullptr, c.tables, c.in, c.out, c.aligned);
        if (rc != r.want) {
            std::printf("FAILED pair (%d, %d): %d, want %d\n", (int)r.a, (int)r.b, rc, r.want);
            return 1;
        }
    }
    return 0;
}
