// The host build of csrc/libm_exact.h over arrays, for tests/test_libm_cases_cpu.py
// (against glibc on the sets of tests/libm_cases.py) and for the failure
// report of tests/test_gpu_libm.py.  op as lphy_test_libm_op
// (csrc/lphy_testing.h); the last one restates detector_power (lphy_demod.h,
// device only) with the host sqrtf.  Build: g++ -O2 -ffp-contract=off -shared.
#include "../../lora-sdr-lightweight-standalone-library-clean_amd/csrc/libm_exact.h"

#include <stddef.h>

extern "C" int lphy_libm_host(int op, const float* a, const float* b, float* out0, float* out1, size_t n) {
    using namespace lphy_libm;
    if (op < 0 || op > 8) return -1;
    for (size_t i = 0; i < n; ++i) {
        const float x = a[i];
        switch (op) {
            case 0: sincosf_exact(x, &out0[i], &out1[i]); break;
            case 1:
                if (sincosf_needs_large(x)) sincosf_large(x, &out0[i], &out1[i]);
                else sincosf_fast(x, &out0[i], &out1[i]);
                break;
            case 2: sincosf_large(x, &out0[i], &out1[i]); break;
            case 3: out0[i] = atan2f_exact(x, b[i]); break;
            case 4: out0[i] = cabsf_exact(x, b[i]); break;
            case 5: out0[i] = logf_exact(x); break;
            case 6: out0[i] = log10f_exact(x); break;
            case 7: out0[i] = sqrtf(x); break;
            default: {
                const float fund = sqrtf(x);
                const float db = 20.0f * log10f_exact(fund);
                out0[i] = db - b[i];
            }
        }
    }
    return 0;
}
