// lphy_testing.h — comparison / test paths of lphy_hip_demod_batch, not part
// of the public C ABI (include/lphy_hip.h).  The flag bits are accepted only
// by the test-only build (Makefile `test`: lib/test/liblphy_hip.so, compiled
// with -DLPHY_TEST_PATHS and -DLPHY_DEBUG_BOUNDS); the product library
// rejects them with -EINVAL.  The kernels are the same code: the flags only
// select schedules the tests use as references.
//
// The same holds for the launch overrides below: only the test build reads
// them from the environment; the product library's dispatch depends on the
// call's arguments and lphy_hip_ctx_set_fused_min_frames alone.
//   * lphy_hip_test_grid_cap(ctx, blocks), per context (0 restores the
//     default): the persistent grids of k_rg_demod, k_detect (both
//     geometries) and k_tx_samples get min(grid, blocks) workgroups, after the
//     launchers' own caps (units_hint, the call's tiles): the last argument
//     of persistent_grid (lphy_args.h).  Those kernels are launched with
//     min(resident grid, tiles of the call) workgroups, so their grid-stride
//     loops take a second trip only in a call with more tiles than the device
//     holds workgroups; under a cap of 1 one workgroup walks every tile, under
//     a small cap the workgroups make unequal numbers of trips
//     (tests/test_gpu_persistent_trips.py).  A host-side argument of the
//     launchers: no kernel reads it, and the product library has neither the
//     symbol nor the cap.  The uniform kernels (k_wave, k_demod, k_frames)
//     are outside it: the suite's larger batches walk their grids many times.
//   * lphy_hip_test_libm(ctx, op, d_a, d_b, d_out0, d_out1, n, stream): the
//     functions of libm_exact.h, the device sqrtf and detector_power as the
//     kernels call them, one element per input, so that the tests see what
//     hipcc makes of the header for the device over inputs they choose
//     (tests/test_gpu_libm.py against glibc through the oracle).  The product
//     library has no such symbol.
#pragma once

#include <cstddef>
#include <cstdlib>

// lphy_hip_test_libm's `op`: a is the argument (ATAN2: y, CABS: re,
// DETECTOR_POWER: max_value), b the second one where there is one (ATAN2: x,
// CABS: im, DETECTOR_POWER: power_scale); the sincos ops write sin to out0
// and cos to out1, the others their value to out0.
enum lphy_test_libm_op {
    LPHY_LIBM_SINCOS_EXACT = 0,    // sincosf_exact
    LPHY_LIBM_SINCOS_SPLIT = 1,    // sincosf_needs_large ? sincosf_large : sincosf_fast (rotate_sample)
    LPHY_LIBM_SINCOS_LARGE = 2,    // sincosf_large alone, whatever the argument
    LPHY_LIBM_ATAN2 = 3,
    LPHY_LIBM_CABS = 4,
    LPHY_LIBM_LOGF = 5,
    LPHY_LIBM_LOG10F = 6,
    LPHY_LIBM_SQRTF = 7,           // the device sqrtf of unit_result
    LPHY_LIBM_DETECTOR_POWER = 8,  // detector_power (lphy_demod.h)
    LPHY_LIBM_OPS = 9,
};

#ifdef LPHY_TEST_PATHS
struct lphy_hip_ctx;
// Test build only.  -EINVAL for a null ctx, a null pointer the op uses (d_b
// and d_out1 may be null for the ops that do not) or an unknown op; then 0
// for n == 0; -ERANGE for n >= 2^32.  Asynchronous on `stream`.
extern "C" int lphy_hip_test_libm(lphy_hip_ctx* ctx, int op, const float* d_a, const float* d_b, float* d_out0,
                                  float* d_out1, size_t n, void* stream);
#endif

// A context's device counters (lphy_hip_ctx::d_counters, kCounters slots),
// each with a slot of its own (the modulator's fallback count
// shared slot 8 with the phase clocks, and the modulator clocks slot 1 with
// the Parseval count):
constexpr int kCtrRecheck = 0;    // symbols re-run exactly (lphy_hip_recheck_count)
constexpr int kCtrParseval = 1;   // test build: symbols the wave kernel certified by Parseval
constexpr int kCtrModSerial = 2;  // frames k_mod_fast gave to its serial walk
constexpr int kCtrDetectSerial = 3;  // windows k_detect summed in bin order (lphy_hip_detect_serial_count)
constexpr int kCtrClocks = 8;     // timing builds only: 8 phase-clock sums (lphy_hip_phase_cycles)
constexpr int kCounters = 16;

enum lphy_test_flags {
    LPHY_F_EXACT_ROTATION = 64u,   // every symbol with the reference's per-sample
                                   // sincos rotation instead of the certified
                                   // per-frame table (tests/test_gpu_fast_rotation.py)
    LPHY_F_SCAN_FIRST = 256u,      // modes 1/2: whole-frame max-abs pre-scan
                                   // instead of the speculative normalisation
                                   // (tests/test_gpu_spec.py)
    LPHY_F_DEBUG_RECHECK = 512u,   // separate launches: every estimated frame
                                   // marked "has open symbols" first; fused
                                   // kernels: every symbol left to k_post's
                                   // exact re-run (tests/test_gpu_concurrency.py)
    LPHY_F_FRAMES_KERNEL = 1024u,  // SF 7-10: k_frames where k_wave would run
                                   // (the certificate tests on k_frames,
                                   // tests/test_gpu_certificate.py)
};
constexpr unsigned kTestFlags =
    LPHY_F_EXACT_ROTATION | 128u | LPHY_F_SCAN_FIRST | LPHY_F_DEBUG_RECHECK | LPHY_F_FRAMES_KERNEL;

// Test build only: LPHY_FUSED_MIN_FRAMES sets the process default of the
// smallest batch the fused kernels take (the lora_phy:: probes run once with
// it at 0 through this build).  -1: the measured per-SF crossover.
inline long lphy_test_fused_min_frames() {
#ifdef LPHY_TEST_PATHS
    static const long v = [] {
        const char* e = std::getenv("LPHY_FUSED_MIN_FRAMES");
        return e ? std::atol(e) : -1L;
    }();
    return v;
#else
    return -1L;
#endif
}
