// lphy_launch.h — the host launch templates of one spreading factor, the
// entries of its SfOps table (lphy_sf.hip, the only includer).  Which of
// them a call takes is lphy_route.h's decision (lphy_hip.hip); which kernels
// exist here follows the same header's frames_kernel / wave_kernel, so a
// routed call always finds its kernel and the -ENOTSUP returns below only
// guard a table entry that does not exist.  Every persistent grid here is
// persistent_grid over resident_blocks<K> / device_cus (lphy_args.h).
#pragma once
#include <type_traits>

#include "lphy_demod.h"
#include "lphy_detect.h"
#include "lphy_frames.h"
#include "lphy_post.h"
#include "lphy_ragged.h"
#include "lphy_route.h"
#include "lphy_wave.h"

namespace {

// The kernels' compile-time MODE of a call: the lphy_mode, kWinBit with a
// window (WIN: the kernel family has windowed forms), kOsrBit with osr > 1
// (OSR: ... oversampled forms).  Calls fn(std::integral_constant<int, MODE>).
template <int BITS, class Fn>
int with_mode_bits(int mode, Fn&& fn) {
    switch (mode) {
        case LPHY_MODE_DEMODULATE: return fn(std::integral_constant<int, LPHY_MODE_DEMODULATE | BITS>{});
        case LPHY_MODE_LORA_DEMODULATE: return fn(std::integral_constant<int, LPHY_MODE_LORA_DEMODULATE | BITS>{});
        default: return fn(std::integral_constant<int, LPHY_MODE_DECHIRP_LORA_DEMODULATE | BITS>{});
    }
}
template <bool WIN, bool OSR, class Fn>
int with_mode(int mode, bool win, bool osr, Fn&& fn) {
    if constexpr (OSR) {
        if (osr) return win ? with_mode_bits<kWinBit | kOsrBit>(mode, fn) : with_mode_bits<kOsrBit>(mode, fn);
    }
    if constexpr (WIN) {
        if (win) return with_mode_bits<kWinBit>(mode, fn);
    }
    return with_mode_bits<0>(mode, fn);
}

// The detector's compile-time PREP of a call (lphy_detect.h).  Calls
// fn(std::integral_constant<int, PREP>).
template <class Fn>
void with_prep(bool dechirp, bool win, Fn&& fn) {
    switch ((dechirp ? kPrepDechirp : 0) | (win ? kPrepWindow : 0)) {
        case 0: fn(std::integral_constant<int, 0>{}); break;
        case kPrepDechirp: fn(std::integral_constant<int, kPrepDechirp>{}); break;
        case kPrepWindow: fn(std::integral_constant<int, kPrepWindow>{}); break;
        default: fn(std::integral_constant<int, kPrepDechirp | kPrepWindow>{}); break;
    }
}

// Waves per SIMD the demod kernel is register-budgeted for (launch bound):
// 3 (<= 168 VGPRs) or 2 (<= 256; the oversampled forms).
constexpr int demod_occ(int sf) { return sf <= 8 ? 3 : 2; }

// per_cu > 0 caps the persistent grid at per_cu workgroups per CU (room
// for a concurrent kernel on another stream)
template <int SF, int MODE, int OCC>
void launch_symbols(const DemodArgs& A0, hipStream_t st, int per_cu) {
    using G = Geo<SF>;
    constexpr bool WAVE = G::LPS <= 64;
    constexpr int WT = WAVE ? 64 / G::LPS : G::T;      // symbols per worker tile
    constexpr int WPB = WAVE ? kTile / 64 : 1;         // workers per workgroup
    const int dev = current_device();
    const unsigned long long wtiles = (A0.frames * A0.total_syms + WT - 1) / WT;
    const unsigned long long grid =
        persistent_grid(resident_blocks<&k_demod<SF, MODE, OCC>>(dev), (wtiles + WPB - 1) / WPB,
                        per_cu > 0 ? (unsigned long long)per_cu * device_cus(dev) : 0);
    DemodArgs A = A0;
    const unsigned long long stride = grid * WPB * WT;  // symbols per worker step
    A.stride_f = (unsigned)(stride / A0.total_syms);
    A.stride_s = (unsigned)(stride % A0.total_syms);
    hipLaunchKernelGGL((k_demod<SF, MODE, OCC>), dim3((unsigned)grid), dim3(kTile), 0, st, A);
}

// The separate launches: prologue (k_maxabs in modes 1/2, k_estimate) and /
// or the symbols (k_demod).
template <int SF>
int launch_demod_sf(const DemodArgs& A, hipStream_t st, bool prologue, bool symbols, int per_cu) {
    using G = Geo<SF>;
    if (prologue) {
        if (A.mode != LPHY_MODE_DEMODULATE)
            hipLaunchKernelGGL(k_maxabs<SF>, dim3((unsigned)A.frames), dim3(kTile), 0, st, A);
        const int fpt = A.est_units <= G::T ? G::T / A.est_units : 1;
        const unsigned long long blocks = (A.frames + fpt - 1) / fpt;
        hipLaunchKernelGGL(k_estimate<SF>, dim3((unsigned)blocks), dim3(kTile), 0, st, A);
    }
    if (symbols && A.frames * A.total_syms) {
        with_mode<true, true>(A.mode, A.win != nullptr, A.osr > 1, [&](auto m) {
            constexpr int MODE = decltype(m)::value;
            if constexpr (!(MODE & kOsrBit)) {
                launch_symbols<SF, MODE, demod_occ(SF)>(A, st, per_cu);
            } else if constexpr ((MODE & 3) != LPHY_MODE_DECHIRP_LORA_DEMODULATE) {
                // oversampled input: strided symbol loads (no dechirp mode here)
                launch_symbols<SF, MODE, 2>(A, st, per_cu);
            }
            return 0;
        });
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// Waves per SIMD of k_frames: 2 (<= 256 VGPRs; its loop carries more state
// than k_demod's and spills at 3).
constexpr int kFramesOcc = 2;
// Fused path, k_frames (lphy_frames.h).
template <int SF>
int launch_frames_sf(const DemodArgs& A, hipStream_t st) {
    static_assert(Geo<SF>::LPS == lphy::route_lps(SF), "lphy_route.h's table: Geo<SF>::LPS");
    if constexpr (!lphy::frames_kernel(SF)) {
        (void)A; (void)st;
        return -ENOTSUP;
    } else {
        return with_mode<true, false>(A.mode, A.win != nullptr, false, [&](auto m) {
            constexpr int MODE = decltype(m)::value;
            FrameArgs P{};
            P.A = A;
            constexpr unsigned WPB = kTile / 64;
            const unsigned blocks = persistent_grid(
                resident_blocks<&k_frames<SF, MODE, kFramesOcc>>(current_device()), (A.frames + WPB - 1) / WPB, 0);
            P.waves = blocks * WPB;
            hipLaunchKernelGGL((k_frames<SF, MODE, kFramesOcc>), dim3(blocks), dim3(kTile), 0, st, P);
            HIP_OK(hipGetLastError());
            return 0;
        });
    }
}

// Fused wave-per-symbol path, SF 7-12: k_wave (lphy_wave.h): one wave per
// SIMD, 256-thread workgroups (wave_wpb), the next unit staged through LDS
// by DMA while a unit computes; its units span frames where lphy_route.h's
// wave_spans says so.
template <int SF>
int launch_wave_sf(const DemodArgs& A, hipStream_t st) {
    if constexpr (lphy::route_spw(SF) == 0) {
        (void)A; (void)st;
        return -ENOTSUP;
    } else {
        static_assert(WGeo<SF>::SPW == lphy::route_spw(SF), "lphy_route.h's table: WGeo<SF>::SPW");
        return with_mode<true, false>(A.mode, A.win != nullptr, false, [&](auto m) {
            constexpr int MODE = decltype(m)::value;
            constexpr bool WIN = (MODE & kWinBit) != 0;
            FrameArgs P{};
            P.A = A;
            constexpr int WPB = wave_wpb<SF, MODE>();
            // (a workgroup per CU: one wave per SIMD)
            const unsigned blocks = persistent_grid(device_cus(current_device()), (A.frames + WPB - 1) / WPB, 0);
            P.waves = blocks * WPB;
            if constexpr (lphy::wave_kernel(SF, MODE & 3, WIN, true)) {
                if (lphy::wave_spans(SF, A.total_syms)) {
                    hipLaunchKernelGGL((k_wave<SF, MODE, true>), dim3(blocks), dim3(64 * WPB), 0, st, P);
                    HIP_OK(hipGetLastError());
                    return 0;
                }
            }
            if constexpr (lphy::wave_kernel(SF, MODE & 3, WIN, false)) {
                hipLaunchKernelGGL((k_wave<SF, MODE, false>), dim3(blocks), dim3(64 * WPB), 0, st, P);
                HIP_OK(hipGetLastError());
                return 0;
            } else {
                return -ENOTSUP;
            }
        });
    }
}

// After the symbol kernels: k_spec_settle where the separate launches
// speculated (A.spec_big: SF 11-12, modes 1/2), then k_post.
template <int SF>
int launch_post_sf(int mode, const DemodArgs& A, const FinalArgs& F, bool fix, bool fin, hipStream_t st) {
    return with_mode<false, false>(mode, false, false, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        if constexpr (MODE != LPHY_MODE_DEMODULATE) {
            if (fix && A.spec_big)
                hipLaunchKernelGGL((k_spec_settle<SF, MODE>), dim3((unsigned)A.frames), dim3(kTile), 0, st, A);
        }
        hipLaunchKernelGGL((k_post<SF, MODE>), dim3((unsigned)((A.frames + kTile - 1) / kTile)), dim3(kTile), 0, st, A,
                           F, (int)fix, (int)fin);
        HIP_OK(hipGetLastError());
        return 0;
    });
}

// lphy_hip_demod_ragged (lphy_ragged.h), SF 7-12: prologue, symbols,
// finalisation.  The symbol kernel's persistent grid covers the call's whole
// symbols when the host knows them (units_hint), else the device (the
// workgroups past the last unit leave at once).  grid_cap > 0 (test build,
// lphy_hip_test_grid_cap) caps that grid, so each workgroup walks more tiles.
template <int SF>
int launch_ragged_sf(const RaggedArgs& R, hipStream_t st, unsigned grid_cap) {
    if constexpr (SF < 7) {
        (void)R; (void)st; (void)grid_cap;
        return -ENOTSUP;
    } else {
        using G = Geo<SF>;
        constexpr int FPW = rg_fpw<SF>();
        const unsigned long long frames = R.A.frames;
        hipLaunchKernelGGL(k_rg_prologue<SF>, dim3((unsigned)((frames + FPW - 1) / FPW)), dim3(kTile), 0, st, R);
        with_mode<true, false>(R.A.mode, R.A.win != nullptr, false, [&](auto m) {
            constexpr int MODE = decltype(m)::value;
            const unsigned grid = persistent_grid(resident_blocks<&k_rg_demod<SF, MODE>>(current_device()),
                                                  (R.units_hint + G::T - 1) / G::T, grid_cap);
            hipLaunchKernelGGL((k_rg_demod<SF, MODE>), dim3(grid), dim3(kTile), 0, st, R);
            return 0;
        });
        hipLaunchKernelGGL(k_rg_final<SF>, dim3((unsigned)((frames + kTile - 1) / kTile)), dim3(kTile), 0, st, R);
        HIP_OK(hipGetLastError());
        return 0;
    }
}

// lphy_hip_detect_batch and lphy_hip_detect_ragged (lphy_detect.h), SF 7-12:
// one persistent launch over tiles of Geo<SF>::T units.  The grid covers the
// call's units when the host knows them (the lattice's windows, the table's
// units_hint), else as in launch_ragged_sf; grid_cap as there.
inline unsigned long long det_units_hint(const DetLattice& g) { return g.windows; }
inline unsigned long long det_units_hint(const DetRagged& g) { return g.units_hint; }

template <int SF, class GEO>
int launch_detect_sf(const DetectArgs& D, const GEO& geo, hipStream_t st, unsigned grid_cap) {
    if constexpr (SF < 7) {
        (void)D; (void)geo; (void)st; (void)grid_cap;
        return -ENOTSUP;
    } else {
        with_prep(D.dechirp != 0, D.win != nullptr, [&](auto p) {
            constexpr int PREP = decltype(p)::value;
            constexpr int T = Geo<SF>::T;
            const unsigned grid = persistent_grid(resident_blocks<&k_detect<SF, PREP, GEO>>(current_device()),
                                                  (det_units_hint(geo) + T - 1) / T, grid_cap);
            hipLaunchKernelGGL((k_detect<SF, PREP, GEO>), dim3(grid), dim3(kTile), 0, st, D, geo);
        });
        HIP_OK(hipGetLastError());
        return 0;
    }
}

template <int SF>
int launch_estimate_sf(const DemodArgs& A, hipStream_t st) {
    const int fpt = A.est_units <= Geo<SF>::T ? Geo<SF>::T / A.est_units : 1;
    hipLaunchKernelGGL(k_estimate<SF>, dim3((unsigned)((A.frames + fpt - 1) / fpt)), dim3(kTile), 0, st, A);
    HIP_OK(hipGetLastError());
    return 0;
}

// lphy_hip_estimate_ragged (lphy_ragged.h), SF 7-12: one launch, a workgroup
// per group of rg_fpw frames (k_rg_prologue's grouping).
template <int SF>
int launch_estimate_ragged_sf(const RaggedArgs& R, unsigned long long est_samples, hipStream_t st) {
    if constexpr (SF < 7) {
        (void)R; (void)est_samples; (void)st;
        return -ENOTSUP;
    } else {
        constexpr int FPW = rg_fpw<SF>();
        hipLaunchKernelGGL(k_rg_estimate<SF>, dim3((unsigned)((R.A.frames + FPW - 1) / FPW)), dim3(kTile), 0, st, R,
                           est_samples);
        HIP_OK(hipGetLastError());
        return 0;
    }
}
}  // namespace
