// lphy_route.h — which kernels a lphy_hip_demod_batch call runs on, decided
// here alone: lphy_hip.hip asks route() once per call, and the per-SF launch
// templates (lphy_launch.h) instantiate exactly the kernels frames_kernel() /
// wave_kernel() name.  Host-only, no HIP dependency
// (tests/cpp/route_check.cpp runs it over the whole grid of shapes).
#pragma once

#include <cstddef>

#include "../../include/lphy_hip.h"
#include "lphy_testing.h"

namespace lphy {

constexpr unsigned kWaveMinSf = 7;  // smallest SF on k_wave
constexpr int kSpanMinSpw = 4;      // fewest symbols per k_wave unit for units spanning frames

// Separate: k_maxabs / k_estimate / k_demod, one launch each; Frames:
// k_frames; Wave: k_wave, its units spanning frames or not (wave_spans)
enum class Path { Separate, Frames, Wave };

// The kernels' geometry by SF: lanes per symbol of the 256-thread tile
// (Geo<SF>::LPS) and symbols per k_wave unit (WGeo<SF>::SPW; 0: no k_wave at
// this SF).  lphy_launch.h static_asserts both against the kernels' own.
constexpr int kRouteLps[13] = {0, 1, 1, 1, 1, 2, 4, 8, 16, 32, 64, 128, 256};
constexpr int kRouteSpw[13] = {0, 0, 0, 0, 0, 0, 0, 32, 16, 8, 4, 2, 1};
constexpr int route_lps(unsigned sf) { return sf <= 12 ? kRouteLps[sf] : 0; }
constexpr int route_spw(unsigned sf) { return sf <= 12 ? kRouteSpw[sf] : 0; }

// k_frames<SF, ...> exists: a symbol's lanes within one wavefront (SF <= 10)
constexpr bool frames_kernel(unsigned sf) { return route_lps(sf) >= 1 && route_lps(sf) <= 64; }
// k_wave's units span frames (WSchedSpan, SF 7-10) when a frame holds at
// least one unit of symbols
constexpr bool wave_spans(unsigned sf, size_t total_syms) {
    return route_spw(sf) >= kSpanMinSpw && total_syms >= (size_t)route_spw(sf);
}
// k_wave<SF, mode [| kWinBit], span> exists.  Not spanning: SF 9-12 only
// (below, k_frames was 1.5x faster on frames shorter than a unit), and not
// SF 12 mode 1 with the Hann window (it spilled 212 B per lane).
constexpr bool wave_kernel(unsigned sf, int mode, bool window, bool span) {
    if (span) return route_spw(sf) >= kSpanMinSpw;
    return route_spw(sf) != 0 && sf >= 9 && !(sf == 12 && window && mode == LPHY_MODE_LORA_DEMODULATE);
}

struct RouteArgs {
    unsigned sf, osr;
    int mode;
    bool window;
    size_t total_syms;  // whole symbols per frame
    int est_units;      // estimate units per frame (est_syms * osr)
    size_t frames, fused_min;  // the batch; the smallest the fused kernels take (fused_min_frames)
    bool spec;          // modes 1/2: the speculative normalisation (DemodArgs::spec)
    bool exact_rotation;
    unsigned flags;     // the call's: LPHY_F_STAGE_*, LPHY_F_UNFUSED, LPHY_F_FRAMES_KERNEL
};

inline Path route(const RouteArgs& r) {
    // one fused launch covers prologue + symbols: every stage, or at least
    // those two, selected; both fused kernels: osr 1, the two-symbol estimate
    const unsigned both = LPHY_F_STAGE_PROLOGUE | LPHY_F_STAGE_SYMBOLS;
    const unsigned stages = r.flags & (both | LPHY_F_STAGE_FINAL);
    if ((stages != 0 && (stages & both) != both) || (r.flags & LPHY_F_UNFUSED) || r.frames < r.fused_min ||
        r.osr != 1 || r.est_units != 2 || r.total_syms < 2)
        return Path::Separate;
    // k_wave: the certified rotation, in modes 1/2 the speculative
    // normalisation; LPHY_F_FRAMES_KERNEL (test build) keeps k_frames
    if (r.sf >= kWaveMinSf && !(r.flags & LPHY_F_FRAMES_KERNEL) && !r.exact_rotation &&
        (r.mode == LPHY_MODE_DEMODULATE || r.spec) &&
        wave_kernel(r.sf, r.mode, r.window, wave_spans(r.sf, r.total_syms)))
        return Path::Wave;
    // k_frames: frames long enough that a frame's estimate tile precedes its
    // first symbol tile by two tiles (S + 1 >= 2 * units per tile)
    if (frames_kernel(r.sf) && r.total_syms + 1 >= 2 * (size_t)(64 / route_lps(r.sf))) return Path::Frames;
    return Path::Separate;
}

}  // namespace lphy
