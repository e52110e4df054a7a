// lphy_detect.h — lphy_hip_detect_batch: LoRaDetector<float>::detect
// (LoRaDetector.hpp:39-74) over a batch of windows, all four outputs per
// window (lphy_detect_rec, include/lphy_hip.h).  One launch, k_detect<SF,
// PREP, DetLattice>: a persistent grid over tiles of T windows, one team (the
// LPS lanes of one symbol) per window as in k_rg_demod.  Window w feeds it
// the N samples iq[first + w * hop + i * step], prepared per PREP:
// [x down[i] with the reference's complex product] [x win[i]].
//   stage (Stage<SF>) -> exact KISS transform with the Annex G products
//   (fft_tile<SF, false, true>: non-finite windows need no second run) ->
//   bins back to the team's LDS slot -> argmax (symbol_argmax) -> fIndex
//   (unit_result) -> power (detector_power) -> powerAvg.
//
// powerAvg = 20 log10f(sqrtf((float)(total - maxValue))) - power_scale with
// `total` the double-precision sum of the |X|^2 values in bin order
// (LoRaDetector.hpp:45-60), which no parallel sum reproduces bit for bit.
// The team sums them in double in its own order, S, and certifies the float
// the reference must arrive at, in one of two ways:
//   * exact sums.  Every term is a float, so a multiple of q = ulp(least
//     non-zero term), and so is every partial sum of any subset, which is at
//     most the exact sum E.  When E <= 2^53 q every such partial sum is a
//     double, no addition rounds in any order, and S = E = total.  Tested as
//     S <= 2^52 q: a rounded S is within a relative N 2^-52 of E.  (Noise
//     spreads the bins over a few dozen octaves at most: nearly every noisy
//     window ends here.)
// otherwise by an interval:
//   * any rounded sum of N non-negative terms lies within a relative
//     (N - 1) 2^-53 (to first order) of the exact sum E, so both S and the
//     reference's total do, and total lies in [S (1 - c), S (1 + c)] for
//     c = N 2^-50 = 8 N 2^-53: four times the 2 (N - 1) 2^-53 between the
//     two sums, which also covers the rounding of the bounds themselves;
//   * double subtraction of maxValue and the cast to float are monotone, so
//     (float)(total - maxValue) lies between (float)(S (1 - c) - maxValue)
//     and (float)(S (1 + c) - maxValue): when those two are the same float,
//     it is the reference's value.
// Otherwise (a clean tone, where total - maxValue is pure cancellation; any
// window whose sum is not finite) the team's first lane walks the slot's bins
// in order and restates the reference loop literally; each such window counts
// in the context's kCtrDetectSerial (lphy_hip_detect_serial_count).
//
// lphy_hip_detect_ragged is the same detector on every whole symbol of every
// frame of a lphy_ragged_desc table, and the same kernel: k_detect<SF, PREP,
// GEO> takes the window geometry, DetLattice or DetRagged (once a kernel of
// its own, k_detect_ragged), whose det_unit finds each team's window.  What
// follows per window is one function, detect_window.
#pragma once
#include "lphy_demod.h"
#include "lphy_ragged_layout.h"
#include "lphy_ragged_unit.h"

namespace {

constexpr int kPrepDechirp = 1;  // LPHY_DET_DECHIRP
constexpr int kPrepWindow = 2;   // the context's Hann window

// The detector's loop over the slot's bins, in bin order, by one lane:
// (float)(total - maxValue) of LoRaDetector.hpp:45-60.
template <int SF>
__device__ __attribute__((noinline)) float detect_walk(const cf32* lds, int slot) {
    using G = Geo<SF>;
    float max_value = 0.0f;
    double total = 0.0;
#pragma unroll 8
    for (int i = 0; i < G::N; ++i) {
        const cf32 bin = lds[G::addr(slot, i)];
        const float mag2 = bin.x * bin.x + bin.y * bin.y;
        total += (double)mag2;
        if (mag2 > max_value) max_value = mag2;
    }
    return (float)(total - (double)max_value);
}

// One window of one team, all four outputs: what k_detect does per tile once
// each team knows its window (det_unit).  The team's window is the N samples
// iq[base + i * step]; its record goes to out[w].  A team that is not
// `live` stages zeros and writes nothing.  Every thread of
// the workgroup calls this together (it holds the tile's barriers; the first
// one also publishes the tables the caller loaded into twl / down / win).
// `iq_end` / `out_end`: one past the last sample / record the caller may
// touch (debug build, bound_check).
template <int SF, int PREP>
__device__ __forceinline__ void detect_window(const cf32* iq, unsigned long long base,
                                              unsigned long long step, unsigned long long iq_end, bool live,
                                              lphy_detect_rec* out, unsigned long long w,
                                              unsigned long long out_end, cf32* lds, const cf32* twl,
                                              const cf32* down, const float* win, ArgMax* red, double* reds,
                                              float* redn, const Stage<SF>& stg, int slot, int lam, float power_scale,
                                              unsigned long long* counters) {
    using G = Geo<SF>;
    constexpr int N = G::N;
    constexpr bool DECH = (PREP & kPrepDechirp) != 0, WIN = (PREP & kPrepWindow) != 0;
    constexpr int WPS = G::LPS > 64 ? G::LPS / 64 : 1;  // waves per window
    const int tid = threadIdx.x;
    cf32 raw[16];
#pragma unroll
    for (int e = 0; e < G::E; ++e) {
        raw[e] = czero();
        if (live) {
            const unsigned long long idx = base + (unsigned long long)(lam + e * G::LPS) * step;
            bound_check((long long)idx, (long long)iq_end);
            raw[e] = iq[idx];
        }
    }
    __syncthreads();  // the tables; the previous tile's readers are done with lds
#pragma unroll
    for (int e = 0; e < G::E; ++e) {
        const int i = lam + e * G::LPS;
        cf32 x = raw[e];
        if constexpr (DECH) x = cmul_x(x, down[i]);  // e2e_chain_test.cpp:88-93
        if constexpr (WIN) x = cscale(x, win[i]);    // LoRaDemod.cpp:96-97
        stg.put(lds, e, x);
    }
    __syncthreads();
    cf32 v[16];
    fft_tile<SF, false, true>(v, lds, slot, lam, twl);
    // keep the bins for the interpolation and the in-order walk; the
    // lane's share of the sum of |X|^2 (the values local_argmax takes)
    // ... and its least non-zero one (NaN never taken)
    double sum = 0.0;
    float least = __builtin_inff();
#pragma unroll
    for (int e = 0; e < G::E; ++e) {
        lds[G::addr(slot, bin_of<SF>(e, lam))] = v[e];
        const cf32 sq = v[e] * v[e];
        const float m2 = sq.x + sq.y;
        sum += (double)m2;
        least = (m2 > 0.0f && m2 < least) ? m2 : least;
    }
#pragma unroll
    for (int off = (G::LPS < 64 ? G::LPS : 64) / 2; off >= 1; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        least = fminf(least, __shfl_xor(least, off, 64));
    }
    if constexpr (WPS > 1) {
        // (visible behind symbol_argmax's first barrier, reused behind
        // the next tile's)
        if ((tid & 63) == 0) {
            reds[tid >> 6] = sum;
            redn[tid >> 6] = least;
        }
    }
    const ArgMax best = symbol_argmax<SF>(local_argmax<SF>(v, lam), red);
    if constexpr (WPS > 1) {
        const int fw = ((tid >> 6) / WPS) * WPS;
        sum = reds[fw];
        least = redn[fw];
#pragma unroll
        for (int k = 1; k < WPS; ++k) {
            sum += reds[fw + k];
            least = fminf(least, redn[fw + k]);
        }
    }
    __syncthreads();  // every bin of the slot written
    if (lam == 0 && live) {
        const UnitResult r = unit_result<SF>(lds, slot, best);
        const float mv = best.v > 0.0f ? best.v : 0.0f;
        const double c = (double)N * 0x1p-50;
        const float lo = (float)(sum * (1.0 - c) - (double)mv);
        const float hi = (float)(sum * (1.0 + c) - (double)mv);
        // 2^52 ulp(least): ulp = 2^(e - 150) for the biased exponent e (1
        // for a denormal); a double's exponent field directly
        const int le = (int)(__float_as_uint(least) >> 23);
        const double lim = __longlong_as_double((long long)((le ? le : 1) - 98 + 1023) << 52);
        float rest = lo;
        if (sum < __builtin_inf() && least < __builtin_inff() && sum <= lim) {
            rest = (float)(sum - (double)mv);  // S is the reference's total
        } else if (!(sum < __builtin_inf() && __float_as_uint(lo) == __float_as_uint(hi))) {
            rest = detect_walk<SF>(lds, slot);
            atomicAdd(&counters[kCtrDetectSerial], 1ull);
        }
        lphy_detect_rec o;
        o.power = detector_power(mv, power_scale);
        o.power_avg = detector_power(rest, power_scale);  // 20 log10f(sqrtf(.)) - scale
        o.findex = r.findex;
        o.index = (uint16_t)r.idx;
        o.reserved = 0;
        bound_check((long long)w, (long long)out_end);
        out[w] = o;
    }
}

// The window geometries (lphy_args.h): the units of a call, and unit u's
// first sample, sample stride, end of its IQ (debug build) and record index.
struct DetUnit {
    unsigned long long base, step, iq_end, rec;
    bool live;
};

__device__ __forceinline__ unsigned long long det_units(const DetLattice& g) { return g.windows; }
__device__ __forceinline__ unsigned long long det_units(const DetRagged& g) { return g.desc[g.frames].unit_offset; }

// window u of the lattice: iq[first + u * hop + i * step], record out[u]
template <int SF>
__device__ __forceinline__ DetUnit det_unit(const DetLattice& g, unsigned long long, unsigned long long u) {
    const bool live = u < g.windows;
    return DetUnit{g.first + (live ? u : 0) * g.hop, g.step, g.total_samples, u, live};
}

// unit u of the table, the global symbol index as in k_rg_demod: symbol s of
// its frame (ragged_unit; from SF 10 on wave-uniform values) is the window
// iq[iq_offset + s N osr + phase + i osr], whose record is out[u]
template <int SF>
__device__ __forceinline__ DetUnit det_unit(const DetRagged& g, unsigned long long units, unsigned long long u) {
    const RaggedUnit ru = ragged_unit<Geo<SF>::LPS >= 64>(g.desc, g.frames, units, u);
    // whole symbols of the frame (samples < 2^31 where it counts)
    const unsigned n = ((unsigned)ru.d.samples >> SF) / g.osr;
    const bool live = ru.live && ru.d.samples < kRaggedMaxSamples && ru.s < n;
    const unsigned long long fstep = (unsigned long long)Geo<SF>::N * g.osr;
    return DetUnit{ru.d.iq_offset + (live ? ru.s : 0) * fstep + g.phase, g.osr, ru.d.iq_offset + n * fstep,
                   ru.d.unit_offset + ru.s, live};
}

// A persistent grid over tiles of T units, one team per unit; the workgroups
// past the last unit leave at once.  Two waves per SIMD up to SF 10, one above.
template <int SF, int PREP, class GEO>
__global__ __launch_bounds__(kTile, SF <= 10 ? 2 : 1) void k_detect(DetectArgs D, GEO geo) {
    using G = Geo<SF>;
    constexpr int N = G::N, T = G::T;
    constexpr bool DECH = (PREP & kPrepDechirp) != 0, WIN = (PREP & kPrepWindow) != 0;
    constexpr bool TAB = N <= 1024;  // chirp + window tables in LDS
    __shared__ cf32 lds[T * G::SSTRIDE];
    __shared__ cf32 twl[N];
    __shared__ cf32 dnl[TAB && DECH ? N : 1];
    __shared__ float wnl[TAB && WIN ? N : 1];
    __shared__ ArgMax red[kTile / 64];
    __shared__ double reds[kTile / 64];
    __shared__ float redn[kTile / 64];

    const unsigned long long units = det_units(geo);
    if ((unsigned long long)blockIdx.x * T >= units) return;  // uniform

    load_tables<N, TAB && DECH, TAB && WIN>(D, twl, dnl, wnl);
    const cf32* down = TAB && DECH ? dnl : D.down;
    const float* win = TAB && WIN ? wnl : D.win;

    const int tid = threadIdx.x;
    const int slot = tid / G::LPS, lam = tid % G::LPS;
    const Stage<SF> stg(slot, lam);
    const unsigned long long stride = (unsigned long long)gridDim.x * T;
    for (unsigned long long t0 = (unsigned long long)blockIdx.x * T; t0 < units; t0 += stride) {
        const DetUnit w = det_unit<SF>(geo, units, t0 + (unsigned)slot);
        detect_window<SF, PREP>(D.iq, w.base, w.step, w.iq_end, w.live, D.out, w.rec, units, lds, twl, down, win, red,
                                reds, redn, stg, slot, lam, D.power_scale, D.counters);
    }
}

}  // namespace
