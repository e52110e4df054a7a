// lphy_demod.h — the separate-launch demodulator: per frame k_maxabs<SF>
// (modes 1/2, LoRaDemod.cpp:60-78) and k_estimate<SF> (LoRaDemod.cpp:80-136 /
// phy.cpp:81-148), then k_demod<SF>: per symbol CFO rotation -> KISS-
// identical FFT (lphy_fft.h) -> |X|^2 argmax (LoRaDemod.cpp:142-176 /
// phy.cpp:204-238).  Also the symbol machinery the other demodulator kernels
// share (lphy_frames.h, lphy_post.h, lphy_wave.h): SymCtx, rotate_sample,
// the staging, UnitResult, EstFold, the certificate; and the exact passes of
// the paths that reproduce the reference's arithmetic plainly (k_maxabs,
// k_estimate, lphy_post.h, lphy_ragged.h): workgroup_max, estimate_unit,
// exact_symbol, settle_verdict, and load_tables (the call's tables into LDS).
#pragma once
#include "lphy_args.h"
#include "libm_exact.h"
#include "lphy_testing.h"  // (the device counter slots)

namespace {

// (int)std::round(x) as the x86-64 reference evaluates it: cvttss2si on the
// rounded value, INT_MIN for NaN / out of range.
__device__ __forceinline__ int round_to_int(float x) {
    const float r = roundf(x);
    if (!(r >= -2147483648.0f && r < 2147483648.0f)) return (int)0x80000000u;
    return (int)r;
}

// Input sample for the estimate (no rotation): raw (mode 0) or
// [dechirped,] [normalised] (modes 1, 2).  idx is the absolute sample index
// in the frame, i the index inside the symbol (window / mode-0 chirp).
__device__ __forceinline__ cf32 est_sample(const DemodArgs& A, const cf32* fr,
                                             unsigned long long idx, int i, int N,
                                             const lphy_frame_meta& m) {
    cf32 x = fr[idx];
    if (A.mode == LPHY_MODE_DECHIRP_LORA_DEMODULATE)
        x = idx < A.total_syms * (unsigned long long)N ? cmul_x(x, A.down[idx & (N - 1)])
                                                       : czero();
    if (A.mode != LPHY_MODE_DEMODULATE && m.normalised) x = cscale(x, m.scale);
    if (A.win) x = cscale(x, A.win[i]);
    return x;
}

// The call's N twiddles (A.tw) and, where the kernel keeps them in LDS, its
// down-chirp (DOWN: A.down) and window (WIN: A.win) into the workgroup's
// arrays, by all kTile threads.  No barrier: the caller's next one publishes
// them.
template <int N, bool DOWN, bool WIN, class ARGS>
__device__ __forceinline__ void load_tables(const ARGS& A, cf32* twl, cf32* dnl = nullptr, float* wnl = nullptr) {
    for (int i = threadIdx.x; i < N; i += kTile) {
        twl[i] = A.tw[i];
        if constexpr (DOWN) dnl[i] = A.down[i];
        if constexpr (WIN) wnl[i] = A.win[i];
    }
}

// max(|I|,|Q|) accumulation of LoRaDemod.cpp:62-66 for one sample:
// std::max(r, im) keeps r when im is NaN and yields NaN (never > mx) when r
// is NaN, so a NaN real part hides the whole sample.
__device__ __forceinline__ void maxabs_acc(float& mx, cf32 x) {
    const float r = fabsf(x.x), im = fabsf(x.y);
    const float m = (r < im) ? im : r;
    if (m > mx) mx = m;
}

// The workgroup's maximum of every lane's mx (order-free), through
// wmax[kTile / 64].  One barrier: the whole workgroup calls it, and another
// barrier stands before wmax is written again.
__device__ __forceinline__ float workgroup_max(float mx, float* wmax) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = wmax[0];
#pragma unroll
    for (int w = 1; w < kTile / 64; ++w) mx = wmax[w] > mx ? wmax[w] : mx;
    return mx;
}

// Normalisation decision of LoRaDemod.cpp:60-78 from the frame's max-abs.
__device__ __forceinline__ lphy_frame_meta norm_meta(float mx, bool have_sync, int no_scratch) {
    lphy_frame_meta m{};
    m.scale = 1.0f;
    m.have_sync = have_sync;
    if (mx > 1.0f) {
        if (no_scratch) m.status = -ERANGE;  // LoRaDemod.cpp:69-71
        m.normalised = 1;
        m.scale = 1.0f / mx;
    }
    return m;
}
// The same in the hot kernels, whose scans return NaN for a frame with a
// non-finite sample: that frame goes to the exact re-run.
__device__ __forceinline__ lphy_frame_meta norm_meta_hot(float mx, bool have_sync, int no_scratch) {
    lphy_frame_meta m = norm_meta(mx, have_sync, no_scratch);
    if (!(mx <= 3.40282347e38f)) m.status = kStatusFixup;
    return m;
}

// ---------------------------------------------------------------------------
// Stage 1a (modes 1, 2): per-frame max(|I|,|Q|) of the [dechirped] frame and
// the normalisation decision (LoRaDemod.cpp:60-78).  A pure streaming
// reduction: one workgroup per frame, 16-byte loads, 8 in flight per lane.
// ---------------------------------------------------------------------------
template <int SF>
__global__ __launch_bounds__(kTile) void k_maxabs(DemodArgs A) {
    constexpr int N = 1 << SF;
    __shared__ float wmax[kTile / 64];
    const unsigned long long f = blockIdx.x;
    const int tid = threadIdx.x;
    const cf32* fr = A.iq + f * A.frame_samples;
    // spec_big: the two estimate symbols only (the symbols fold the rest)
    const unsigned long long count = A.spec_big ? 2ull * N : A.frame_samples;
    const unsigned long long dech_end = A.total_syms * N;  // whole symbols
    const bool dech = A.mode == LPHY_MODE_DECHIRP_LORA_DEMODULATE;
    float mx = 0.0f;
    bool bad = false;  // a non-finite [dechirped] sample: exact re-run (k_post)
    auto acc = [&](cf32 x, unsigned long long i) {
        if (dech) x = i < dech_end ? cmul(x, A.down[i & (N - 1)]) : czero();
        bad |= !(__builtin_isfinite(x.x) && __builtin_isfinite(x.y));
        maxabs_acc(mx, x);
    };
    if ((reinterpret_cast<uintptr_t>(fr) & 15) == 0) {
        const float4* f4 = reinterpret_cast<const float4*>(fr);
        const unsigned long long n4 = count / 2;
        constexpr int U = 8;
        unsigned long long j = tid;
        for (; j + (U - 1) * kTile < n4; j += U * kTile) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = f4[j + u * kTile];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned long long i = 2 * (j + u * kTile);
                acc(cf32{v[u].x, v[u].y}, i);
                acc(cf32{v[u].z, v[u].w}, i + 1);
            }
        }
        for (; j < n4; j += kTile) {
            const float4 v = f4[j];
            acc(cf32{v.x, v.y}, 2 * j);
            acc(cf32{v.z, v.w}, 2 * j + 1);
        }
        if ((count & 1) && tid == 0) acc(fr[count - 1], count - 1);
    } else {
        for (unsigned long long i = tid; i < count; i += kTile) acc(fr[i], i);
    }
    // a wave that met a non-finite sample enters NaN, which its wmax entry
    // keeps (a NaN loses every comparison of the maximum)
    if (__ballot(bad)) mx = __builtin_nanf("");
    mx = workgroup_max(mx, wmax);
    if (tid == 0) {
        bool nf = false;
#pragma unroll
        for (int w = 0; w < kTile / 64; ++w) nf |= !(wmax[w] == wmax[w]);
        A.meta[f] = norm_meta_hot(nf ? __builtin_nanf("") : mx, A.total_syms >= 2, A.no_scratch);
        if (A.spec_big) A.spec_big[f] = make_uint4(__float_as_uint(nf ? 0.0f : mx), 0u, 0x7f7fffffu, nf ? 1u : 0u);
    }
}

// ---------------------------------------------------------------------------
// Stage 1b: offset estimate (LoRaDemod.cpp:80-140 / phy.cpp:81-148).
// Units = (symbol, osr phase) FFTs; a 256-thread tile packs T units, i.e.
// T/U whole frames when a frame has U <= T units (8 frames per workgroup at
// SF7), otherwise loops over one frame's units.  Per frame, one thread folds
// the unit results in symbol order exactly like the reference loop.
// ---------------------------------------------------------------------------
struct UnitResult {
    int idx;
    int valid;   // p > best_p reachable (maxValue > 0)
    float findex;
    float phase;
    int nan;     // a NaN bin (k_frames: the frame goes to the exact re-run)
};
// a unit without a symbol (the tail of a tile); an unset best bin is (0, 0),
// whose atan2 is 0
constexpr UnitResult kNoUnit{0, 0, 0.0f, 0.0f, 0};

// Detector outputs of one estimate unit from its FFT bins, which the team
// has written back to its LDS slot (LoRaDetector.hpp:60-71).
template <int SF>
__device__ __forceinline__ UnitResult unit_result(const cf32* lds, int slot, ArgMax best) {
    using G = Geo<SF>;
    constexpr int N = G::N;
    UnitResult r;
    const int idx = best.i;
    const float mv = best.v > 0.0f ? best.v : 0.0f;
    const float fund = sqrtf(mv);
    const cf32 lb = lds[G::addr(slot, idx > 0 ? idx - 1 : N - 1)];
    const cf32 rb = lds[G::addr(slot, idx < N - 1 ? idx + 1 : 0)];
    const float left = lphy_libm::cabsf_exact(lb.x, lb.y);
    const float right = lphy_libm::cabsf_exact(rb.x, rb.y);
    const double demon = (2.0 * (double)fund) - (double)right - (double)left;
    const float fi = demon == 0.0 ? 0.0f : (float)(0.5 * (double)(right - left) / demon);
    const cf32 bin = lds[G::addr(slot, idx)];
    r.idx = idx;
    r.valid = mv > 0.0f;  // osr == 1: p > -1e30 <=> maxValue > 0
    r.findex = fi;
    r.phase = lphy_libm::atan2f_exact(bin.y, bin.x);
    r.nan = 0;
    return r;
}

// Detector power of LoRaDetector.hpp:64, 20*log10(sqrt(maxValue)) - scale in
// single precision with glibc's log10f.  Only the osr > 1 estimate compares
// powers (with one phase, p > -1e30 <=> maxValue > 0).
__device__ __forceinline__ float detector_power(float max_value, float power_scale) {
    const float fund = sqrtf(max_value);
    const float db = 20.0f * lphy_libm::log10f_exact(fund);
    return db - power_scale;
}

// One estimate unit per team, in the reference's arithmetic
// (LoRaDemod.cpp:86-92): osr phase t of estimate symbol s of the frame at fr,
// whose element i is sample (s N + i) osr + t (the reference's sym[t + i osr]),
// staged through est_sample in natural order; the exact FFT;
// the bins written back to the team's slot for the interpolation and the
// phase; the argmax, which it returns: the team's lane 0 then takes the
// detector outputs from the slot (unit_result; kNoUnit when not live; the
// osr > 1 power from the winner's |X|^2).  Holds the two barriers between
// staging and the result, so the whole workgroup calls it; the barriers before
// (the slot's previous readers) and after (the result's readers) are the
// caller's.  (The same pass stands written out in exact_frame and
// settle_frames, lphy_post.h, and in k_rg_prologue, lphy_ragged.h, where the
// helper cost registers: change those with it.)
template <int SF>
__device__ __forceinline__ ArgMax estimate_unit(const DemodArgs& A, const cf32* fr, int s, int t, int osr,
                                                const lphy_frame_meta& m, bool live, cf32* lds,
                                                int slot, int lam, const cf32* tw, ArgMax* red) {
    using G = Geo<SF>;
    const Stage<SF> st(slot, lam);
#pragma unroll
    for (int e = 0; e < G::E; ++e) {
        const int i = lam + e * G::LPS;
        cf32 x = czero();
        if (live) x = est_sample(A, fr, ((unsigned long long)s * G::N + (unsigned)i) * osr + t, i, G::N, m);
        st.put(lds, e, x);
    }
    __syncthreads();
    cf32 v[16];
    fft_tile<SF, false, true>(v, lds, slot, lam, tw);
#pragma unroll
    for (int e = 0; e < G::E; ++e) lds[G::addr(slot, bin_of<SF>(e, lam))] = v[e];
    const ArgMax best = symbol_argmax<SF>(local_argmax<SF>(v, lam), red);
    __syncthreads();
    return best;
}

// Running fold of the per-symbol estimates in symbol order
// (LoRaDemod.cpp:95-128 / phy.cpp:95-135).
struct EstFold {
    float sum_index = 0.0f, phase_diff = 0.0f, prev_phase = 0.0f;
    bool have_prev = false;
    unsigned sum_t = 0;
    __device__ __forceinline__ void add(int best_idx, float best_f, int best_t, float best_phase) {
        sum_t += (unsigned)best_t;
        sum_index += (float)best_idx + best_f;
        if (have_prev) {
            float d = best_phase - prev_phase;
            while (d > kPi) d -= 2.0f * kPi;
            while (d < -kPi) d += 2.0f * kPi;
            phase_diff += d;
        }
        prev_phase = best_phase;
        have_prev = true;
    }
    // per-phase selection over the osr phases of one symbol
    // (LoRaDemod.cpp:93-113 with the lowest-index tie-break, phy.cpp:106-121
    // without it); units arrive in (symbol, phase) order
    float best_p = -1e30f, best_f = 0.0f, best_phase = 0.0f;
    int best_idx = 0, best_t = 0, t = 0;
    __device__ __forceinline__ void unit(const UnitResult& r, float p, int osr, bool tie_low) {
        if (r.valid && (p > best_p || (tie_low && p == best_p && r.idx < best_idx))) {
            best_p = p; best_idx = r.idx; best_f = r.findex; best_t = t; best_phase = r.phase;
        }
        if (++t == osr) {
            add(best_idx, best_f, best_t, best_phase);
            best_p = -1e30f; best_f = 0.0f; best_phase = 0.0f;
            best_idx = 0; best_t = 0; t = 0;
        }
    }
    // offsets of LoRaDemod.cpp:130-140 / phy.cpp:137-147 into m
    __device__ __forceinline__ void finish(lphy_frame_meta& m, int est_syms, int N, int osr) const {
        const float avg_index = sum_index / (float)est_syms;
        const float cfo_coarse = avg_index / (float)N;
        float cfo_fine = 0.0f;
        if (est_syms > 1)
            cfo_fine = (phase_diff / (float)(est_syms - 1)) / (2.0f * kPi * (float)N);
        m.cfo = cfo_coarse + cfo_fine;
        const float frac = avg_index - floorf(avg_index + 0.5f);
        const float avg_t = (float)sum_t / (float)est_syms;
        m.time_offset = avg_t - frac * (float)N * (float)osr;
        m.t_off = round_to_int(m.time_offset);
        m.rate = -2.0f * kPi * m.cfo / (float)N;
    }
};

template <int SF>
__global__ __launch_bounds__(kTile) void k_estimate(DemodArgs A) {
    using G = Geo<SF>;
    constexpr int N = G::N, T = G::T;
    __shared__ cf32 lds[T * G::SSTRIDE];
    __shared__ cf32 twl[N];
    __shared__ ArgMax red[kTile / 64];
    __shared__ UnitResult units[T];
    __shared__ float upow[T];

    const int tid = threadIdx.x;
    const int U = A.est_units;
    const bool packed = U <= T;
    const int FPT = packed ? T / U : 1;
    const unsigned long long fbase = (unsigned long long)blockIdx.x * FPT;
    for (int i = tid; i < N; i += kTile) twl[i] = A.tw[i];

    // fold state of frame (fbase + tid), held by thread tid < FPT
    EstFold fold;
    lphy_frame_meta mine{};
    const bool folder = tid < FPT && fbase + tid < A.frames;
    if (folder) {
        if (A.mode == LPHY_MODE_DEMODULATE) {
            mine.scale = 1.0f;
            mine.have_sync = A.total_syms >= 2;
        } else {
            mine = A.meta[fbase + tid];
        }
    }

    const int slot = tid / G::LPS, lam = tid % G::LPS;
    const int chunks = packed ? 1 : (U + T - 1) / T;
    for (int c = 0; c < chunks; ++c) {
        int fl, u;
        if (packed) { fl = slot / U; u = slot % U; }
        else        { fl = 0; u = c * T + slot; }
        const unsigned long long f = fbase + fl;
        bool live = (packed ? fl < FPT : u < U) && f < A.frames;
        lphy_frame_meta m{};
        if (live) {
            if (A.mode == LPHY_MODE_DEMODULATE) m.scale = 1.0f;
            else m = A.meta[f];
            live = m.status == 0;
        }
        const int s = live ? u / A.osr : 0, t = live ? u % A.osr : 0;
        const cf32* fr = A.iq + f * A.frame_samples;
        __syncthreads();  // previous chunk's readers are done with lds / units
        // the samples sym[t + i*osr] of symbol s
        const ArgMax best = estimate_unit<SF>(A, fr, s, t, A.osr, m, live, lds, slot, lam, twl, red);
        if (lam == 0) {
            units[slot] = live ? unit_result<SF>(lds, slot, best) : kNoUnit;
            if (A.osr > 1)
                upow[slot] = live ? detector_power(best.v > 0.0f ? best.v : 0.0f, A.power_scale) : 0.0f;
        }
        __syncthreads();
        if (folder) {
            const int first = packed ? tid * U : 0;
            const int nu = packed ? U : ((U - c * T) < T ? (U - c * T) : T);
            const bool tie_low = A.mode != LPHY_MODE_DEMODULATE;
            for (int k = 0; k < nu; ++k)
                fold.unit(units[first + k], A.osr > 1 ? upow[first + k] : 0.0f, A.osr, tie_low);
        }
    }

    if (folder && mine.status == 0) {
        lphy_frame_meta m = mine;
        fold.finish(m, U / A.osr, N, A.osr);
        A.meta[fbase + tid] = m;
    }
}

// ---------------------------------------------------------------------------
// Stage 2: per-symbol demodulation.  Persistent grid; each 256-thread
// workgroup stages the twiddles (and, up to N = 1024, the down-chirp and the
// window) in LDS once, then loops over tiles of T symbols.
// ---------------------------------------------------------------------------
// Per-tile context of the symbol a team (LPS lanes) works on.  Frame and
// symbol indices are 32-bit (lphy_hip_demod_batch checks frames*symbols and
// frame_samples fit) and advance incrementally: no division per tile.
struct SymCtx {
    unsigned f, s;            // frame, symbol within the frame
    unsigned base;            // first sample of the (shifted) window in the frame
    float start, rate, scale;
    int toff;                 // the frame's t_off (fast-rotation table offset)
    bool ok, have_sync, live;
};

template <bool OSR = false>
__device__ __forceinline__ SymCtx sym_ctx(const DemodArgs& A, unsigned f, unsigned s, bool live,
                                          int N, const lphy_frame_meta& m) {
    SymCtx c;
    c.f = f;
    c.s = s;
    // kStatusRecheck only marks that some symbol of the frame left a
    // sentinel for k_post (another team or workgroup may set it while this
    // symbol's record is read): its estimate stands, and k_post recomputes
    // the sentinels only, so every other symbol must still be demodulated
    c.ok = live && (m.status == 0 || m.status == kStatusRecheck);
    c.live = live;
    c.have_sync = m.have_sync != 0;
    // LoRaDemod.cpp:144-151 / phy.cpp:208-216, in 32 bits
    const unsigned osr = OSR ? (unsigned)A.osr : 1u;
    const unsigned step = (unsigned)N * osr, count = (unsigned)A.frame_samples;
    unsigned base = s * step;
    const int t = m.t_off;
    // all in 32 bits without overflow: count < 2^31 (lphy_hip_demod_batch),
    // base + step <= count for a symbol of the frame, |INT_MIN| = 2^31
    if (t > 0) {
        if (base + step <= count && (unsigned)t <= count - step - base) base += (unsigned)t;
    } else if (t < 0) {
        const unsigned off = 0u - (unsigned)t;
        if (off <= base) base -= off;
    }
    c.base = base;
    c.rate = m.rate;
    c.scale = m.scale;
    c.toff = m.t_off;
    // LoRaDemod.cpp:152-153 / phy.cpp:217-218; (float) of the size_t product
    // equals (float) of the same value held in 32 bits; x / 1.0f == x
    const float toff = OSR ? (float)m.t_off / (float)osr : (float)m.t_off;
    c.start = m.rate * ((float)(s * (unsigned)N) + toff);
    return c;
}

// One rotated input sample (LoRaDemod.cpp:152-163, phy.cpp:217-229).
template <int SF, int MODE, bool AG = false>
__device__ __forceinline__ cf32 rotate_sample(cf32 x, int i, const SymCtx& c,
                                              const cf32* down, const float* win, bool large) {
    constexpr int N = 1 << SF;
    if constexpr ((MODE & 3) == LPHY_MODE_DEMODULATE) {
        x = cmul_t<AG>(x, down[i]);  // phy.cpp:219-220: down-chirp of the window
    } else {
        if constexpr ((MODE & 3) == LPHY_MODE_DECHIRP_LORA_DEMODULATE) {
            // the external dechirp ran on the unshifted buffer
            // (e2e_chain_test.cpp:88-93): chirp index of the absolute sample
            // (frames hold whole symbols in this mode)
            x = cmul_t<AG>(x, down[((unsigned)c.base + (unsigned)i) & (N - 1)]);
        }
        // LoRaDemod.cpp:74-76; scale == 1.0f exactly when no rescale was
        // needed and x * 1.0f == x, so the multiply is unconditional
        x = cscale(x, c.scale);
    }
    const float ph = c.start + c.rate * (float)i;
    float sn, cs;
    if (large) lphy_libm::sincosf_large(ph, &sn, &cs);
    else lphy_libm::sincosf_fast(ph, &sn, &cs);
    x = cmul_t<AG>(x, cf32{cs, sn});
    if constexpr ((MODE & kWinBit) != 0) x = cscale(x, win[i]);
    return x;
}

// Exact restaging of the team's symbol from its IQ in memory, one sample at
// a time (rare paths: the certificate's re-check, and the Annex G re-run of
// a transform that produced a NaN bin).
template <int SF, int MODE, bool AG>
__device__ __forceinline__ void restage_symbol(cf32* lds, const Stage<SF>& stg, const cf32* src,
                                               const SymCtx& c, int lam, const cf32* down,
                                               const float* win, unsigned osr = 1) {
    using G = Geo<SF>;
    // the lane's samples loaded first, all in flight together (one memory
    // round trip for the symbol: k_post re-runs run at low occupancy, where
    // a load per sincos cost a round trip each - mode A's ~6,600 re-runs at
    // SF 7 took 43 us)
    cf32 raw[G::E];
#pragma unroll
    for (int e = 0; e < G::E; ++e) raw[e] = src[(unsigned)(lam + e * G::LPS) * osr];
#pragma unroll
    for (int e = 0; e < G::E; ++e) {
        const int i = lam + e * G::LPS;
        const float ph = c.start + c.rate * (float)i;
        stg.put(lds, e, rotate_sample<SF, MODE, AG>(raw[e], i, c, down, win, lphy_libm::sincosf_needs_large(ph)));
    }
}

// The team's symbol c of the frame at fr in the reference's arithmetic
// (k_post's re-runs): restage_symbol with its Annex G products and the
// call's window, the exact FFT, the argmax.  Holds the barrier between the
// two, so the whole workgroup calls it; the barrier after the caller's store
// (before the slot is staged again) is the caller's.
template <int SF, int MODE>
__device__ __forceinline__ ArgMax exact_symbol(const DemodArgs& A, const cf32* fr, const SymCtx& c,
                                               cf32* lds, int slot, int lam, ArgMax* red) {
    if (A.win)
        restage_symbol<SF, MODE | kWinBit, true>(lds, Stage<SF>(slot, lam), fr + c.base, c, lam,
                                                 A.down, A.win, (unsigned)A.osr);
    else
        restage_symbol<SF, MODE, true>(lds, Stage<SF>(slot, lam), fr + c.base, c, lam,
                                       A.down, nullptr, (unsigned)A.osr);
    __syncthreads();
    cf32 v[16];
    fft_tile<SF, false, true>(v, lds, slot, lam, A.tw);
    return symbol_argmax<SF>(local_argmax<SF>(v, lam), red);
}

// Stage the team's symbol (rotated, natural order) into its LDS slot.
template <int SF, int MODE>
__device__ __forceinline__ void stage_symbol(cf32* lds, const Stage<SF>& stg, const cf32 (&raw)[16],
                                             const cf32* src, const SymCtx& c, int lam,
                                             const cf32* down, const float* win, int osr = 1) {
    using G = Geo<SF>;
#pragma unroll
    for (int e = 0; e < G::E; ++e)
        stg.put(lds, e, rotate_sample<SF, MODE>(raw[e], lam + e * G::LPS, c, down, win, false));
    // rare: |phase| >= 120 rad (large CFO x long frame).  The angle is
    // monotone in i, so the lane's first and last samples bound it.
    if (lphy_libm::sincosf_needs_large(c.start + c.rate * (float)lam) ||
        lphy_libm::sincosf_needs_large(c.start + c.rate * (float)(lam + (G::E - 1) * G::LPS))) {
        for (int e = 0; e < G::E; ++e) {
            const int i = lam + e * G::LPS;
            if (lphy_libm::sincosf_needs_large(c.start + c.rate * (float)i))
                stg.put(lds, e, rotate_sample<SF, MODE>(src[(unsigned)i * (unsigned)osr], i, c, down, win, true));
        }
    }
}

// debug build: sample `off` of frame `f` lies inside the batch (bound_check)
__device__ __forceinline__ void iq_check(const DemodArgs& A, unsigned long long f, long long off) {
    bound_check((long long)f, (long long)A.frames);
    bound_check(off, (long long)A.frame_samples);
}

// k_frames' IQ loads (each sample read once, the estimate symbols twice):
// non-temporal, so the stream does not evict the partly written output
// lines and the tables from L2 (as k_wave's IQ DMA, lphy_wave.h
// kIqCpol).  Same-box A/B (profiles/r5/ab_iq_nt.txt): SF 8 fused
// 0.999-1.012 -> 0.977-0.979 ms, SF 7 within noise; C1 WRITE_SIZE 33.0 ->
// 12.6 MB per launch.
__device__ __forceinline__ cf32 ld_iq(const cf32* p) {
    return __builtin_nontemporal_load(p);
}

__device__ __forceinline__ void store_symbol(const DemodArgs& A, const SymCtx& c, uint16_t idx) {
    bound_check(c.f, (long long)A.frames);
    if (c.have_sync && c.s < 2) {
        if (c.s == 0) A.meta[c.f].sw0 = idx;
        else A.meta[c.f].sw1 = idx;
    } else {
        const unsigned o = c.have_sync ? c.s - 2 : c.s;
        bound_check(o, (long long)A.out_per_frame);
        A.syms[(unsigned long long)c.f * A.out_per_frame + o] = idx;
    }
}

// (shared by k_demod's fast path and k_frames; see "Certified fast
// rotation" in lphy_frames.h)
__device__ __forceinline__ float max3_abs(float m, float a, float b) {
    float r;
    asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}

constexpr float kU = 5.9604645e-8f;  // 2^-24

// Table of frame `rec` (rate, scale, t_off): t_i for i = lane, lane+64, ...
template <int SF, int MODE>
__device__ __forceinline__ void build_rtab(cf32* tab, float rate, float scale, int t_off,
                                           const cf32* down, const float* win, int lane) {
    constexpr int N = 1 << SF;
    (void)t_off;
    for (int i = lane; i < N; i += 64) {
        float sn, cs;
        lphy_libm::sincosf_exact(rate * (float)i, &sn, &cs);
        cf32 t = cf32{cs, sn};
        if constexpr ((MODE & 3) == LPHY_MODE_DEMODULATE) t = cmul(down[i], t);
        if constexpr ((MODE & 3) != LPHY_MODE_DEMODULATE) t = cscale(t, scale);
        if constexpr ((MODE & kWinBit) != 0) t = cscale(t, win[i]);
        tab[i] = t;
    }
}

// Whether the fast path may take this symbol unit: every window (mode 2
// dechirps each sample exactly at its own chirp index before the table).
template <int SF, int MODE>
__device__ __forceinline__ bool fast_applies(const SymCtx& c, int t_off) {
    (void)c;
    (void)t_off;
    return true;
}

// The certificate of "Certified fast rotation" (lphy_frames.h).  amax bounds max(|Re y|, |Im y|)
// over the symbol's samples before rotation (modes 1/2: <= 1 after the
// frame's normalisation; mode 0: measured).
//
// Range guards keep every rounding relative: amax >= 1e-20 (denormal
// arithmetic stays negligible against B), b.v >= 1e-30 (a normal |X|^2), and
// a runner-up below 1e-30 is taken as 1e-30.
// extra: further u-multiples of a sample's rotation error (the two-table
// rotation of k_demod's fast path)
template <int SF>
__device__ __forceinline__ float cert_bound(float rate, float start, float amax, float extra = 0.0f) {
    constexpr int N = 1 << SF, L = (SF + 1) / 2;
    const float A = (float)N * 1.41421366f * amax * 1.0001f;
    const float ar = fabsf(rate) * (float)N;
    const float P = fabsf(start) + ar;
    return kU * A * ((24.0f + 12.0f * L + extra) + 2.0f * ar + P) * 1.001f;
}
// winner's lead over the runner-up, less the |X|^2 roundings.  The square
// roots are the hardware v_sqrt_f32 (within 1 ulp, i.e. 2u relative, for the
// normal inputs the certificate admits: b.v >= 1e-30, runner-up clamped to
// 1e-30), charged as 2 ulp = 4u on each side on top of the 8u: the
// correctly rounded sqrtf's Newton fix-up cost ~20 VALU per symbol tile.
// A NaN winner stays NaN and fails the comparison.
__device__ __forceinline__ float cert_gap(const ArgMax2& b) {
    return __builtin_amdgcn_sqrtf(b.v) * (1.0f - 12.0f * kU) -
           __builtin_amdgcn_sqrtf(fmaxf(b.v2, 1e-30f)) * (1.0f + 12.0f * kU);
}
template <int SF>
__device__ __forceinline__ bool fast_certified(const ArgMax2& b, const SymCtx& c, float amax,
                                               float extra = 0.0f) {
    constexpr int N = 1 << SF;
    const float A = (float)N * 1.41421366f * amax * 1.0001f;
    const float B = cert_bound<SF>(c.rate, c.start, amax, extra);
    return cert_gap(b) > 4.0f * B && A < 1e18f && amax >= 1e-20f && b.v >= 1e-30f;
}

// Verdict on a frame whose symbols were certified under a speculative
// normalisation (record sm) that its later samples overturned (settle_frames,
// k_spec_settle).  e holds the exact normalisation, u0 / u1 the two estimate
// units transformed again with it; they are folded into e's exact offsets.
// The symbols stand when the time shift is unchanged and every certified
// symbol's lead still covers the larger sample bound and the rate difference:
// a rate error d moves every bin by at most |d| N sum|y_i| <= |d| N A (the
// phase error of sample i is |d| i), charged twice on both sides of the
// comparison as fast_certified charges its B.  amax: the frame's max-abs under
// the speculative scale; lead: the symbols' least certificate ratio; open:
// some symbols still wait for recheck_frames.  Returns the record to store,
// status kStatusFixup when the frame must be re-run whole.
template <int SF>
__device__ __forceinline__ lphy_frame_meta settle_verdict(const lphy_frame_meta& sm, lphy_frame_meta e,
                                                          const UnitResult& u0, const UnitResult& u1,
                                                          float amax, float lead, bool open) {
    constexpr int N = 1 << SF;
    EstFold fold;
    if (u0.valid) fold.add(u0.idx, u0.findex, 0, u0.phase);
    else fold.add(0, 0.0f, 0, 0.0f);
    if (u1.valid) fold.add(u1.idx, u1.findex, 0, u1.phase);
    else fold.add(0, 0.0f, 0, 0.0f);
    fold.finish(e, 2, N, 1);
    // amplitude bound of the speculatively scaled samples, and the smallest
    // bound of any symbol (|start| grows with the symbol)
    const float a = fmaxf(1.0f, amax) * 1.0001f;
    const float b1 = cert_bound<SF>(sm.rate, sm.rate * (float)sm.t_off, 1.0f);
    const float d = fabsf(e.rate - sm.rate) * (1.0f + 4.0f * kU);
    const float A1 = (float)N * 1.41421366f * 1.0001f;
    const bool ok = e.t_off == sm.t_off && sm.t_off >= -N && sm.t_off <= N &&
                    lead > 4.0f * a + 4.0f * d * (float)N * A1 * a / b1;
    e.sw0 = sm.sw0;
    e.sw1 = sm.sw1;
    e.status = !ok ? kStatusFixup : (open ? kStatusRecheck : 0);
    return e;
}

// Stage 2: per-symbol demodulation, persistent grid.  The workgroup stages
// the twiddles (and, up to N = 1024, the down-chirp and window) in LDS once.
//  * SF <= 10 (a symbol's LPS <= 64 lanes sit in one wavefront): every
//    wavefront is an independent worker with its own LDS slots and no
//    workgroup barrier in its loop; it software-pipelines the next tile's
//    frame record (during staging) and IQ (during the FFT).
//  * SF 11-12: workgroup tiles with barriers (a symbol spans wavefronts).
//    Symbols take the certified fast rotation (as k_frames) with
//    a two-table rotation: e^{j rate i} = e^{j rate 64h} e^{j rate l} for
//    i = 64h + l, whose 64 + N/64 entries the team computes per tile (exact
//    sincos) instead of one sincos per sample; uncertified symbols are left
//    to k_post (kSymRecheck, kStatusRecheck).  LPHY_F_EXACT_ROTATION and
//    osr > 1 keep the per-sample rotation.
template <int SF, int MODE, int OCC>
__global__ __launch_bounds__(kTile, OCC) void k_demod(DemodArgs A) {
    using G = Geo<SF>;
    constexpr int N = G::N;
    constexpr bool TAB = N <= 1024;  // chirp + window tables in LDS
    constexpr bool WAVE = G::LPS <= 64;
    constexpr int WT = WAVE ? 64 / G::LPS : G::T;  // symbols per worker tile
    constexpr bool FASTB = !WAVE && (MODE & kOsrBit) == 0;  // two-table fast path
    constexpr int NH = N / 64;                               // high-part entries
    __shared__ cf32 lds[G::T * G::SSTRIDE];
    __shared__ cf32 twl[N];
    __shared__ cf32 dnl[TAB ? N : 1];
    __shared__ float wnl[TAB ? N : 1];
    __shared__ ArgMax red[kTile / 64];
    // double-buffered by tile parity: the next tile's tables are built at the
    // end of this one, and the reductions need no trailing barrier
    __shared__ ArgMax2 red2[2][FASTB ? kTile / 64 : 1];
    __shared__ float redm[2][FASTB ? kTile / 64 : 1];
    __shared__ cf32 thi[2][FASTB ? G::T : 1][FASTB ? NH : 1];
    __shared__ cf32 tlo[2][FASTB ? G::T : 1][FASTB ? 64 : 1];
    const bool fastb = FASTB && !A.exact_rotation;
    unsigned tp = 0;  // tile parity

    const int tid = threadIdx.x;
    for (int i = tid; i < N; i += kTile) {
        twl[i] = A.tw[i];
        if constexpr (TAB) {
            if ((MODE & 3) != LPHY_MODE_LORA_DEMODULATE) dnl[i] = A.down[i];
            if (A.win) wnl[i] = A.win[i];
        }
    }
    __syncthreads();
    const cf32* down = TAB ? dnl : A.down;
    const float* win = A.win ? (TAB ? wnl : A.win) : nullptr;

    const int slot = tid / G::LPS, lam = tid % G::LPS;
    const unsigned S = (unsigned)A.total_syms;
    const unsigned nframes = (unsigned)A.frames;
    const int wslot = WAVE ? slot % WT : slot;  // symbol slot inside the worker tile
    unsigned worker;
    if constexpr (WAVE) worker = blockIdx.x * (kTile / 64) + (tid >> 6);
    else worker = blockIdx.x;
    const Stage<SF> stg(slot, lam);

    // this team's first symbol and its (frame, symbol) coordinates
    const unsigned g0 = worker * WT + wslot;
    unsigned f = g0 / S, s = g0 - f * S;
    auto step = [&](unsigned& ff, unsigned& ss) {
        ss += A.stride_s;
        ff += A.stride_f;
        if (ss >= S) { ss -= S; ++ff; }
    };
    // the worker's tile loop ends when its first team passes the last frame
    const unsigned fw0 = (worker * WT) / S;
    unsigned fw = fw0, sw = worker * WT - fw0 * S;

    // prologue of the software pipeline
    constexpr bool OSR = (MODE & kOsrBit) != 0;
    const unsigned osr = OSR ? (unsigned)A.osr : 1u;  // sample stride of a symbol
    lphy_frame_meta m = A.meta[f < nframes ? f : 0];
    SymCtx c = sym_ctx<OSR>(A, f < nframes ? f : 0, f < nframes ? s : 0, f < nframes, N, m);
    // the two rotation tables of a tile's symbol (scale folded into the low
    // one), written by the team's first NH + 64 lanes
    auto build_tables = [&](const SymCtx& cc, unsigned b) __attribute__((always_inline)) {
        if constexpr (FASTB) {
            if (cc.ok) {
                float sn, cs;
                if (lam < NH) {
                    lphy_libm::sincosf_exact(cc.rate * (float)(64 * lam), &sn, &cs);
                    thi[b][slot][lam] = cf32{cs, sn};
                } else if (lam < NH + 64) {
                    const int l = lam - NH;
                    lphy_libm::sincosf_exact(cc.rate * (float)l, &sn, &cs);
                    cf32 t = cf32{cs, sn};
                    if constexpr ((MODE & 3) != LPHY_MODE_DEMODULATE) t = cscale(t, cc.scale);
                    tlo[b][slot][l] = t;
                }
            }
        }
    };
    if (FASTB && fastb) build_tables(c, 0);  // visible after the loop's first barrier
    cf32 raw[16];
    {
        const cf32* src = A.iq + (unsigned long long)c.f * A.frame_samples + c.base;
#pragma unroll
        for (int e = 0; e < G::E; ++e) raw[e] = src[(unsigned)(lam + e * G::LPS) * osr];
    }

#ifdef LPHY_PROFILE_PHASES  // timing experiments only: per-phase clock sums
    unsigned long long ph_stage = 0, ph_fft = 0, ph_tail = 0;
#endif
    while (fw < nframes) {
#ifdef LPHY_PROFILE_PHASES
        const unsigned long long p0 = clock64();
#endif
        // next tile: coordinates and frame record (in flight during staging)
        unsigned nf = f, ns = s, nfw = fw, nsw = sw;
        step(nf, ns);
        step(nfw, nsw);
        const bool nlive = nf < nframes;
        const lphy_frame_meta nm = A.meta[nlive ? nf : 0];

        if constexpr (!WAVE) __syncthreads();  // previous tile's readers done
        float amax = 0.0f;  // fast path, mode 0: the team's max(|Re x|, |Im x|)
        if (FASTB && fastb) {
            // this tile's tables were built at the end of the previous one
            const cf32 tl = tlo[tp][slot][lam & 63];
#pragma unroll
            for (int e = 0; e < G::E; ++e) {
                const int i = lam + e * G::LPS;
                cf32 p = raw[e];
                if constexpr ((MODE & 3) == LPHY_MODE_DEMODULATE) {
                    amax = max3_abs(amax, p.x, p.y);
                    p = cmul(p, down[i]);
                }
                if constexpr ((MODE & 3) == LPHY_MODE_DECHIRP_LORA_DEMODULATE)
                    p = cmul(p, down[(c.base + (unsigned)i) & (N - 1)]);
                // modes 1/2 (spec_big): the [dechirped] samples' max-abs
                if constexpr ((MODE & 3) != LPHY_MODE_DEMODULATE) amax = max3_abs(amax, p.x, p.y);
                cf32 q = cmul_fma(cmul_fma(p, tl), thi[tp][slot][(lam >> 6) + e * (G::LPS / 64)]);
                if constexpr ((MODE & kWinBit) != 0) q = cscale(q, win[i]);
                stg.put(lds, e, c.ok ? q : czero());
            }
        } else {
            stage_symbol<SF, MODE>(lds, stg, raw, A.iq + (unsigned long long)c.f * A.frame_samples + c.base,
                                   c, lam, down, win, (int)osr);
        }
        team_sync<SF>();
#ifdef LPHY_PROFILE_PHASES
        const unsigned long long p1 = clock64();
#endif

        // next tile's IQ: in flight during this tile's FFT
        const SymCtx nc = sym_ctx<OSR>(A, nlive ? nf : 0, nlive ? ns : 0, nlive, N, nm);
        if (nfw < nframes) {
            const cf32* nsrc = A.iq + (unsigned long long)nc.f * A.frame_samples + nc.base;
#pragma unroll
            for (int e = 0; e < G::E; ++e) raw[e] = nsrc[(unsigned)(lam + e * G::LPS) * osr];
        }

        cf32 v[16];
        if (FASTB && fastb) fft_tile<SF, true>(v, lds, slot, lam, twl);
        else fft_tile<SF>(v, lds, slot, lam, twl);
        if constexpr (FASTB) {
            if (fastb) {
#ifdef LPHY_PROFILE_PHASES
                const unsigned long long q2 = clock64();
#endif
                // certificate (fast_certified, with the two-table rotation's
                // further 6u); a NaN or near-tie leaves the symbol to k_post
                // the team's top two and its samples' max-abs in one exchange
                const bool tm = (MODE & 3) == LPHY_MODE_DEMODULATE || A.spec_big != nullptr;
                const ArgMax2 b2 = symbol_argmax2_wg<SF, false>(local_argmax2<SF>(v, lam), red2[tp],
                                                                tm ? &amax : nullptr, redm[tp]);
                // modes 1/2: normalised frame (under spec_big, k_post's close
                // confirms the normalisation or settles the frame)
                const float am = (MODE & 3) == LPHY_MODE_DEMODULATE ? amax : 1.0f;
                const bool redo = !fast_certified<SF>(b2, c, am, 6.0f);
                if (c.ok && lam == 0) {
                    store_symbol(A, c, redo ? kSymRecheck : (uint16_t)b2.i);
                    if (redo) A.meta[c.f].status = kStatusRecheck;
                }
                if constexpr ((MODE & 3) != LPHY_MODE_DEMODULATE) {
                    if (A.spec_big && c.ok) {
                        uint4* r = &A.spec_big[c.f];
                        const cf32 q = v[0] * v[0];
                        const float q2 = q.x + q.y;
                        if (!(q2 == q2)) atomicOr(&r->w, 1u);  // a NaN sample reaches every bin
                        if (lam == 0) {
                            atomicMax(&r->y, __float_as_uint(amax));
                            if (redo) atomicOr(&r->w, 2u);
                            else atomicMin(&r->z, __float_as_uint(cert_gap(b2) / cert_bound<SF>(c.rate, c.start, 1.0f, 6.0f)));
                        }
                    }
                }
                build_tables(nc, tp ^ 1u);  // the next tile's, behind its first barrier
                tp ^= 1u;
                c = nc;
                f = nf; s = ns; fw = nfw; sw = nsw;
#ifdef LPHY_PROFILE_PHASES
                const unsigned long long q3 = clock64();
                ph_stage += p1 - p0; ph_fft += q2 - p1; ph_tail += q3 - q2;
#endif
                continue;
            }
        }
        // a NaN bin may hide a (NaN, NaN) product, where the reference's
        // Annex G product differs: the frame goes to the exact re-run
        if (fft_has_nan<SF>(v) && c.ok) A.meta[c.f].status = kStatusFixup;
#ifdef LPHY_PROFILE_PHASES
        const unsigned long long p2 = clock64();
#endif
        const ArgMax best = symbol_argmax<SF>(local_argmax<SF>(v, lam), red);
        if (c.ok && lam == 0) store_symbol(A, c, (uint16_t)best.i);
        if constexpr (WAVE) team_sync<SF>();  // slot reads done before restaging
        c = nc;
        f = nf; s = ns; fw = nfw; sw = nsw;
#ifdef LPHY_PROFILE_PHASES
        const unsigned long long p3 = clock64();
        ph_stage += p1 - p0; ph_fft += p2 - p1; ph_tail += p3 - p2;
#endif
    }
#ifdef LPHY_PROFILE_PHASES
    if ((tid & 63) == 0) {
        atomicAdd(&A.counters[kCtrClocks + 0], ph_stage);
        atomicAdd(&A.counters[kCtrClocks + 1], ph_fft);
        atomicAdd(&A.counters[kCtrClocks + 2], ph_tail);
    }
#endif
}

}  // namespace
