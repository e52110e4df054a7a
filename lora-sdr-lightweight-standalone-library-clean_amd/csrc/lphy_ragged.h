// lphy_ragged.h — lphy_hip_demod_ragged: frames of different lengths in one
// call, each described by a lphy_ragged_desc (include/lphy_hip.h).  Three
// symbol-parallel launches, like the separate launches of lphy_demod.h:
//   k_rg_prologue<SF>  per frame: the length checks the uniform call makes on
//                      the host, max-abs (modes 1/2, LoRaDemod.cpp:60-78) and
//                      the estimate on min(total, 2) symbols
//                      (LoRaDemod.cpp:80-140 / phy.cpp:81-148);
//   k_rg_demod<SF, M>  per symbol: the work unit is a global symbol index u,
//                      its frame found by binary search over unit_offset;
//                      the reference's per-sample rotation -> FFT -> argmax
//                      (LoRaDemod.cpp:142-176 / phy.cpp:204-238);
//   k_rg_final<SF>     per frame: sync word, decode, CRC (lphy_final.h).
// The device functions of lphy_demod.h take the uniform DemodArgs; here they
// get a per-frame view of it (frame_view: base pointers, samples, total_syms,
// out_per_frame of one frame, frame index 0), so the end clamp, the max-abs
// extent and the output slots are the frame's own and the uniform kernels are
// compiled from unchanged code.  From there: the prologue's max-abs reduction
// (workgroup_max) and the tables' trip into LDS (load_tables); the unit's
// frame and record come from ragged_unit (lphy_ragged_unit.h, shared with the
// ragged detector and transmit).  The prologue's estimate pass is estimate_unit
// written out (at SF 12 the helper cost registers and a wave per SIMD): a
// change to it is made here too.
// Exactness: every product a non-finite value could reach is redone with the
// reference's Annex G product in place (the max-abs scan and a symbol's
// staging + FFT), so no frame is handed to a later exact re-run.
// Also lphy_hip_estimate_ragged, on the same table: k_rg_estimate<SF>, one
// launch, estimate_offsets (phy.cpp:81-148) on each frame's first symbols.
#pragma once
#include "lphy_demod.h"
#include "lphy_final.h"
#include "lphy_ragged_layout.h"
#include "lphy_ragged_unit.h"

namespace {

// x86-64's default NaN (0.0f / 0.0f on the reference's host): what
// lora_demodulate's estimate leaves in cfo and time_offset for a frame
// without a whole symbol (est_syms == 0, LoRaDemod.cpp:80,130-140)
constexpr unsigned kHostDefaultNan = 0xffc00000u;

template <int SF>
__device__ __forceinline__ DemodArgs frame_view(const RaggedArgs& R, unsigned long long f,
                                                const lphy_ragged_desc& d) {
    DemodArgs V = R.A;
    const unsigned long long total = d.samples >> SF;
    bound_check((long long)f, (long long)R.A.frames);
    V.iq = R.A.iq + d.iq_offset;
    V.syms = R.A.syms + d.sym_offset;
    V.meta = R.A.meta + f;
    V.frames = 1;
    V.frame_samples = d.samples;
    V.total_syms = total;
    V.out_per_frame = ragged_out_syms(total, R.A.mode);
    V.est_units = (int)ragged_est_syms(total, R.A.mode);
    return V;
}

// The frame's status from its length alone: the conditions the uniform call
// returns before it launches anything (lphy_hip_demod_batch)
__device__ __forceinline__ int length_status(int mode, unsigned long long samples, int N) {
    if (samples >= kRaggedMaxSamples) return -ERANGE;  // 32-bit sample bookkeeping (sym_ctx)
    const unsigned long long total = samples / (unsigned)N;
    if (mode == LPHY_MODE_DEMODULATE) {
        if (samples % (unsigned)N) return -EINVAL;  // phy.cpp:190-194
        if (total < 2) return -ERANGE;
    }
    if (mode == LPHY_MODE_DECHIRP_LORA_DEMODULATE && samples % (unsigned)N) return -EINVAL;
    return 0;
}

// Frames per workgroup of the prologue and of k_rg_estimate, and so of their
// launchers' grids (lphy_launch.h): half a tile's symbols, two per frame.
template <int SF>
constexpr int rg_fpw() { return Geo<SF>::T >= 2 ? Geo<SF>::T / 2 : 1; }

// ---------------------------------------------------------------------------
// Prologue.  A workgroup takes FPW = rg_fpw consecutive frames (one at SF
// 11-12): it scans them one after the other with all its threads (modes 1/2),
// then transforms their 2 FPW estimate symbols in one tile pass (two at
// SF 12, whose tile holds one symbol) and thread k folds frame k.
// ---------------------------------------------------------------------------
template <int SF>
__global__ __launch_bounds__(kTile) void k_rg_prologue(RaggedArgs R) {
    using G = Geo<SF>;
    constexpr int N = G::N, T = G::T;
    constexpr int FPW = rg_fpw<SF>();
    constexpr int PASSES = (2 * FPW + T - 1) / T;
    __shared__ cf32 lds[T * G::SSTRIDE];
    __shared__ cf32 twl[N];
    __shared__ ArgMax red[kTile / 64];
    __shared__ float wmax[kTile / 64];
    __shared__ lphy_frame_meta fm[FPW];
    __shared__ int fest[FPW];  // estimate symbols of the frame
    __shared__ UnitResult units[2 * FPW];

    const int tid = threadIdx.x;
    const int mode = R.A.mode;
    const unsigned long long nframes = R.A.frames;
    const unsigned long long f0 = (unsigned long long)blockIdx.x * FPW;
    load_tables<N, false, false>(R.A, twl);

    // (1) length checks and normalisation, frame by frame
    for (int k = 0; k < FPW; ++k) {
        const unsigned long long f = f0 + k;
        if (f >= nframes) break;  // uniform
        const lphy_ragged_desc d = R.desc[f];
        const int st = length_status(mode, d.samples, N);
        const unsigned long long total = d.samples >> SF;
        float mx = 0.0f;
        if (st == 0 && mode != LPHY_MODE_DEMODULATE) {
            const cf32* fr = R.A.iq + d.iq_offset;
            const unsigned count = (unsigned)d.samples;  // the frame's own extent, a partial symbol included
            // four loads in flight per lane
            auto scan = [&](auto&& acc) __attribute__((always_inline)) {
                unsigned i = (unsigned)tid;
                for (; i + 3u * kTile < count; i += 4u * kTile) {
                    const cf32 x0 = fr[i], x1 = fr[i + kTile], x2 = fr[i + 2u * kTile], x3 = fr[i + 3u * kTile];
                    acc(x0, i);
                    acc(x1, i + kTile);
                    acc(x2, i + 2u * kTile);
                    acc(x3, i + 3u * kTile);
                }
                for (; i < count; i += kTile) acc(fr[i], i);
            };
            if (mode == LPHY_MODE_DECHIRP_LORA_DEMODULATE) {
                bool bad = false;
                scan([&](cf32 x, unsigned i) {
                    x = cmul(x, R.A.down[i & (N - 1)]);
                    bad |= !(__builtin_isfinite(x.x) && __builtin_isfinite(x.y));
                    maxabs_acc(mx, x);
                });
                if (__syncthreads_or(bad)) {  // rare: the reference's product
                    mx = 0.0f;
                    for (unsigned i = tid; i < count; i += kTile) maxabs_acc(mx, cmul_x(fr[i], R.A.down[i & (N - 1)]));
                }
            } else {
                scan([&](cf32 x, unsigned) { maxabs_acc(mx, x); });
            }
        }
        mx = workgroup_max(mx, wmax);  // (0 where nothing was scanned: scale 1)
        if (tid == 0) {
            lphy_frame_meta m = norm_meta(mx, total >= 2, R.A.no_scratch);
            if (st != 0) {
                m = lphy_frame_meta{};
                m.status = st;
            }
            fm[k] = m;
            fest[k] = (int)ragged_est_syms(total, mode);
        }
        __syncthreads();
    }

    // (2) estimate units: unit u = 2 k + s is estimate symbol s of frame k
    const int slot = tid / G::LPS, lam = tid % G::LPS;
    for (int p = 0; p < PASSES; ++p) {
        const int u = p * T + slot;
        const int k = u >> 1, s = u & 1;
        const unsigned long long f = f0 + k;
        bool live = k < FPW && f < nframes;
        lphy_frame_meta m{};
        DemodArgs V = R.A;
        if (live) {
            m = fm[k];
            live = m.status == 0 && s < fest[k];
            V = frame_view<SF>(R, f, R.desc[f]);
        }
        __syncthreads();  // the previous pass's readers are done with lds
        const Stage<SF> stg(slot, lam);
#pragma unroll
        for (int e = 0; e < G::E; ++e) {
            const int i = lam + e * G::LPS;
            cf32 x = czero();
            if (live) {
                const unsigned long long idx = (unsigned long long)s * N + (unsigned)i;
                iq_check(V, 0, (long long)idx);
                x = est_sample(V, V.iq, idx, i, N, m);
            }
            stg.put(lds, e, x);
        }
        __syncthreads();
        cf32 v[16];
        fft_tile<SF, false, true>(v, lds, slot, lam, twl);
        // keep the bins for the interpolation and the phase
#pragma unroll
        for (int e = 0; e < G::E; ++e) lds[G::addr(slot, bin_of<SF>(e, lam))] = v[e];
        const ArgMax best = symbol_argmax<SF>(local_argmax<SF>(v, lam), red);
        __syncthreads();
        if (lam == 0 && k < FPW) {
            bound_check(u, 2 * FPW);
            units[u] = live ? unit_result<SF>(lds, slot, best) : kNoUnit;
        }
    }
    __syncthreads();

    // (3) fold and publish
    if (tid < FPW && f0 + tid < nframes) {
        lphy_frame_meta m = fm[tid];
        if (m.status == 0) {
            const int est = fest[tid];
            if (est == 0) {
                m.cfo = m.time_offset = m.rate = __uint_as_float(kHostDefaultNan);
                m.t_off = (int)0x80000000u;  // round_to_int(NaN)
            } else {
                EstFold fold;
                const bool tie_low = mode != LPHY_MODE_DEMODULATE;
                for (int s = 0; s < est; ++s) fold.unit(units[2 * tid + s], 0.0f, 1, tie_low);
                fold.finish(m, est, N, 1);
            }
        }
        R.A.meta[f0 + tid] = m;
    }
}

// ---------------------------------------------------------------------------
// Symbols.  Persistent grid over tiles of T units; a team (the LPS lanes of
// one symbol) finds its unit's frame by binary search over unit_offset
// (ragged_unit): the last record whose offset is <= u.  From SF 10 a symbol
// fills at least one wavefront, so the search runs on wave-uniform values;
// below, once per team.
// Staging as k_demod's exact path (stage_symbol: per-sample sincos, the large-
// argument form where the phase needs it); a NaN bin sends the wave's (SF <=
// 10) or the workgroup's symbols through the Annex G products once more, in
// place of the uniform kernels' kStatusFixup hand-off.
// ---------------------------------------------------------------------------
// Two waves per SIMD up to SF 10 (<= 256 VGPRs), one above.
template <int SF, int MODE>
__global__ __launch_bounds__(kTile, SF <= 10 ? 2 : 1) void k_rg_demod(RaggedArgs R) {
    using G = Geo<SF>;
    constexpr int N = G::N, T = G::T;
    constexpr bool TAB = N <= 1024;  // chirp + window tables in LDS
    constexpr bool WAVE = G::LPS <= 64;
    __shared__ cf32 lds[T * G::SSTRIDE];
    __shared__ cf32 twl[N];
    __shared__ cf32 dnl[TAB ? N : 1];
    __shared__ float wnl[TAB ? N : 1];
    __shared__ ArgMax red[kTile / 64];

    const unsigned nframes = (unsigned)R.A.frames;
    const lphy_ragged_desc* __restrict__ desc = R.desc;
    const unsigned long long units = desc[nframes].unit_offset;
    if ((unsigned long long)blockIdx.x * T >= units) return;  // uniform

    const int tid = threadIdx.x;
    // (mode 1 reads no down-chirp)
    load_tables<N, TAB && (MODE & 3) != LPHY_MODE_LORA_DEMODULATE, TAB && (MODE & kWinBit) != 0>(R.A, twl, dnl, wnl);
    __syncthreads();
    const cf32* down = TAB ? dnl : R.A.down;
    const float* win = (MODE & kWinBit) ? (TAB ? wnl : R.A.win) : nullptr;

    const int slot = tid / G::LPS, lam = tid % G::LPS;
    const Stage<SF> stg(slot, lam);
    const unsigned long long stride = (unsigned long long)gridDim.x * T;
    for (unsigned long long t0 = (unsigned long long)blockIdx.x * T; t0 < units; t0 += stride) {
        // (one symbol per wavefront or more: scalar search)
        const RaggedUnit ru = ragged_unit<G::LPS >= 64>(desc, nframes, units, t0 + (unsigned)slot);
        const lphy_ragged_desc& d = ru.d;
        const DemodArgs V = frame_view<SF>(R, ru.frame, d);
        const unsigned long long s64 = ru.s;
        const bool live = ru.live && s64 < V.total_syms && d.samples < kRaggedMaxSamples;
        lphy_frame_meta m{};
        if (live) m = V.meta[0];
        SymCtx c = sym_ctx(V, 0u, live ? (unsigned)s64 : 0u, live, N, m);
        if (!c.ok) {  // nothing loaded, zeros staged
            c.base = 0;
            c.rate = c.start = 0.0f;
            c.scale = 1.0f;
        }
        const cf32* src = V.iq + c.base;
        cf32 raw[16];
#pragma unroll
        for (int e = 0; e < G::E; ++e) {
            raw[e] = czero();
            if (c.ok) {
                iq_check(V, 0, (long long)c.base + lam + e * G::LPS);
                raw[e] = src[lam + e * G::LPS];
            }
        }
        if constexpr (!WAVE) __syncthreads();  // the previous tile's readers are done
        stage_symbol<SF, MODE>(lds, stg, raw, src, c, lam, down, win);
        team_sync<SF>();
        cf32 v[16];
        fft_tile<SF>(v, lds, slot, lam, twl);
        // a NaN bin may hide a (NaN, NaN) product, where the reference's
        // Annex G product differs
        const bool nan = c.ok && fft_has_nan<SF>(v);
        bool redo;
        if constexpr (WAVE) redo = __ballot(nan) != 0;
        else redo = __syncthreads_or(nan);
        if (redo) {
            team_sync<SF>();
            // (the samples are read again: held over the transform they cost 32 registers)
#pragma unroll
            for (int e = 0; e < G::E; ++e) raw[e] = c.ok ? src[lam + e * G::LPS] : czero();
#pragma unroll
            for (int e = 0; e < G::E; ++e) {
                const int i = lam + e * G::LPS;
                const float ph = c.start + c.rate * (float)i;
                stg.put(lds, e, rotate_sample<SF, MODE, true>(raw[e], i, c, down, win,
                                                              lphy_libm::sincosf_needs_large(ph)));
            }
            team_sync<SF>();
            fft_tile<SF, false, true>(v, lds, slot, lam, twl);
        }
        const ArgMax best = symbol_argmax<SF>(local_argmax<SF>(v, lam), red);
        if (c.ok && lam == 0) store_symbol(V, c, (uint16_t)best.i);
        if constexpr (WAVE) team_sync<SF>();  // slot reads done before restaging
    }
}

// ---------------------------------------------------------------------------
// Finalisation, a thread per frame: lphy_final.h on the frame's own slots.
// ---------------------------------------------------------------------------
template <int SF>
__global__ __launch_bounds__(kTile) void k_rg_final(RaggedArgs R) {
    const unsigned long long f = (unsigned long long)blockIdx.x * kTile + threadIdx.x;
    if (f >= R.A.frames) return;
    const lphy_ragged_desc d = R.desc[f];
    const unsigned long long total = d.samples >> SF;
    FinalArgs F{};
    F.syms = R.A.syms + d.sym_offset;
    F.bytes = R.bytes ? R.bytes + d.sym_offset / 2 : nullptr;
    F.meta = R.A.meta + f;
    F.frames = 1;
    F.nsyms = ragged_out_syms(total, R.A.mode);
    F.sym_stride = F.nsyms;
    F.shift = R.shift;
    F.decode = R.decode;
    F.set_sync = 1;
    finalize_frame(F, 0);
}

// ---------------------------------------------------------------------------
// lphy_hip_estimate_ragged: estimate_offsets (phy.cpp:81-148) on the first
// n_f = min(samples, est_samples) / (N osr) whole symbols of every frame
// (est_samples == 0: the whole frame).  k_estimate's packed form (several
// short frames in a tile) and its unpacked form (one long frame in chunks of
// T) as one loop: a workgroup takes the prologue's group of FPW consecutive
// frames and walks their concatenated units, U_f = n_f osr each, in passes of
// T; a pass may hold the tail of one frame, whole frames and the head of the
// next.  Thread k folds the units of frame k that lay in the pass, in unit
// order, and carries the fold across passes (EstFold keeps the state between
// the osr phases of a symbol, so a pass edge may split them).  The table's
// unit_offset counts the whole symbols of the whole frame, not these units,
// and is not read; nor are sym_offset and record [frames].
// In-frame parallelism is T units per pass per workgroup, as in k_estimate.
// ---------------------------------------------------------------------------
template <int SF>
__global__ __launch_bounds__(kTile) void k_rg_estimate(RaggedArgs R, unsigned long long est_samples) {
    using G = Geo<SF>;
    constexpr int N = G::N, T = G::T;
    constexpr int FPW = rg_fpw<SF>();
    __shared__ cf32 lds[T * G::SSTRIDE];
    __shared__ cf32 twl[N];
    __shared__ ArgMax red[kTile / 64];
    __shared__ UnitResult units[T];
    __shared__ float upow[T];
    __shared__ unsigned long long fiq[FPW];  // the frame's first sample
    __shared__ unsigned upre[FPW + 1];       // exclusive prefix of the group's units (< FPW 2^31 / N)

    const int tid = threadIdx.x;
    const int osr = R.A.osr;
    const unsigned step = (unsigned)N * (unsigned)osr;
    const unsigned long long nframes = R.A.frames;
    const unsigned long long f0 = (unsigned long long)blockIdx.x * FPW;
    load_tables<N, false, false>(R.A, twl);

    // (1) the frame of thread k < FPW: status, estimate symbols, units
    int st = 0;
    unsigned nsym = 0;       // n_f
    bool have_sync = false;
    const bool mine = tid < FPW && f0 + tid < nframes;
    if (tid < FPW) {
        unsigned long long off = 0;
        if (mine) {
            const lphy_ragged_desc d = R.desc[f0 + tid];
            if (d.samples >= kRaggedMaxSamples) {
                st = -ERANGE;  // the ragged demodulator's rule (length_status)
            } else {
                const unsigned long long e = est_samples && est_samples < d.samples ? est_samples : d.samples;
                nsym = (unsigned)e / step;
                have_sync = (unsigned)d.samples / step >= 2;
                off = d.iq_offset;
            }
        }
        fiq[tid] = off;
        upre[tid + 1] = nsym * (unsigned)osr;  // the count; thread 0 makes it the prefix
    }
    __syncthreads();
    if (tid == 0) {
        unsigned acc = 0;
        upre[0] = 0;
        for (int k = 1; k <= FPW; ++k) {
            acc += upre[k];
            upre[k] = acc;
        }
    }
    __syncthreads();
    const unsigned total = upre[FPW];  // uniform
    const unsigned ubeg = tid < FPW ? upre[tid] : 0u, uend = tid < FPW ? upre[tid + 1] : 0u;

    // (2) passes of T units; (3) the folds of the frames a pass touched
    EstFold fold;
    lphy_frame_meta none{};
    none.scale = 1.0f;
    const int slot = tid / G::LPS, lam = tid % G::LPS;
    for (unsigned p0 = 0; p0 < total; p0 += T) {
        const unsigned u = p0 + (unsigned)slot;
        const bool live = u < total;
        int k = 0;  // the last frame whose prefix is <= u: the one that holds it
        if (live) {
#pragma unroll
            for (int j = 1; j < FPW; ++j) k = upre[j] <= u ? j : k;
        }
        const unsigned uf = live ? u - upre[k] : 0u;
        const int s = (int)(uf / (unsigned)osr), t = (int)(uf % (unsigned)osr);
        DemodArgs V = R.A;  // (mode 0: est_sample reads A.mode and A.win)
        V.iq = R.A.iq + fiq[k];
        V.frames = 1;
        V.frame_samples = (unsigned long long)(upre[k + 1] - upre[k]) * (unsigned)N;  // n_f step: the extent read
        if (live) {
            bound_check(k, FPW);
#pragma unroll
            for (int e = 0; e < G::E; ++e)
                iq_check(V, 0, (long long)(((unsigned long long)s * N + (unsigned)(lam + e * G::LPS)) * osr + t));
        }
        __syncthreads();  // the previous pass's readers are done with lds / units
        const ArgMax best = estimate_unit<SF>(V, V.iq, s, t, osr, none, live, lds, slot, lam, twl, red);
        if (lam == 0) {
            bound_check(slot, T);
            units[slot] = live ? unit_result<SF>(lds, slot, best) : kNoUnit;
            if (osr > 1) upow[slot] = live ? detector_power(best.v > 0.0f ? best.v : 0.0f, R.A.power_scale) : 0.0f;
        }
        __syncthreads();
        if (tid < FPW) {
            const unsigned a = ubeg > p0 ? ubeg : p0;
            const unsigned b = uend < p0 + T ? uend : p0 + T;
            for (unsigned j = a; j < b; ++j) {
                bound_check((long long)(j - p0), T);
                fold.unit(units[j - p0], osr > 1 ? upow[j - p0] : 0.0f, osr, false);  // phy.cpp:106-121: no tie-break
            }
        }
    }

    // (4) publish; a frame without a whole symbol keeps its record (phy.cpp:87,91)
    if (mine) {
        lphy_frame_meta m{};
        if (st != 0) {
            m.status = st;
            R.A.meta[f0 + tid] = m;
        } else if (nsym != 0) {
            m.scale = 1.0f;
            m.have_sync = have_sync;
            fold.finish(m, (int)nsym, N, osr);
            R.A.meta[f0 + tid] = m;
        }
    }
}

}  // namespace
