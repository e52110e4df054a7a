// lphy_frames.h — k_frames, the fused single launch for SF <= 10 (a wavefront
// per frame: max-abs scan, estimate, symbols), and the wave-wide scans
// (wave_maxabs, wave_range_maxabs) and fast staging (stage_fast) it shares
// with k_wave (lphy_wave.h).
#pragma once
#include "lphy_demod.h"

namespace {

// ---------------------------------------------------------------------------
// Fused single launch (LPS <= 64 i.e. SF <= 10, two estimate symbols, osr 1).
// Every wavefront owns the frames f = w, w + W, w + 2W, ... (W waves in the
// grid) and runs their whole chain itself, so no data crosses wavefronts:
//   M  max(|I|,|Q|) scan of the frame (LoRaDemod.cpp:60-78), wave-wide
//   E  the two estimate FFTs (LoRaDemod.cpp:80-140 / phy.cpp:81-148) and the
//      fold into the frame's offsets
//   D  the frame's symbols (rotation, FFT, argmax)
// The wave works through a stream of "units" in tiles of WT = 64/LPS, one
// unit per team of LPS lanes.  Its frames go in groups of F = WT/2 (at
// least 1), whose 2F estimate units fill EBT whole tiles (EB):
//   [EB(0), one spacer tile] then per group g:
//   [D(g): DBT - 1 tiles, EB(g+1), D(g): its last tile]
// where D(g) is the F S symbol units of the group (the last tile padded
// with dead units).  No tile mixes estimate units with symbol units: a
// mixed tile runs the estimate staging, the exact transform and the exact
// top two for the whole wave (measured at SF7: one mixed tile per frame
// cost 1.8x a symbol tile, 20 % of the wave's clocks; a whole EB tile for
// four frames costs 2.1x, 6 %).  The F frames of an EB tile fold on the
// first lanes of their teams at once.  EB(g+1) folds two tiles before
// D(g+1) starts (what the one-tile-ahead context and IQ prefetch need).
// M of group g+1's frames runs right before the EB tile.  Measured
// alternatives, all slower at SF7 than this blocking 8-deep scan: M
// streamed in row chunks held in registers across the FFT (spills, 1.35x),
// M streamed by LDS-DMA into a per-wave ring (1.15x), scan-only workgroups
// beside the symbol waves (1.3-5x: they need ~25 % of the slots to stay
// ahead), the group's F scans with all their loads in flight at once (2 %
// slower in mode 2).
// Frame records pass between teams through a 2F-slot ring per wave in LDS
// (the group in demodulation and the next one).  Compared with separate launches this
// removes a whole-batch pass (the prologue kernels) and overlaps the
// HBM-bound max-abs scans of some waves with the VALU-bound transforms of
// the others.
// ---------------------------------------------------------------------------

// Per-frame record of the public meta array written by E: every field but
// sw0 / sw1, which the D tasks of symbols 0 and 1 write (disjoint bytes, so
// the two L2 write-backs cannot clobber each other).
__device__ __forceinline__ void meta_put_est(lphy_frame_meta* dst, const lphy_frame_meta& m) {
    float4* d16 = reinterpret_cast<float4*>(dst);
    d16[0] = float4{m.cfo, m.time_offset, m.rate, m.scale};
    int* d8 = reinterpret_cast<int*>(dst);
    d8[4] = m.t_off;
    d8[5] = m.status;
    uint8_t* b = reinterpret_cast<uint8_t*>(dst);
    b[28] = m.sync_word;
    b[29] = m.crc_ok;
    b[30] = m.normalised;
    b[31] = m.have_sync;
}

// Max-abs of frame f by one wavefront (16-byte loads, 8 in flight per
// lane), same arithmetic as k_maxabs; the result is in every lane.
//
// Fast form of the aligned bulk (one v_max3 per sample): max(mx, |re|, |im|)
// equals the reference's fold for samples without NaN, and the frame's
// samples are summed alongside (one packed add per sample) so that any NaN
// - or an overflow to inf, which could make one - sends the whole frame to
// the per-sample fold above, whose NaN rules (a NaN real part hides the
// sample) v_max3 does not have.  In mode 2 only the whole symbols are
// scanned: the zeros the reference's dechirp leaves past them never raise
// the maximum.

template <int SF, int MODE>
__device__ __forceinline__ float wave_maxabs(const DemodArgs& A, unsigned f, const cf32* down,
                                             unsigned limit = 0) {
    constexpr int N = 1 << SF;
    constexpr bool DECH = (MODE & 3) == LPHY_MODE_DECHIRP_LORA_DEMODULATE;
    const int lane = threadIdx.x & 63;
    const cf32* fr = A.iq + (unsigned long long)f * A.frame_samples;
    // limit: the first `limit` samples only (speculative normalisation)
    const unsigned count = limit ? limit : (DECH ? (unsigned)A.total_syms * N : (unsigned)A.frame_samples);
    iq_check(A, f, (long long)count - 1);
    float mx = 0.0f;
    bool bad = false;  // non-finite [dechirped] sample
    auto acc = [&](cf32 x, unsigned i) {
        if constexpr (DECH) x = cmul(x, down[i & (N - 1)]);
        bad |= !(__builtin_isfinite(x.x) && __builtin_isfinite(x.y));
        maxabs_acc(mx, x);
    };
    // loads in flight per lane (round 1, whole-frame scan at SF7: 16, 24,
    // 32 and 33 within 1 %; round 2, with the samples staged in registers:
    // 8 spills 6 VGPRs where 16 spills 15, 4 % faster under speculation and
    // 1 % with the whole-frame scan)
    constexpr int U = 8;
    // chirp index of sample 2 (b + 64 u + lane) for a round base b = 64 U r:
    // the 128 U r term vanishes mod N
    static_assert((128 * U) % N == 0, "chirp phase of the unrolled scan");
    bool exact = (reinterpret_cast<uintptr_t>(fr) & 15) != 0;
    if (!exact) {
        const float4* f4 = reinterpret_cast<const float4*>(fr);
        const unsigned n4 = count / 2;
        float fm = 0.0f;
        cf32 sum = czero();
        auto round = [&](const float4 (&v)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cf32 a = cf32{v[u].x, v[u].y}, b = cf32{v[u].z, v[u].w};
                if constexpr (DECH) {
                    const unsigned ci = (2u * (unsigned)lane + 128u * (unsigned)u) & (N - 1);
                    a = cmul(a, down[ci]);
                    b = cmul(b, down[(ci + 1) & (N - 1)]);
                }
                fm = max3_abs(fm, a.x, a.y);
                fm = max3_abs(fm, b.x, b.y);
                sum = sum + a;
                sum = sum + b;
            }
        };
        unsigned base = 0;
        for (; base + U * 64 <= n4; base += U * 64) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = f4[base + u * 64 + lane];
            round(v);
        }
        if (base < n4) {  // last partial round, zero-filled (zeros never raise the max)
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned j = base + u * 64 + lane;
                v[u] = j < n4 ? f4[j] : float4{0.0f, 0.0f, 0.0f, 0.0f};
            }
            round(v);
        }
        // a NaN or inf sample (or an inf - inf) ends in the sum as NaN, or
        // in the maximum as inf: the frame goes to the exact re-run
        bad = !(sum.x == sum.x && sum.y == sum.y) || !(fm <= 3.40282347e38f);
        mx = fm;
        if ((count & 1) && lane == 0) acc(fr[count - 1], count - 1);
    } else {
        for (unsigned i = lane; i < count; i += 64) acc(fr[i], i);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    // NaN: the caller's norm_meta_hot routes the frame to k_post
    return __ballot(bad) ? __builtin_nanf("") : mx;
}

// Max-abs of samples [lo, hi) of frame f by one wavefront, per-sample fold
// with the reference's NaN rules; `bad` when one is non-finite.  Used for
// the few samples no symbol window of a speculatively normalised frame
// covers (a negative time shift's last samples, mode 1's partial symbol).
template <int SF, int MODE>
__device__ float wave_range_maxabs(const DemodArgs& A, unsigned f, unsigned lo, unsigned hi,
                                   const cf32* down, bool& bad) {
    constexpr int N = 1 << SF;
    const int lane = threadIdx.x & 63;
    const cf32* fr = A.iq + (unsigned long long)f * A.frame_samples;
    float mx = 0.0f;
    bool b = false;
    if (hi > lo) iq_check(A, f, (long long)hi - 1);
    for (unsigned i = lo + (unsigned)lane; i < hi; i += 64) {
        cf32 x = fr[i];
        if constexpr ((MODE & 3) == LPHY_MODE_DECHIRP_LORA_DEMODULATE) x = cmul(x, down[i & (N - 1)]);
        b |= !(__builtin_isfinite(x.x) && __builtin_isfinite(x.y));
        maxabs_acc(mx, x);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    bad = __ballot(b) != 0;
    return mx;
}

// End of the samples the frame's symbol windows (shifted by t_off as
// LoRaDemod.cpp:144-150 does) and its two estimate symbols cover together,
// a contiguous run from sample 0; the frame's max-abs needs [end, count) too.
__device__ __forceinline__ unsigned covered_end(unsigned S, unsigned N, unsigned count, int t) {
    unsigned end = S * N;
    if (t > 0) {
        // windows s with s N + t + N <= count are shifted
        if ((unsigned long long)t + N <= count) {
            const unsigned long long smax = ((unsigned long long)count - (unsigned)t - N) / N;
            const unsigned long long last = smax < S - 1 ? smax : S - 1;
            const unsigned long long e = (last + 1) * N + (unsigned)t;
            if (e > end) end = (unsigned)e;
        }
    } else if (t < 0) {
        const unsigned long long off = (unsigned long long)(-(long long)t);
        if (off <= (unsigned long long)(S - 1) * N) end = (unsigned)(S * N - off);
    }
    return end > 2 * N ? end : 2 * N;
}

enum : int { kUnitDead = 0, kUnitEst = 1, kUnitSym = 2 };

// ---------------------------------------------------------------------------
// Certified fast rotation (k_frames symbol units).
//
// The reference rotates sample i of symbol s by the glibc sincosf of
// ph_i = fl(start_s + fl(rate * i)), start_s = rate * (s*N + t_off)
// (LoRaDemod.cpp:152-158, phy.cpp:217-222): one double-precision sincos per
// sample, half of the path's arithmetic.  A symbol's output is only the
// argmax of |FFT|^2, and |FFT(y * e^{j start})| = |FFT(y)|: the common phase
// start_s drops out of every magnitude.  So symbols are transformed as
//     q_i = x_i * t_i,   t_i = [down] * e^{j rate i} * [scale] * [win]
// with t a per-FRAME table (N entries, built once per frame from exact
// sincos of fl(rate*i)), i.e. one complex multiply per sample instead of a
// dechirp, a rescale, a sincos and a rotation.
//
// Exactness is certified per symbol, not assumed.  With u = 2^-24, A an
// upper bound of sum_i |y_i| (the symbol's L1 norm), P = |start| + |rate| N,
// L the number of KISS stages, the reference's bins X and ours X' satisfy
//   | |X_k| - |X'_k| | <= B = u A (24 + 12 L + 2 |rate| N + P) (1 + 1e-3):
//   * rotation inputs: the reference's sample differs from the ideal
//     y_i e^{j(start + rate i)} by <= u(10 + |rate| N + P)|y_i| (dechirp
//     3u, rescale u, sincos sqrt(2)u, phase roundings u(|rate| i + |ph|),
//     rotation 3u, window u); ours from e^{j start}-times-ideal by
//     <= u(10 + |rate| N)|y_i|;
//   * transform: each KISS stage adds <= 6u (sum of its butterfly's input
//     magnitudes) to an output; an output depends on one value of every
//     sub-transform of a level, whose inputs partition the symbol, so both
//     FFTs are within 6 L u A of the exact map (same float twiddles), and
//     the input difference passes with gain (1+u)^L.
// The reference's winner is ours when |X'_best| - 2B > |X'_second| (plus
// the 2u rounding of |X|^2 on both sides and of the check itself); any
// symbol that fails it - ties, near-ties, NaN, overflow risk, frames whose
// time shift is not applied to every symbol - is recomputed with the exact
// per-sample path.  The check below uses 4B (a factor 2 of slack).
// ---------------------------------------------------------------------------

// Fast staging of one tile: symbol units q_i = y_i * t_i from the frame's
// rotation table t (LDS ring for SF <= 8, the lane's registers above) with a
// fused product, where y is the sample, or in mode 2 its exact dechirp at
// its own chirp index (down: the doubled table); estimate units exactly as
// stage_mixed (no rotation).  Returns the lane's max(|Re y|, |Im y|) over its
// symbol samples: mode 0's certificate amplitude, and for modes 1/2 the
// samples' share of the frame's max-abs (speculative normalisation).
//
// The samples are held in first-pass order (element e of lane lam is sample
// fl + first_pass_index<SF>(e, 0), fl = the lane part): the staged values
// stay in registers and the transform starts there (fft_tile REG0).
template <int SF, int MODE, bool MIXED, bool EARLY>
__device__ __forceinline__ float stage_fast(cf32 (&v)[16], cf32 (&raw)[16], const SymCtx& c, int fl,
                                            const cf32* down, const float* win, const cf32* rt,
                                            const cf32* thl, bool est, const cf32* nsrc) {
    using G = Geo<SF>;
    constexpr int N = G::N;
    constexpr bool RLDS = SF <= 8;
    float amax = 0.0f;
    const cf32* dl = down + (c.base & (N - 1)) + fl;  // doubled table: no wrap
    const cf32* rtl = rt + fl;
    const float* wl = win + fl;
    // one branch per tile, not per element (per-element branches serialise
    // the table reads behind their own waits)
    if (MIXED && est) {
#pragma unroll
        for (int e = 0; e < G::E; ++e) {
            const int ce = first_pass_index<SF>(e, 0);
            bound_check((c.base & (N - 1)) + fl + ce, 2 * N);
            cf32 p = raw[e];
            if constexpr (EARLY) raw[e] = ld_iq(nsrc + ce);  // the next tile's sample, as this one is consumed
            if constexpr ((MODE & 3) != LPHY_MODE_DEMODULATE) {
                if constexpr ((MODE & 3) == LPHY_MODE_DECHIRP_LORA_DEMODULATE) p = cmul(p, dl[ce]);
                p = cscale(p, c.scale);
            }
            cf32 y = c.ok ? p : czero();
            if constexpr ((MODE & kWinBit) != 0) y = cscale(y, wl[ce]);
            v[e] = y;
        }
    } else {
#pragma unroll
        for (int e = 0; e < G::E; ++e) {
            const int ce = first_pass_index<SF>(e, 0);
            bound_check((c.base & (N - 1)) + fl + ce, 2 * N);
            bound_check(fl + ce, N);
            cf32 p = raw[e];
            if constexpr (EARLY) raw[e] = ld_iq(nsrc + ce);
            if constexpr ((MODE & 3) == LPHY_MODE_DECHIRP_LORA_DEMODULATE) p = cmul(p, dl[ce]);
            amax = max3_abs(amax, p.x, p.y);
            if constexpr (RLDS) {
                v[e] = cmul_fma(p, rtl[ce]);
            } else {
                // SF 9-10: two-table rotation (build_rtab2): thl[0..63] the low
                // part e^{j rate l} [* scale], thl[64..] the high part
                const int i = fl + ce;
                if constexpr ((MODE & 3) == LPHY_MODE_DEMODULATE) p = cmul(p, down[i]);
                cf32 q = cmul_fma(cmul_fma(p, thl[i & 63]), thl[64 + (i >> 6)]);
                if constexpr ((MODE & kWinBit) != 0) q = cscale(q, win[i]);
                v[e] = q;
            }
        }
    }
    return amax;
}

template <int SF, int MODE, int OCC>
__global__ __launch_bounds__(kTile, OCC) void k_frames(FrameArgs P) {
    using G = Geo<SF>;
    static_assert(G::LPS <= 64, "fused path needs a symbol inside one wavefront");
    constexpr int N = G::N;
    constexpr bool TAB = N <= 1024;
    static_assert(TAB, "LDS tables (the doubled down-chirp) for every fused SF");
    constexpr int WT = 64 / G::LPS;               // units per tile
    constexpr unsigned U = 2;                      // estimate units per frame
    // frames per group: the estimate units of F frames fill whole tiles
    // (EBT estimate-only tiles), so no tile mixes estimates with symbols
    constexpr unsigned F = WT >= (int)U ? (unsigned)WT / U : 1u;
    constexpr unsigned EBU = U * F, EBT = (EBU + WT - 1) / WT;
    // prefix tiles: EB(0), then one tile that keeps group 0's symbols two
    // tiles behind it like every later group's
    constexpr unsigned PT = EBT + 1;
    constexpr unsigned NSLOT = 2 * F;  // frame slots: the group in demodulation, the next one
    constexpr int WPB = kTile / 64;
    // rotation tables: per-wave LDS ring of two frames up to SF 8, per-lane
    // registers (built when a team reaches a new frame) for SF 9-10
    constexpr bool RLDS = SF <= 8;
    const DemodArgs& A = P.A;
    __shared__ cf32 lds[G::T * G::SSTRIDE];
    __shared__ cf32 twl[N];
    // down-chirp twice over (entry i = down[i mod N]): a symbol window's
    // chirp indices t0 + i, i < N, need no wrap
    __shared__ cf32 dnl[TAB ? 2 * N : 1];
    __shared__ float wnl[TAB ? N : 1];
    __shared__ UnitResult ures[WPB][F][U];
    __shared__ float4 ring[WPB][NSLOT];  // frame records: rate, scale, t_off, flags
    __shared__ float ringmx[WPB][NSLOT];  // ... and the max-abs their normalisation used
    __shared__ cf32 rtab[RLDS ? WPB : 1][RLDS ? NSLOT : 1][RLDS ? N : 1];
    // SF 9-10: two-table rotation per frame (64 low + N/64 high entries): a
    // whole-symbol table per lane cost 32 VGPRs and spilled
    __shared__ cf32 rtab2[RLDS ? 1 : WPB][RLDS ? 1 : NSLOT][RLDS ? 1 : 64 + N / 64];

    const int tid = threadIdx.x;
    for (int i = tid; i < N; i += kTile) {
        twl[i] = A.tw[i];
        if constexpr (TAB) {
            if ((MODE & 3) != LPHY_MODE_LORA_DEMODULATE) dnl[i] = dnl[i + N] = A.down[i];
            if (A.win) wnl[i] = A.win[i];
        }
    }
    __syncthreads();  // the last workgroup barrier: waves are independent below
    const cf32* down = TAB ? dnl : A.down;
    const float* win = A.win ? (TAB ? wnl : A.win) : nullptr;

    const int lane = tid & 63, wv = tid >> 6;
    const int slot = tid / G::LPS, lam = tid % G::LPS;
    const unsigned wslot = (unsigned)(slot % WT);
    const int fl = first_pass_index<SF>(0, lam);  // lane part of the sample index
    const unsigned nframes = (unsigned)A.frames;
    const unsigned S = (unsigned)A.total_syms;
    const unsigned W = P.waves;
    const unsigned w = blockIdx.x * WPB + wv;
    if (w >= nframes) return;
    const unsigned nk = (nframes - 1 - w) / W + 1;  // frames of this wave
    // group g: D(g) = the F S symbol units of frames gF..gF+F-1 in DBT tiles
    // (the last one padded with dead units), and EB(g+1) = the next group's
    // estimate units in EBT tiles after D(g)'s first PB = DBT - 1 tiles, so
    // that the last EB tile folds two tiles before D(g+1) starts (what the
    // one-tile-ahead context and IQ prefetch need; lphy_route.h: S >= WT, so
    // DBT >= 2 and the scan ahead of EB(g+1) runs in a D(g) tile)
    const unsigned DBT = (F * S + WT - 1) / WT, GT = DBT + EBT, PB = DBT - 1;
    const unsigned ng = (nk + F - 1) / F;
    const unsigned dt_last = ((nk - (ng - 1) * F) * S + WT - 1) / WT;  // live D tiles of the last group
    const unsigned ntiles = PT + (ng - 1) * GT + (dt_last <= PB ? dt_last : dt_last + EBT);
    auto slot_of = [](unsigned kf) -> unsigned {
        const unsigned sl = ((kf / F) & 1u) * F + kf % F;
        bound_check(sl, NSLOT);
        return sl;
    };
    // no certified outputs: LPHY_F_EXACT_ROTATION, or LPHY_F_DEBUG_RECHECK
    // (tests: every symbol left to k_post's exact re-run)
    const bool exact_only = A.exact_rotation != 0 || A.debug_recheck != 0;
    constexpr bool DECH = (MODE & 3) == LPHY_MODE_DECHIRP_LORA_DEMODULATE;
    // Speculative normalisation (modes 1/2).  The reference scales the whole
    // frame by 1 / max(|I|,|Q|) before it estimates (LoRaDemod.cpp:60-78), so
    // the exact estimate needs every sample first: a blocking pre-scan that
    // re-reads the frame.  Instead M scans only the two estimate symbols, the
    // frame is estimated and demodulated with that normalisation, and each
    // symbol unit folds its own samples' max-abs while they are in registers.
    // When the symbol that ends the frame is done, the frame's true max-abs
    // is known: the same normalisation means every output stands; otherwise
    // the frame goes to k_post's settle_frames (exact estimate, certificates
    // re-checked against the exact rate, else the whole-frame re-run).
    const bool spec = (MODE & 3) != LPHY_MODE_DEMODULATE && A.spec != 0;
    constexpr bool EARLY = (MODE & 3) == LPHY_MODE_DEMODULATE && (SF == 7 || SF == 8);

    // unit of this team in tile t; for t >= PT: group g, tile tg of the
    // group, and the team's symbol unit (frame dj of the group, symbol ds)
    // when tg is a D tile
    auto unit_of = [&](unsigned t, unsigned g, unsigned tg, unsigned dj, unsigned ds, unsigned& kind,
                       unsigned& fk, unsigned& s) {
        if (t < PT) {
            const unsigned q = t * WT + wslot;
            const bool e = t < EBT && q < EBU;
            fk = e ? q / U : 0u;
            s = e ? q % U : 0u;
            kind = e && fk < nk ? kUnitEst : kUnitDead;
        } else if (tg >= PB && tg < PB + EBT) {
            const unsigned q = (tg - PB) * WT + wslot;
            fk = (g + 1) * F + q / U;
            s = q % U;
            kind = q < EBU && fk < nk ? kUnitEst : kUnitDead;
        } else {
            fk = g * F + dj;
            s = ds;
            kind = dj < F && fk < nk ? kUnitSym : kUnitDead;
        }
    };
    // context of a unit; symbol units read their frame record from the ring
    auto ctx_of = [&](unsigned kind, unsigned fk, unsigned s) -> SymCtx {
        const unsigned f = w + fk * W;
        if (kind == kUnitSym) {
            const float4 r = ring[wv][slot_of(fk)];
            lphy_frame_meta m{};
            m.rate = r.x;
            m.scale = r.y;
            m.t_off = __float_as_int(r.z);
            const unsigned fl = __float_as_uint(r.w);
            m.status = (fl & 1u) ? 0 : -1;
            m.have_sync = (fl & 2u) ? 1 : 0;
            return sym_ctx(A, f, s, true, N, m);
        }
        SymCtx c{};
        c.f = kind == kUnitEst ? f : w;
        c.s = s;
        c.base = kind == kUnitEst ? s * N : 0;
        c.scale = 1.0f;
        c.live = kind == kUnitEst;
        return c;
    };

    unsigned g = 0, tg = 0, dj = 0, ds = wslot;  // position of tile t (t >= PT)
    unsigned kind, fk, su;
    unit_of(0, g, tg, dj, ds, kind, fk, su);
    SymCtx c = ctx_of(kind, fk, su);
    // M (modes 1/2): the max-abs scans of a group's frames run in the tile
    // before its first EB tile, between that tile's staging and its IQ
    // prefetch, when no tile data is held in registers; tile 0 holds EB(0),
    // scanned here.  Each frame's maximum goes to its slot of ringmx.
    // (Measured alternative, 1.4x slower at SF7: the scan streamed one
    // chunk per tile through a per-wave LDS buffer by LDS-DMA, issued after
    // staging and folded a tile later.)
    unsigned m_seq = 0xffffffffu;  // group whose frames are scanned
    // Under speculation (modes 1/2 with scratch) the EB tile takes its
    // frames' two-symbol max-abs from its own staged samples instead
    // (EST_MAX below), so the scans run only for the pre-scan schedule.
    // That needs both estimate units of a frame in one tile (teams 2j and
    // 2j + 1): 2 LPS <= 64 lanes, i.e. SF <= 9.  At SF 10 a team is the
    // whole wave (EBT = 2 tiles per frame), so the scans stay.
    constexpr bool kEbMax = 2 * G::LPS <= 64;
    auto scan_ahead = [&](unsigned nkind_, unsigned nfk_) {
        if constexpr ((MODE & 3) != LPHY_MODE_DEMODULATE) {
            if (kEbMax && spec) return;
            const unsigned long long nem = __ballot(nkind_ == kUnitEst);
            if (nem) {
                const unsigned grp = (unsigned)__shfl((int)nfk_, __ffsll((long long)nem) - 1, 64) / F;
                if (grp != m_seq) {
                    for (unsigned j = 0; j < F && grp * F + j < nk; ++j) {
                        const unsigned kk = grp * F + j;
                        const float m = wave_maxabs<SF, MODE>(A, w + kk * W, down, spec ? 2u * N : 0u);
                        if (lane == 0) ringmx[wv][slot_of(kk)] = m;
                    }
                    m_seq = grp;
                }
            }
        }
    };
    scan_ahead(kind, fk);
    cf32 raw[16];  // the next unit's samples, first-pass order
    {
        const cf32* src = A.iq + (unsigned long long)c.f * A.frame_samples + c.base + fl;
#pragma unroll
        for (int e = 0; e < G::E; ++e) {
            iq_check(A, c.f, (long long)c.base + fl + first_pass_index<SF>(e, 0));
            raw[e] = ld_iq(src + first_pass_index<SF>(e, 0));
        }
    }
    // speculative normalisation: the lane's running state for the two frames
    // whose symbols can be in flight (by parity of the frame): max-abs of the
    // symbol samples, least certificate ratio, flags (1 NaN, 2 symbol open)
    constexpr float kBig = 3.0e38f;
    float sp_mx0 = 0.0f, sp_mx1 = 0.0f, sp_r0 = kBig, sp_r1 = kBig;
    unsigned sp_fl0 = 0u, sp_fl1 = 0u;
#ifdef LPHY_PROFILE_PHASES  // timing experiments only: mixed / symbol-only tile clocks
    unsigned long long ph_mix = 0, ph_sym = 0, ph_fold = 0, n_mix = 0;
#endif

    for (unsigned t = 0; t < ntiles; ++t) {
#ifdef LPHY_PROFILE_PHASES
        const unsigned long long p0 = clock64();
        unsigned long long pf = 0;
#endif
        cf32 v[16];  // this tile's unit: staged samples, then its bins
        const cf32* rt = rtab[RLDS ? wv : 0][RLDS ? slot_of(fk) : 0];
        const cf32* thl = rtab2[RLDS ? 0 : wv][RLDS ? 0 : slot_of(fk)];
        // next tile's unit and context
        unsigned ng_ = g, ntg = tg, ndj = dj, nds = ds;
        unsigned nkind, nfk, nsu;
        SymCtx nc;
        auto next_pos = [&] {
            if (t + 1 == PT) {
                ng_ = 0; ntg = 0; ndj = 0; nds = wslot;
            } else if (t + 1 > PT) {
                if (tg < PB || tg >= PB + EBT) {  // tile t was a D tile
                    nds += WT;
                    if (nds >= S) { nds -= S; ++ndj; }
                }
                if (++ntg == GT) { ntg = 0; ++ng_; ndj = 0; nds = wslot; }
            }
            unit_of(t + 1, ng_, ntg, ndj, nds, nkind, nfk, nsu);
        };
        auto next_ctx = [&] {
            if (t + 1 < ntiles) scan_ahead(nkind, nfk);
            nc = ctx_of(nkind, nfk, nsu);
        };
        // EARLY (mode 0 at SF 7-8, measured): the next tile's IQ is loaded as
        // this tile's staging consumes the registers, so it is in flight
        // during staging and the FFT.  (Mode 2: 13 % slower at SF7, mode 0
        // at SF9: 6 % slower.)  The last tile reloads a valid window: a
        // dead unit's is frame w's first.
        const cf32* nsrc = nullptr;
        next_pos();
        // (measured alternative: early in modes 1/2 too, except in the tile
        // before an EB tile, whose scans need the registers: 4-5x slower,
        // the two staging variants of one loop spilled)
        constexpr bool early = EARLY;
        if (early) {
            next_ctx();
            nsrc = A.iq + (unsigned long long)nc.f * A.frame_samples + nc.base + fl;
            iq_check(A, nc.f, (long long)nc.base);
            iq_check(A, nc.f, (long long)nc.base + N - 1);
        }
        // an EB tile (estimate units of one group, and dead units): each
        // unit's frame max-abs, scanned ahead, first
        const unsigned long long emask = __ballot(kind == kUnitEst);
        float amax;
        if (kEbMax && spec && emask) {
            // EST_MAX: an EB tile holds both estimate units of each of its
            // frames, in teams 2j and 2j + 1 (2 LPS lanes).  The samples are
            // staged [dechirped], the frame's max(|I|,|Q|) over them folded
            // (v_max3, and NaN when one is non-finite, like wave_maxabs: such
            // a frame goes to k_post's exact re-run), then the normalisation
            // applied: the same operations on the same operands as staging
            // with the scanned maximum, without reading the two symbols
            // twice or blocking on a scan.  (Modes 1/2 only, so never with
            // EARLY, the mode-0 in-staging reload of `raw`, which this
            // staging does not do.)
            static_assert(!EARLY || (MODE & 3) == LPHY_MODE_DEMODULATE, "EST_MAX staging has no EARLY reload");
            const cf32* dl = down + (c.base & (N - 1)) + fl;
            float fm = 0.0f;
            cf32 sum = czero();
#pragma unroll
            for (int e = 0; e < G::E; ++e) {
                const int ce = first_pass_index<SF>(e, 0);
                cf32 p = raw[e];
                if constexpr (DECH) p = cmul(p, dl[ce]);
                fm = max3_abs(fm, p.x, p.y);
                sum = sum + p;
                v[e] = p;
            }
            bool bad = !(sum.x == sum.x && sum.y == sum.y) || !(fm <= 3.40282347e38f);
#pragma unroll
            for (int off = G::LPS; off >= 1; off >>= 1) {
                const float o = __shfl_xor(fm, off, 64);
                fm = o > fm ? o : fm;
            }
            const unsigned long long bm = __ballot(bad);
            const unsigned pair = (unsigned)(lane / (2 * G::LPS));
            constexpr unsigned long long PM = 2 * G::LPS >= 64 ? ~0ull : ((1ull << (2 * G::LPS)) - 1ull);
            bad = ((bm >> (pair * 2 * G::LPS)) & PM) != 0;
            const float mx = bad ? __builtin_nanf("") : fm;
            if (kind == kUnitEst) {
                const lphy_frame_meta nm = norm_meta_hot(mx, true, A.no_scratch);
                c.scale = nm.scale;
                c.live = nm.status == 0;
                if (su == 0 && lam == 0) ringmx[wv][slot_of(fk)] = mx;
            }
            c.ok = kind == kUnitEst && c.live;
            const float* wl = win + fl;
#pragma unroll
            for (int e = 0; e < G::E; ++e) {
                cf32 y = c.ok ? cscale(v[e], c.scale) : czero();
                if constexpr ((MODE & kWinBit) != 0) y = cscale(y, wl[first_pass_index<SF>(e, 0)]);
                v[e] = y;
            }
            amax = 0.0f;
        } else if (emask) {
            if (kind == kUnitEst) {
                if ((MODE & 3) != LPHY_MODE_DEMODULATE) {
                    const lphy_frame_meta nm = norm_meta_hot(ringmx[wv][slot_of(fk)], true, A.no_scratch);
                    c.scale = nm.scale;
                    c.live = nm.status == 0;
                }
                c.ok = c.live;  // estimate this unit (else stage zeros)
            }
            amax = early ? stage_fast<SF, MODE, true, true>(v, raw, c, fl, down, win, rt, thl, kind != kUnitSym, nsrc)
                         : stage_fast<SF, MODE, true, false>(v, raw, c, fl, down, win, rt, thl, kind != kUnitSym, nsrc);
        } else {
            amax = early ? stage_fast<SF, MODE, false, true>(v, raw, c, fl, down, win, rt, thl, false, nsrc)
                         : stage_fast<SF, MODE, false, false>(v, raw, c, fl, down, win, rt, thl, false, nsrc);
        }
        if constexpr ((MODE & 3) == LPHY_MODE_DEMODULATE) {
            if constexpr (G::LPS <= 16) {
                amax = team_max_first<SF>(amax);  // the certificate reads lane lam == 0
            } else {
#pragma unroll
                for (int off = G::LPS / 2; off >= 1; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
            }
        } else {
            // normalised frame: max(|I|,|Q|) <= 1 (see fast_certified); under
            // speculation the frame end confirms it or settles the frame
            if (spec) {
                // the symbol's [dechirped] samples, as the pre-scan folds them
                const float lm = kind == kUnitSym && c.ok ? amax : 0.0f;
                if (fk & 1) sp_mx1 = fmaxf(sp_mx1, lm);
                else sp_mx0 = fmaxf(sp_mx0, lm);
            }
            amax = 1.0f;
        }
        team_sync<SF>();

        if (!early) {
            // next tile's context and IQ (in flight during the FFT)
            next_ctx();
            if (t + 1 < ntiles) {
                const cf32* lsrc = A.iq + (unsigned long long)nc.f * A.frame_samples + nc.base + fl;
#pragma unroll
                for (int e = 0; e < G::E; ++e) {
                    iq_check(A, nc.f, (long long)nc.base + fl + first_pass_index<SF>(e, 0));
                    raw[e] = ld_iq(lsrc + first_pass_index<SF>(e, 0));
                }
            }
        }

        // tiles of symbol units only: magnitude-only transform (fft_tile TRIV)
        // (measured alternative: a packed-key max/min tournament for the top
        // two, 3 % slower than this ordered scan)
        // the transform and the top two at issue priority 1: of the two
        // waves on a SIMD, the one in its arithmetic segment issues first
        // (the other is mostly in staging, bookkeeping or waiting on loads),
        // so each wave's compute segment ends, and its next loads go out,
        // sooner.  Same-box A/B: fused 1.037 -> 1.016 ms (three rounds;
        // priority over the transform alone: 1.021)
        __builtin_amdgcn_s_setprio(1);
        if (emask) fft_tile<SF, false, false, true>(v, lds, slot, lam, twl);
        else fft_tile<SF, true, false, true>(v, lds, slot, lam, twl);

        // (SF <= 8: reduced toward lane lam == 0 by DPP, the only lane that
        // reads it; above, every lane of the team holds it)
        // (symbol-only tiles: keyed top two, a bound that only certified
        // symbols use; estimate units need the detector's exact argmax)
        ArgMax2 b2;
        if constexpr (G::LPS <= 16) {
            if (emask) b2 = team_argmax2_first<SF>(local_argmax2<SF>(v, lam));
            else b2 = team_argmax2_keyed_first<SF>(v, lam);
        } else {
            b2 = symbol_argmax2<SF>(local_argmax2<SF>(v, lam));
        }
        __builtin_amdgcn_s_setprio(0);
        ArgMax best{b2.v, b2.i};
        if (emask) {
            // detector outputs of the estimate units (LoRaDetector.hpp:60-71)
            if (kind == kUnitEst) {
#pragma unroll
                for (int e = 0; e < G::E; ++e) lds[G::addr(slot, bin_of<SF>(e, lam))] = v[e];
            }
            team_sync<SF>();
            // a NaN bin may hide an Annex G product: exact re-run (k_post)
            const unsigned long long nanm = __ballot(kind == kUnitEst && c.ok && fft_has_nan<SF>(v));
            if (kind == kUnitEst && lam == 0) {
                UnitResult& ur = ures[wv][fk % F][su];
                ur = c.ok ? unit_result<SF>(lds, slot, best) : UnitResult{0, 0, 0.0f, 0.0f};
                ur.nan = ((nanm >> (slot * G::LPS)) & ((G::LPS == 64) ? ~0ull : ((1ull << G::LPS) - 1))) != 0;
            }
            team_sync<SF>();  // slot reads done before a re-check restages
        }
        // symbols the certificate does not cover: exact per-sample rotation
        // certificate (fast_certified, written out so that the speculation
        // below reuses its lead and bound): B is linear in amax
        const float cb1 = cert_bound<SF>(c.rate, c.start, 1.0f, RLDS ? 0.0f : 6.0f);
        const float cgap = cert_gap(b2);
        const bool cert = cgap > 4.0f * (cb1 * amax) && (float)N * 1.41421366f * amax * 1.0001f < 1e18f &&
                          amax >= 1e-20f && b2.v >= 1e-30f && b2.v < 1e30f;
        const bool redo = kind == kUnitSym && c.ok &&
                          (exact_only || !fast_applies<SF, MODE>(c, c.toff) || !cert);
        // (no exact re-run here: it would keep a second transform's state
        // live beside the prefetch.  The symbol is left as kSymRecheck and
        // its frame as kStatusRecheck; k_post recomputes it exactly.)
        if (spec && kind == kUnitSym && c.ok) {
            // a NaN sample reaches every bin (fft_has_nan); the certificate's
            // lead over its bound, for the frame end's rate check (from the
            // team's first lane, which holds the team's top two)
            const cf32 q = v[0] * v[0];
            const float q2 = q.x + q.y;
            unsigned fl = q2 == q2 ? 0u : 1u;
            float r = kBig;
            if (lam == 0) {
                // a lower bound of the lead / bound ratio (v_rcp within 1 ulp)
                if (redo) fl |= 2u;
                else r = cgap * __builtin_amdgcn_rcpf(cb1) * (1.0f - 4.0f * kU);
            }
            if (fk & 1) {
                sp_fl1 |= fl;
                sp_r1 = fminf(sp_r1, r);
            } else {
                sp_fl0 |= fl;
                sp_r0 = fminf(sp_r0, r);
            }
        }
        if (kind == kUnitSym && lam == 0) {
            // sw0 / sw1 also for frames that are not demodulated (0, as the
            // separate-launch path leaves them)
            const uint16_t out = redo ? kSymRecheck : (uint16_t)best.i;
            if (c.have_sync && c.s < 2) store_symbol(A, c, c.ok ? out : (uint16_t)0);
            else if (c.ok) store_symbol(A, c, out);
            if (redo) A.meta[c.f].status = kStatusRecheck;
        }
        team_sync<SF>();  // slot reads (and ures) done
#ifdef LPHY_PROFILE_PHASES
        pf = clock64();
#endif
        // the frames whose last estimate unit was in this tile: each folds on
        // the first lane of the team holding that unit (F lanes at once)
        const bool my_fold = kind == kUnitEst && su == U - 1 && lam == 0;
        const unsigned long long fmask = __ballot(my_fold);
        if (my_fold) {
            const unsigned sl = slot_of(fk);
            lphy_frame_meta m{};
            m.scale = 1.0f;
            m.have_sync = 1;
            if ((MODE & 3) != LPHY_MODE_DEMODULATE) m = norm_meta_hot(ringmx[wv][sl], true, A.no_scratch);
            if (m.status == 0) {
                EstFold fold;
                bool nan = false;
#pragma unroll
                for (unsigned u = 0; u < U; ++u) {
                    const UnitResult r = ures[wv][fk % F][u];
                    nan |= r.nan != 0;
                    if (r.valid) fold.add(r.idx, r.findex, 0, r.phase);
                    else fold.add(0, 0.0f, 0, 0.0f);
                }
                fold.finish(m, (int)U, N, 1);
                if (nan) m.status = kStatusFixup;
            }
            ring[wv][sl] = float4{m.rate, m.scale, __int_as_float(m.t_off),
                                  __uint_as_float((m.status == 0 ? 1u : 0u) | 2u)};
            bound_check(w + fk * W, (long long)A.frames);
            meta_put_est(&A.meta[w + fk * W], m);
        }
        team_sync<SF>();
        // the folded frames' rotation tables, first read two tiles later
        // (their slots' previous frames, of group g - 1, have no units left)
        for (unsigned long long fm = fmask; fm; fm &= fm - 1) {
            const unsigned kf = (unsigned)__shfl((int)fk, __ffsll((long long)fm) - 1, 64);
            const unsigned sl = slot_of(kf);
            const float4 r = ring[wv][sl];
            if (__float_as_uint(r.w) & 1u) {
                if constexpr (RLDS) {
                    build_rtab<SF, MODE>(rtab[wv][sl], r.x, r.y, __float_as_int(r.z), down, win, lane);
                } else {
                    cf32* tb = rtab2[wv][sl];
                    for (int j = lane; j < 64 + N / 64; j += 64) {
                        const int ph = j < 64 ? j : 64 * (j - 64);
                        float sn, cs;
                        lphy_libm::sincosf_exact(r.x * (float)ph, &sn, &cs);
                        cf32 t = cf32{cs, sn};
                        if constexpr ((MODE & 3) != LPHY_MODE_DEMODULATE)
                            if (j < 64) t = cscale(t, r.y);
                        tb[j] = t;
                    }
                }
            }
        }
        // speculative normalisation: the tile holding a frame's last symbol
        // unit closes the frame (its other symbols are in earlier tiles)
        if (spec) {
            const unsigned long long fe = __ballot(kind == kUnitSym && su == S - 1);
            if (fe) {
                const unsigned kf = (unsigned)__shfl((int)fk, __ffsll((long long)fe) - 1, 64);
                const bool p1 = (kf & 1) != 0;
                float m = p1 ? sp_mx1 : sp_mx0, r = p1 ? sp_r1 : sp_r0;
                const unsigned fl = p1 ? sp_fl1 : sp_fl0;
                if (p1) { sp_mx1 = 0.0f; sp_r1 = kBig; sp_fl1 = 0u; }
                else { sp_mx0 = 0.0f; sp_r0 = kBig; sp_fl0 = 0u; }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    m = fmaxf(m, __shfl_xor(m, off, 64));
                    r = fminf(r, __shfl_xor(r, off, 64));
                }
                const bool nan = __ballot(fl & 1u) != 0, open = __ballot(fl & 2u) != 0;
                const float4 rr = ring[wv][slot_of(kf)];
                if (__float_as_uint(rr.w) & 1u) {
                    const unsigned f = w + kf * W;
                    bound_check(f, (long long)A.frames);
                    const unsigned cnt = DECH ? S * N : (unsigned)A.frame_samples;
                    const unsigned end = covered_end(S, N, cnt, __float_as_int(rr.z));
                    bool fbad = false;
                    if (end < cnt) m = fmaxf(m, wave_range_maxabs<SF, MODE>(A, f, end, cnt, down, fbad));
                    if (lane == 0) {
                        const float mx01 = ringmx[wv][slot_of(kf)];
                        const float mt = fmaxf(m, mx01);
                        const lphy_frame_meta mg = norm_meta(mx01, true, 0), me = norm_meta(mt, true, 0);
                        if (nan || fbad || !(mt <= 3.40282347e38f)) {
                            A.meta[f].status = kStatusFixup;
                        } else if (me.scale != mg.scale || me.normalised != mg.normalised) {
                            A.meta[f].cfo = mt;
                            A.meta[f].time_offset = r;
                            A.meta[f].status = open ? kStatusSettleRecheck : kStatusSettle;
                        }
                    }
                }
            }
        }
        g = ng_;
        tg = ntg;
        dj = ndj;
        ds = nds;
        kind = nkind;
        fk = nfk;
        su = nsu;
        c = nc;
#ifdef LPHY_PROFILE_PHASES
        const unsigned long long p9 = clock64();
        if (emask) { ph_mix += p9 - p0; ph_fold += p9 - pf; ++n_mix; }
        else ph_sym += p9 - p0;
#endif
    }
#ifdef LPHY_PROFILE_PHASES
    if (lane == 0) {
        atomicAdd(&A.counters[kCtrClocks + 0], ph_mix);
        atomicAdd(&A.counters[kCtrClocks + 1], ph_sym);
        atomicAdd(&A.counters[kCtrClocks + 2], ph_fold);
        atomicAdd(&A.counters[kCtrClocks + 3], n_mix);
    }
#endif
}

}  // namespace
