// lphy_post.h — what runs after the symbol kernels of a call: the exact
// re-runs of the frames and symbols they flagged (exact_frame,
// recheck_frames, settle_frames; k_spec_settle closes the SF 11-12
// separate launches' speculation) and, in the same launch, the finalisation
// (k_post).  The passes these share are defined once, in lphy_demod.h:
// workgroup_max (the max-abs reduction), exact_symbol (a symbol with the
// per-sample Annex G rotation), settle_verdict (the certificate check of a
// speculatively normalised frame) and, in k_spec_settle, estimate_unit (an
// estimate symbol: staging, exact FFT, bins kept).  exact_frame and
// settle_frames hold estimate_unit's pass written out (inside k_post the
// helper cost registers): a change to it is made there too.
#pragma once
#include "lphy_demod.h"
#include "lphy_final.h"

namespace {

// ---------------------------------------------------------------------------
// Exact re-run of one frame by a whole 256-thread workgroup (k_post): the
// reference's arithmetic with its Annex G complex products (cmul_x)
// everywhere - max-abs (LoRaDemod.cpp:60-78), estimate (LoRaDemod.cpp:80-140
// / phy.cpp:81-148), every symbol (LoRaDemod.cpp:142-176 / phy.cpp:204-238).
// Frames get here only when a hot kernel met a non-finite value (status
// kStatusFixup), so this path favours plainness over speed.
// ---------------------------------------------------------------------------
template <int SF>
struct PostShared {
    cf32 lds[Geo<SF>::T * Geo<SF>::SSTRIDE];
    ArgMax red[kTile / 64];
    UnitResult units[Geo<SF>::T];  // exact_frame: a chunk's estimate units ...
    float upow[Geo<SF>::T];        // ... and, osr > 1, their detector powers
    float wmax[kTile / 64];
    lphy_frame_meta m;
    uint16_t sw[2];
    unsigned list[kTile];
    unsigned listf[kTile];
    unsigned count;
    UnitResult ures2[kTile][2];  // settle_frames, k_spec_settle: both estimate units of each listed frame
};

template <int SF, int MODE>
__device__ void exact_frame(const DemodArgs& A, unsigned f, PostShared<SF>& sh) {
    using G = Geo<SF>;
    constexpr int N = G::N, T = G::T;
    const int tid = threadIdx.x;
    const int slot = tid / G::LPS, lam = tid % G::LPS;
    const cf32* fr = A.iq + (unsigned long long)f * A.frame_samples;
    const unsigned long long step = (unsigned long long)N * A.osr;
    const bool have_sync = A.total_syms >= 2;
    // (1) normalisation (modes 1, 2; mode 0 keeps mx = 0: scale 1)
    float mx = 0.0f;
    if (MODE != LPHY_MODE_DEMODULATE) {
        const unsigned long long count = MODE == LPHY_MODE_DECHIRP_LORA_DEMODULATE
                                             ? A.total_syms * N : A.frame_samples;
        for (unsigned long long i = tid; i < count; i += kTile) {
            cf32 x = fr[i];
            if (MODE == LPHY_MODE_DECHIRP_LORA_DEMODULATE) x = cmul_x(x, A.down[i & (N - 1)]);
            maxabs_acc(mx, x);
        }
        mx = workgroup_max(mx, sh.wmax);
    }
    if (tid == 0) {
        sh.m = norm_meta(mx, have_sync, A.no_scratch);
        sh.sw[0] = sh.sw[1] = 0;
    }
    __syncthreads();
    // (2) estimate: units (symbol, osr phase) in chunks of T, folded in
    // order by thread 0 (the separate k_estimate's unpacked path)
    EstFold fold;
    const int U = A.est_units;
    const bool tie_low = MODE != LPHY_MODE_DEMODULATE;
    for (int c0 = 0; c0 < U && sh.m.status == 0; c0 += T) {
        const lphy_frame_meta m = sh.m;
        const int u = c0 + slot;
        const bool live = u < U;
        const int s = live ? u / A.osr : 0, t = live ? u % A.osr : 0;
        const Stage<SF> st(slot, lam);
#pragma unroll
        for (int e = 0; e < G::E; ++e) {
            const int i = lam + e * G::LPS;
            cf32 x = czero();
            if (live) x = est_sample(A, fr, (unsigned long long)s * step + t + (unsigned long long)i * A.osr, i, N, m);
            st.put(sh.lds, e, x);
        }
        __syncthreads();
        cf32 v[16];
        fft_tile<SF, false, true>(v, sh.lds, slot, lam, A.tw);
#pragma unroll
        for (int e = 0; e < G::E; ++e) sh.lds[G::addr(slot, bin_of<SF>(e, lam))] = v[e];
        const ArgMax best = symbol_argmax<SF>(local_argmax<SF>(v, lam), sh.red);
        __syncthreads();
        if (lam == 0) {
            sh.units[slot] = live ? unit_result<SF>(sh.lds, slot, best) : kNoUnit;
            sh.upow[slot] = live && A.osr > 1 ? detector_power(best.v > 0.0f ? best.v : 0.0f, A.power_scale) : 0.0f;
        }
        __syncthreads();
        if (tid == 0) {
            const int nu = U - c0 < T ? U - c0 : T;
            for (int k = 0; k < nu; ++k) fold.unit(sh.units[k], A.osr > 1 ? sh.upow[k] : 0.0f, A.osr, tie_low);
        }
        __syncthreads();
    }
    if (tid == 0 && sh.m.status == 0) fold.finish(sh.m, U / A.osr, N, A.osr);
    __syncthreads();
    // (3) symbols, T per tile, exact per-sample rotation
    const lphy_frame_meta m = sh.m;
    const unsigned S = (unsigned)A.total_syms;
    for (unsigned s0 = 0; s0 < S; s0 += T) {
        const unsigned s = s0 + slot;
        const bool live = s < S;
        const SymCtx c = sym_ctx<true>(A, f, live ? s : 0, live, N, m);
        const ArgMax best = exact_symbol<SF, MODE>(A, fr, c, sh.lds, slot, lam, sh.red);
        if (lam == 0 && live) {
            if (c.have_sync && s < 2) sh.sw[s] = c.ok ? (uint16_t)best.i : (uint16_t)0;
            else if (c.ok) A.syms[(unsigned long long)f * A.out_per_frame + (c.have_sync ? s - 2 : s)] = (uint16_t)best.i;
        }
        __syncthreads();
    }
    if (tid == 0) {
        lphy_frame_meta r = sh.m;
        r.sw0 = sh.sw[0];
        r.sw1 = sh.sw[1];
        A.meta[f] = r;
    }
    __syncthreads();
}

// Symbols the fused kernel's certificate left open (kSymRecheck in the
// output, frame status kStatusRecheck) among the workgroup's frames fb ..
// fb + kTile - 1: the reference's per-sample rotation with its Annex G
// products, T (frame, symbol) pairs per tile; the frames' offsets from the
// hot kernel stand (only symbol units were uncertified).  Thread t scans
// frame fb + t when `mine` (its status is kStatusRecheck).
template <int SF, int MODE>
__device__ void recheck_frames(const DemodArgs& A, unsigned long long fb, bool mine, PostShared<SF>& sh) {
    using G = Geo<SF>;
    constexpr int N = G::N, T = G::T;
    const int tid = threadIdx.x;
    const int slot = tid / G::LPS, lam = tid % G::LPS;
    const unsigned S = (unsigned)A.total_syms;
    unsigned cur = mine ? 0u : S;  // this thread's scan position in its frame
    unsigned long long done = 0;
    lphy_frame_meta mm{};
    if (mine) mm = A.meta[fb + tid];
    // Rows of up to 64 aligned data symbols (every bench shape): the row's
    // sentinels as a bit mask from its words loaded at once (one memory round
    // trip per frame; a load per symbol, then per 8, made the scan k_post's
    // longest part at mode A's ~6,600 re-runs per SF 7 launch)
    const bool hs0 = mm.have_sync != 0;
    const uint16_t* const out0 = A.syms + (fb + (unsigned)tid) * A.out_per_frame;
    const unsigned ofs0 = hs0 ? 2u : 0u;
    const bool fastscan = A.out_per_frame <= 64 && (A.out_per_frame & 7) == 0 && ((unsigned long long)out0 & 15ull) == 0ull &&
                          S == A.out_per_frame + ofs0;
    unsigned long long smask = 0;  // bit b: data symbol b is a sentinel; bits 62/63: sw0/sw1 (shifted below)
    unsigned smask_sync = 0;
    if (mine && fastscan) {
        uint4 q[8];
#pragma unroll
        for (int w = 0; w < 8; ++w)
            if (w * 8 < (int)A.out_per_frame) q[w] = reinterpret_cast<const uint4*>(out0)[w];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            if (w * 8 >= (int)A.out_per_frame) break;
            const unsigned x[4] = {q[w].x, q[w].y, q[w].z, q[w].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if ((x[k] & 0xffffu) == kSymRecheck) smask |= 1ull << (8 * w + 2 * k);
                if ((x[k] >> 16) == kSymRecheck) smask |= 1ull << (8 * w + 2 * k + 1);
            }
        }
        if (hs0) smask_sync = (mm.sw0 == kSymRecheck ? 1u : 0u) | (mm.sw1 == kSymRecheck ? 2u : 0u);
    }
    for (;;) {
        __syncthreads();
        if (tid == 0) sh.count = 0;
        __syncthreads();
        // collect up to kTile open symbols
        if (cur < S && fastscan) {
            for (;;) {
                // the next sentinel at or after cur
                unsigned next = S;
                if (cur < ofs0) {
                    const unsigned sm = smask_sync >> cur;
                    if (sm) next = cur + (unsigned)(__ffs(sm) - 1);
                }
                if (next == S) {
                    const unsigned d = cur > ofs0 ? cur - ofs0 : 0u;
                    const unsigned long long m = d < 64 ? (smask >> d) << d : 0ull;
                    if (m) next = ofs0 + (unsigned)(__ffsll((long long)m) - 1);
                }
                cur = next;
                if (cur >= S) break;
                const unsigned k = atomicAdd(&sh.count, 1u);
                if (k >= kTile) break;  // full: this symbol goes in the next round
                sh.list[k] = cur;
                sh.listf[k] = (unsigned)tid;
                ++cur;
            }
        } else if (cur < S) {
            const unsigned long long f = fb + tid;
            const bool hs = mm.have_sync != 0;
            const uint16_t* out = A.syms + f * A.out_per_frame;
            for (; cur < S; ++cur) {
                const uint16_t v = (hs && cur < 2) ? (cur == 0 ? mm.sw0 : mm.sw1) : out[hs ? cur - 2 : cur];
                if (v != kSymRecheck) continue;
                const unsigned k = atomicAdd(&sh.count, 1u);
                if (k >= kTile) break;  // full: this symbol goes in the next round
                sh.list[k] = cur;
                sh.listf[k] = (unsigned)tid;
            }
        }
        __syncthreads();
        const unsigned n = sh.count < kTile ? sh.count : kTile;
        if (n == 0) break;
        done += n;
        for (unsigned k0 = 0; k0 < n; k0 += T) {
            const unsigned k = k0 + (unsigned)slot;
            const bool live = k < n;
            const unsigned sy = live ? sh.list[k] : 0;
            const unsigned long long f = fb + (live ? sh.listf[k] : 0);
            lphy_frame_meta m = A.meta[f];
            m.status = 0;
            const SymCtx c = sym_ctx<true>(A, (unsigned)f, sy, live, N, m);
            const ArgMax best = exact_symbol<SF, MODE>(A, A.iq + f * A.frame_samples, c, sh.lds, slot, lam, sh.red);
            if (lam == 0 && live) store_symbol(A, c, (uint16_t)best.i);
            __syncthreads();
        }
    }
    if (tid == 0 && done) atomicAdd(&A.counters[kCtrRecheck], done);
}

// Frames k_frames demodulated under a speculative normalisation that the
// frame's later samples overturned (status kStatusSettle[Recheck]), among the
// workgroup's frames fb .. fb + kTile - 1 (thread t: frame fb + t, `mine`).
// Their two estimate symbols are transformed again, T/2 frames per tile, with
// the exact normalisation (as estimate_unit), and settle_verdict folds them into
// the exact offsets and decides whether the symbols stand or the frame is
// re-run whole (kStatusFixup).
template <int SF, int MODE>
__device__ void settle_frames(const DemodArgs& A, unsigned long long fb, bool mine, PostShared<SF>& sh) {
    using G = Geo<SF>;
    constexpr int N = G::N, T = G::T;
    const int tid = threadIdx.x;
    const int slot = tid / G::LPS, lam = tid % G::LPS;
    if (tid == 0) sh.count = 0;
    __syncthreads();
    if (mine) sh.list[atomicAdd(&sh.count, 1u)] = (unsigned)tid;
    __syncthreads();
    const unsigned n = sh.count;
    // units (frame k, estimate symbol s) = 2k + s, T per tile pass
    for (unsigned u0 = 0; u0 < 2 * n; u0 += T) {
        const unsigned u = u0 + (unsigned)slot;
        const bool live = u < 2 * n;
        const unsigned k = live ? u / 2 : 0u, s = u & 1u;
        const unsigned long long f = fb + (live ? sh.list[k] : 0u);
        const lphy_frame_meta m = norm_meta(A.meta[f].cfo, true, 0);  // cfo holds the max-abs
        const cf32* fr = A.iq + f * A.frame_samples;
        const Stage<SF> st(slot, lam);
#pragma unroll
        for (int e = 0; e < G::E; ++e) {
            const int i = lam + e * G::LPS;
            st.put(sh.lds, e, live ? est_sample(A, fr, (unsigned long long)s * N + (unsigned)i, i, N, m) : czero());
        }
        __syncthreads();
        cf32 v[16];
        fft_tile<SF, false, true>(v, sh.lds, slot, lam, A.tw);
#pragma unroll
        for (int e = 0; e < G::E; ++e) sh.lds[G::addr(slot, bin_of<SF>(e, lam))] = v[e];
        const ArgMax best = symbol_argmax<SF>(local_argmax<SF>(v, lam), sh.red);
        __syncthreads();
        if (lam == 0 && live) sh.ures2[k][s] = unit_result<SF>(sh.lds, slot, best);
        __syncthreads();
    }
    if ((unsigned)tid < n) {
        const unsigned long long g = fb + sh.list[tid];
        const lphy_frame_meta sm = A.meta[g];
        // the record holds {cfo: the max-abs, time_offset: the least certificate ratio}
        A.meta[g] = settle_verdict<SF>(sm, norm_meta(sm.cfo, true, 0), sh.ures2[tid][0], sh.ures2[tid][1],
                                       sm.cfo * sm.scale, sm.time_offset, sm.status == kStatusSettleRecheck);
    }
    __syncthreads();
}

// Separate launches with spec_big (SF 11-12, modes 1/2): the frame-end
// check k_frames makes in-kernel, one workgroup per frame (so the exact
// estimates of settled frames run in parallel).  The samples no symbol
// window covers are scanned; the frame's true max-abs then confirms the
// two-symbol normalisation, or - NaN / inf - sends the frame to k_post's
// exact re-run, or settles it here as settle_frames does: both estimate
// units again with the exact scale (estimate_unit), then settle_verdict
// against the exact rate, else the exact re-run.
template <int SF, int MODE>
__global__ __launch_bounds__(kTile) void k_spec_settle(DemodArgs A) {
    using G = Geo<SF>;
    constexpr int N = G::N, T = G::T;
    constexpr bool DECH = MODE == LPHY_MODE_DECHIRP_LORA_DEMODULATE;
    __shared__ PostShared<SF> sh;
    const unsigned long long f = blockIdx.x;
    const int tid = threadIdx.x;
    const lphy_frame_meta m = A.meta[f];
    if (!(m.status == 0 || m.status == kStatusRecheck)) return;  // uniform
    const unsigned S = (unsigned)A.total_syms;
    const unsigned cnt = DECH ? S * N : (unsigned)A.frame_samples;
    const unsigned end = covered_end(S, N, cnt, m.t_off);
    const cf32* fr = A.iq + f * A.frame_samples;
    float frag = 0.0f;
    bool fbad = false;
    if (end < cnt) {
        float mx = 0.0f;
        bool bad = false;
        for (unsigned i = end + (unsigned)tid; i < cnt; i += kTile) {
            cf32 x = fr[i];
            if constexpr (DECH) x = cmul(x, A.down[i & (N - 1)]);
            bad |= !(__builtin_isfinite(x.x) && __builtin_isfinite(x.y));
            maxabs_acc(mx, x);
        }
        fbad = __syncthreads_or(bad);
        frag = workgroup_max(mx, sh.wmax);
    }
    const uint4 r = A.spec_big[f];
    const float mx01 = __uint_as_float(r.x);
    const float mt = fmaxf(fmaxf(mx01, __uint_as_float(r.y)), frag);
    const lphy_frame_meta mg = norm_meta(mx01, true, 0), me = norm_meta(mt, true, 0);
    if ((r.w & 1u) || fbad || !(mt <= 3.40282347e38f)) {
        if (tid == 0) A.meta[f].status = kStatusFixup;
        return;
    }
    if (me.scale == mg.scale && me.normalised == mg.normalised) return;  // confirmed
    // settle: the two estimate units, T per pass
    const int slot = tid / G::LPS, lam = tid % G::LPS;
    for (unsigned u0 = 0; u0 < 2; u0 += T) {
        const unsigned s = u0 + (unsigned)slot;
        const bool live = s < 2;
        const ArgMax best = estimate_unit<SF>(A, fr, (int)s, 0, 1, me, live, sh.lds, slot, lam, A.tw, sh.red);
        if (lam == 0 && live) sh.ures2[0][s] = unit_result<SF>(sh.lds, slot, best);
        __syncthreads();
    }
    if (tid == 0)
        A.meta[f] = settle_verdict<SF>(m, me, sh.ures2[0][0], sh.ures2[0][1], mt * m.scale, __uint_as_float(r.z),
                                       (r.w & 2u) || m.status == kStatusRecheck);
}

// After the symbol kernels: the exact re-run of the frames they flagged
// (kStatusFixup: whole frame; kStatusRecheck: the open symbols), then (fin)
// the per-frame finalisation (lphy_final.h: the workgroup's rows staged
// through LDS, finalize_block, else a thread per frame).
template <int SF>
union PostLds {  // the exact re-runs' workspace, then the finalisation's staging
    PostShared<SF> sh;
    FinStage fs;
};
template <int SF, int MODE>
__global__ __launch_bounds__(kTile) void k_post(DemodArgs A, FinalArgs F, int fix, int fin) {
    __shared__ PostLds<SF> L;
    PostShared<SF>& sh = L.sh;
    __shared__ unsigned flist[kTile];
    __shared__ unsigned fcount;
    const unsigned long long f = (unsigned long long)blockIdx.x * kTile + threadIdx.x;
    if (fix) {
        int st = f < A.frames ? A.meta[f].status : 0;
        const bool settle = st == kStatusSettle || st == kStatusSettleRecheck;
        if (__syncthreads_or(settle)) {
            settle_frames<SF, MODE>(A, (unsigned long long)blockIdx.x * kTile, settle, sh);
            __syncthreads();
            if (f < A.frames) st = A.meta[f].status;
        }
        const bool fixup = st == kStatusFixup;
        const bool recheck = st == kStatusRecheck;
        if (__syncthreads_or(fixup)) {
            if (threadIdx.x == 0) fcount = 0;
            __syncthreads();
            if (fixup) flist[atomicAdd(&fcount, 1u)] = (unsigned)f;
            __syncthreads();
            const unsigned n = fcount;
            for (unsigned k = 0; k < n; ++k) exact_frame<SF, MODE>(A, flist[k], sh);
            // every symbol of these frames was re-run exactly (lphy_hip_recheck_count)
            if (threadIdx.x == 0) atomicAdd(&A.counters[kCtrRecheck], (unsigned long long)n * A.total_syms);
        }
        if (__syncthreads_or(recheck)) {
            recheck_frames<SF, MODE>(A, (unsigned long long)blockIdx.x * kTile, recheck, sh);
            __syncthreads();
            if (recheck) A.meta[f].status = 0;
        }
    }
    if (!fin) return;
    if (fix) __syncthreads();  // the re-runs are done with the shared workspace
    if (finalize_block(F, (unsigned long long)blockIdx.x * kTile, L.fs)) return;
    if (f < A.frames) finalize_frame(F, f);
}

}  // namespace
