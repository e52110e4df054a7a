// lphy_mod.h — bit-exact lora_modulate (k_mod_*, the producer of synthetic
// IQ) and compensate_offsets (k_comp_*).  Independent of the spreading
// factor: only lphy_hip.hip includes it.
#pragma once
#include "lphy_args.h"
#include "libm_exact.h"
#include "lphy_demod.h"    // (round_to_int)
#include "lphy_testing.h"  // (the device counter slots)

namespace {

// ---------------------------------------------------------------------------
// lora_modulate (LoRaMod.cpp:8-43 + ChirpGenerator.hpp:24-51), bit-exact.
// The phase accumulator is one float recurrence through the whole frame
// (phase += f, f += fStep with one wrap per symbol), so some thread has to
// walk it in order.  Batches (many symbols): pass 1, one thread per frame,
// walks it and records the phase at each symbol start; pass 2, one thread
// per symbol, regenerates its samples from there.  Few symbols (a single
// frame, the reference's per-packet loop): pass 2 would be a handful of
// threads each walking N samples with a sincos per step, so instead each
// symbol's frequency sequence is built in parallel (k_mod_freq), one thread
// per frame adds them up in order (k_mod_accumulate, one dependent add per
// sample, loads a block ahead) and a sample-parallel pass turns the phases into IQ
// (k_mod_sincos).
// ---------------------------------------------------------------------------
struct ModArgs {
    const uint16_t* syms;
    cf32* iq;
    float* phase0;           // frames * (nsyms + 2) phase at symbol start
    float* phases;           // (walk) frames * (nsyms + 2) * N * osr phases
    unsigned long long frames, nsyms;
    int N, osr;
    float bws, ampl;
    uint8_t sync;
    unsigned long long* slow;  // (k_mod_fast) frames that took the serial walk
    int force_serial;          // (test build) k_mod_fast takes its serial walk for every frame
    struct ModFastG* mfg;      // (k_mod_fast GROWS, split) per frame: windows, pivots, chain start
    unsigned char* mft;        // (ditto) per frame: T, kModFastSyms x kModFastWin
    int blk;                   // 0: phases row after row; else (split form) rows interleaved by
                               // 16-byte groups, blk = rows per frame (k_mod_fast GROWS)
};

__device__ __forceinline__ float mod_f0(const ModArgs& A, unsigned long long f, unsigned long long s) {
    uint16_t v;
    if (s < 2) {
        int sf = 0;
        while ((1 << sf) < A.N) ++sf;
        const unsigned sh = sf > 4 ? sf - 4 : 0;
        v = s == 0 ? (uint16_t)((A.sync >> 4) << sh) : (uint16_t)((A.sync & 0x0f) << sh);
    } else {
        v = A.syms[f * A.nsyms + (s - 2)];
    }
    return (2.0f * kPi * (float)v * A.bws) / ((float)A.N * (float)A.osr);
}

// Eight steps of the chirp recurrence (ChirpGenerator.hpp:39-43): f += fStep,
// wrap once past fMax, phase += f; every rounding as the reference's loop.
// f only grows between wraps, so when the eighth f is not past fMax none of
// the eight is and the wrap test is skipped.
struct ChirpWalk {
    float fmin, fmax, fstep;
    __device__ __forceinline__ void step8(float& fr, float& phase, float p[8]) const {
        float g[8];
        float x = fr;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            x += fstep;
            g[k] = x;
        }
        if (g[7] > fmax) {
            x = fr;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                x += fstep;
                if (x > fmax) x -= (fmax - fmin);
                g[k] = x;
            }
        }
        fr = g[7];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            phase += g[k];
            p[k] = phase;
        }
    }
    __device__ __forceinline__ void step1(float& fr, float& phase) const {
        fr += fstep;
        if (fr > fmax) fr -= (fmax - fmin);
        phase += fr;
    }
};

template <class ARGS>  // (ModArgs, TxArgs: N, osr, bws)
__device__ __forceinline__ ChirpWalk chirp_walk(const ARGS& A) {
    ChirpWalk w;
    w.fmin = -kPi * A.bws / (float)A.osr;
    w.fmax = kPi * A.bws / (float)A.osr;
    w.fstep = (2.0f * kPi * A.bws) / (float)(A.N * A.osr * A.osr);
    return w;
}

// the symbol-end wrap (ChirpGenerator.hpp:49, evaluated in double there)
__device__ __forceinline__ float wrap_phase(float phase) {
    const double w = floor((double)(phase / (2.0f * kPi))) * 2 * (double)kPi;
    return (float)((double)phase - w);
}

// Batch pass 1: the phase at every symbol start.
__global__ void k_mod_walk(ModArgs A) {
    const unsigned long long f = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= A.frames) return;
    const ChirpWalk W = chirp_walk(A);
    const int step = A.N * A.osr;
    float phase = 0.0f;
    const unsigned long long ns = A.nsyms + 2;
    for (unsigned long long s = 0; s < ns; ++s) {
        A.phase0[f * ns + s] = phase;
        float fr = W.fmin + mod_f0(A, f, s);
        int i = 0;
        for (; i + 8 <= step; i += 8) {
            float p[8];
            W.step8(fr, phase, p);
        }
        for (; i < step; ++i) W.step1(fr, phase);
        phase = wrap_phase(phase);
    }
}

// Few-symbol pass 1a: each symbol's frequency sequence (ChirpGenerator.hpp:
// 39-40; it restarts at fMin + f0 every symbol, so symbols run in parallel),
// one thread per symbol, into phases[].
__global__ void k_mod_freq(ModArgs A) {
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long ns = A.nsyms + 2;
    if (g >= A.frames * ns) return;
    const ChirpWalk W = chirp_walk(A);
    const int step = A.N * A.osr;
    float fr = W.fmin + mod_f0(A, g / ns, g % ns);
    float* out = A.phases + g * (unsigned long long)step;
    int i = 0;
    for (; (step & 3) == 0 && i + 4 <= step; i += 4) {  // 16-B aligned rows
        float q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            fr += W.fstep;
            if (fr > W.fmax) fr -= (W.fmax - W.fmin);
            q[k] = fr;
        }
        *reinterpret_cast<float4*>(out + i) = make_float4(q[0], q[1], q[2], q[3]);
    }
    for (; i < step; ++i) {
        fr += W.fstep;
        if (fr > W.fmax) fr -= (W.fmax - W.fmin);
        out[i] = fr;
    }
}

// Few-symbol pass 1b: the phase accumulator through the frame, in order
// (ChirpGenerator.hpp:41, 49), one thread per frame: phases[] holds each
// sample's f on entry and its phase on return.  The chain is one dependent
// add per sample, so the loads must never be what it waits for: blocks of
// 64 samples in registers, the next block's 16 loads issued before the
// current block's adds (ping-pong).  Loads and stores share vmcnt, so when
// a block starts, the 16 stores of the previous block and the 16 loads of
// the next are younger than its own loads: the explicit vmcnt(32) says so
// (the compiler's own analysis of the loop falls back to a near-full
// drain).  Rows of a multiple of 64 samples (SF >= 6 at osr 1); the rest
// take the plain loop.
constexpr int kAccBlock = 64;

__device__ __forceinline__ void acc_load(float4 (&b)[kAccBlock / 4], const float* p) {
#pragma unroll
    for (int k = 0; k < kAccBlock / 4; ++k) b[k] = *reinterpret_cast<const float4*>(p + 4 * k);
}

__device__ __forceinline__ void acc_run(float4 (&b)[kAccBlock / 4], float& phase, float* p) {
    __builtin_amdgcn_s_waitcnt(0x8F70);  // vmcnt(32): this block's loads have landed
#pragma unroll
    for (int k = 0; k < kAccBlock / 4; ++k) {
        float4 o;
        phase += b[k].x;
        o.x = phase;
        phase += b[k].y;
        o.y = phase;
        phase += b[k].z;
        o.z = phase;
        phase += b[k].w;
        o.w = phase;
        *reinterpret_cast<float4*>(p + 4 * k) = o;
    }
}

__global__ __launch_bounds__(64) void k_mod_accumulate(ModArgs A) {
    const unsigned long long f = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= A.frames) return;
    const unsigned long long step = (unsigned long long)A.N * A.osr;
    const unsigned long long ns = A.nsyms + 2;
    float* io = A.phases + f * ns * step;
    float phase = 0.0f;
    if (step % kAccBlock == 0) {
        const unsigned long long nb = ns * step / kAccBlock, per = step / kAccBlock;
        float4 b0[kAccBlock / 4], b1[kAccBlock / 4];
        acc_load(b0, io);
        // (the look-ahead loads are unconditional - past the end they
        // re-read the last block - so every path has the same VMEM count
        // and the compiler's waits stay relaxed)
        for (unsigned long long k = 0; k < nb; k += 2) {
            acc_load(b1, io + (k + 1 < nb ? k + 1 : nb - 1) * kAccBlock);
            acc_run(b0, phase, io + k * kAccBlock);
            if ((k + 1) % per == 0) phase = wrap_phase(phase);
            if (k + 1 >= nb) break;
            acc_load(b0, io + (k + 2 < nb ? k + 2 : nb - 1) * kAccBlock);
            acc_run(b1, phase, io + (k + 1) * kAccBlock);
            if ((k + 2) % per == 0) phase = wrap_phase(phase);
        }
        return;
    }
    for (unsigned long long s = 0; s < ns; ++s) {
        float* row = io + s * step;
        for (unsigned long long i = 0; i < step; ++i) {
            phase += row[i];
            row[i] = phase;
        }
        phase = wrap_phase(phase);
    }
}

// A packet's walk without walking it in order, one
// workgroup per frame, everything in LDS.  Symbol s's walk from its pivot
// sample k_s (where |phase| is largest, so consecutive floats are furthest
// apart) to the next symbol's pivot depends only on the float at k_s.  So:
// estimate every symbol's start in double (exact sums of its f row, then
// once more with each symbol's own rounding error, measured by walking every
// symbol from the first estimate in parallel), take the 64 consecutive
// floats around each pivot's estimate as candidates, walk every candidate in
// parallel to the next pivot (tail, symbol-end wrap, head of the next
// symbol) and record where it lands among that symbol's candidates.  The
// serial part is then a chain of ns table lookups from symbol 0's pivot,
// which is walked exactly from phase 0.  Every step is the reference's
// arithmetic on floats (ChirpGenerator.hpp:39-49), so a chain that stays
// inside the windows is the serial walk; one that leaves them (an estimate
// off by more than 32 floats, measured ≤ 19 at SF 7-8: tools/walk_lattice.py)
// falls back to the serial walk of the whole frame.  Rows `stride` floats
// apart in LDS, then T (dynamic LDS: up to SF 9 at 66 symbols); at most
// kModFastSyms symbols; the phases go to A.phases for k_mod_sincos.
// GROWS (round 6, frames whose rows do not fit the LDS: SF 10-12): the rows
// live in A.phases itself (stride = step, where k_mod_sincos reads the
// phases anyway), only T in dynamic LDS; the walks read them through L1/L2
// (one frame's rows: 66 x 16 KiB at SF 12), 16 candidates per thread in the
// candidate walks (one load per 16 chains).  The drift of the corrected
// estimates stays inside the window there too: <= 27 floats at SF 10-12
// after one correction (tools/walk_lattice.py 10 11 12, host).
constexpr int kModFastThreads = 1024;
constexpr int kModFastSyms = 256;
constexpr int kModFastWin = 64;
constexpr size_t kModFastLds = size_t(144) << 10;  // the f rows and T (dynamic)

__device__ __forceinline__ int f_ord(float x) {
    const int i = __float_as_int(x);
    return i >= 0 ? i : (int)(0x80000000u - (unsigned)i);
}
__device__ __forceinline__ float f_unord(int o) {
    return __int_as_float(o >= 0 ? o : (int)(0x80000000u - (unsigned)o));
}

// The split GROWS form's hand-over between its launches (per frame).
struct ModFastG {
    int base[kModFastSyms];
    int kp[kModFastSyms];
    int j0, ok;
};

struct ModFastShared {
    double est[kModFastSyms + 1];  // start estimates
    double tot[kModFastSyms];      // exact sum of each f row
    double err[kModFastSyms];      // each row's rounding error from est
    double piv[kModFastSyms];      // exact partial sum up to the pivot
    int kp[kModFastSyms];          // pivot sample
    int base[kModFastSyms];        // f_ord of the window's first candidate
    int J[kModFastSyms];           // the chain's candidate per symbol
    float xs[kModFastSyms];        // exact symbol starts
    int ok;
};

// f rows read 8 at a time: one LDS round trip per 8 steps of a walk, the
// loads of a block issued before its adds (and stores)
// (PF, rows in global memory, 16-byte aligned: chunks of 16 floats, NB of
// them in flight - a walk waits for one cache round trip per NB x 16 steps
// instead of one per 8; round 6: at SF 12 the round trips were most of the
// split modulator's 390 us per packet)
// PF: element i of the row at row[(i / 4) bs + i % 4] (bs = 4: contiguous;
// the split modulator's interleaved rows: 4 x rows per frame)
template <bool PF = false, int NB = 4, class Fn>
__device__ __forceinline__ void row_blocks(const float* row, int bs, int i0, int i1, Fn fn) {
    int i = i0;
    if constexpr (PF) {
        for (; i < i1 && (i & 3); ++i) fn(i, row[(i >> 2) * bs + (i & 3)]);
        const int nc = i < i1 ? (i1 - i) >> 4 : 0;
        if (nc > 0) {
            // float4 j of chunk c: group (i / 4) + j
            auto src = [&](int j) __attribute__((always_inline)) {
                return reinterpret_cast<const float4*>(row + (size_t)((i >> 2) + j) * (unsigned)bs);
            };
            float4 b[NB][4];
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int c = k < nc ? k : nc - 1;
#pragma unroll
                for (int q = 0; q < 4; ++q) b[k][q] = *src(4 * c + q);
            }
            auto eat = [&](int c, const float4 (&ch)[4]) __attribute__((always_inline)) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ii = i + 16 * c + 4 * q;
                    fn(ii, ch[q].x);
                    fn(ii + 1, ch[q].y);
                    fn(ii + 2, ch[q].z);
                    fn(ii + 3, ch[q].w);
                }
            };
            // (whole rounds without branches, so the load counter's waits
            // stay partial across the loop's back edge; then the rest)
            int c0 = 0;
            for (; c0 + NB <= nc; c0 += NB) {
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    eat(c0 + k, b[k]);
                    const int cn = c0 + k + NB < nc ? c0 + k + NB : nc - 1;  // (past the end: a harmless re-read)
#pragma unroll
                    for (int q = 0; q < 4; ++q) b[k][q] = *src(4 * cn + q);
                }
            }
#pragma unroll
            for (int k = 0; k < NB - 1; ++k)
                if (c0 + k < nc) eat(c0 + k, b[k]);
            i += 16 * nc;
        }
        for (; i < i1; ++i) fn(i, row[(i >> 2) * bs + (i & 3)]);
    } else {
        (void)bs;  // (rows in LDS: contiguous)
        for (; i + 8 <= i1; i += 8) {
            float b[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) b[k] = row[i + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) fn(i + k, b[k]);
        }
        for (; i < i1; ++i) fn(i, row[i]);
    }
}

// The in-place running sum of a global row over [i0, i1) from p (row[i] =
// p += row[i]), the loads pipelined as row_blocks<true, NB> and each chunk
// of 16 stored as four 16-byte stores; returns p.
template <int NB = 4>
__device__ __forceinline__ float walk_store(float* row, int bs, int i0, int i1, float p) {
    int i = i0;
    auto at = [&](int k) -> float& { return row[(k >> 2) * bs + (k & 3)]; };
    for (; i < i1 && (i & 3); ++i) at(i) = p += at(i);
    const int nc = i < i1 ? (i1 - i) >> 4 : 0;
    if (nc > 0) {
        auto io = [&](int j) __attribute__((always_inline)) {
            return reinterpret_cast<float4*>(row + (size_t)((i >> 2) + j) * (unsigned)bs);
        };
        float4 b[NB][4];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int c = k < nc ? k : nc - 1;
#pragma unroll
            for (int q = 0; q < 4; ++q) b[k][q] = *io(4 * c + q);
        }
        auto eat = [&](int c, const float4 (&ch)[4]) __attribute__((always_inline)) {
            float4 o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                o[q].x = p += ch[q].x;
                o[q].y = p += ch[q].y;
                o[q].z = p += ch[q].z;
                o[q].w = p += ch[q].w;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) *io(4 * c + q) = o[q];
        };
        int c0 = 0;
        for (; c0 + NB <= nc; c0 += NB) {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                eat(c0 + k, b[k]);
                const int cn = c0 + k + NB < nc ? c0 + k + NB : nc - 1;  // (a chunk not yet stored, or a re-read)
#pragma unroll
                for (int q = 0; q < 4; ++q) b[k][q] = *io(4 * cn + q);
            }
        }
#pragma unroll
        for (int k = 0; k < NB - 1; ++k)
            if (c0 + k < nc) eat(c0 + k, b[k]);
        i += 16 * nc;
    }
    for (; i < i1; ++i) at(i) = p += at(i);
    return p;
}

// sum of row s's samples [0, i1[s]) in double, a wave per row (GROWS: the
// rows are in global memory, interleaved by 16-byte groups, and every thread
// of the workgroup helps; the sums are estimates, exact to far below a
// float step)
template <class I1>
__device__ __forceinline__ void mf_row_sums(double* out, const float* rows, int ns, int tid, I1 i1) {
    const int wave = tid >> 6, lane = tid & 63, nw = kModFastThreads / 64;
    for (int s = wave; s < ns; s += nw) {
        const float* row = rows + 4 * s;
        const int n = i1(s);
        auto at = [&](int i) { return row[(i >> 2) * 4 * ns + (i & 3)]; };
        double t = 0.0;
        int i = lane;
        // (16 loads in flight per lane before their adds: one cache round
        // trip per 1,024 samples, not per 64)
        for (; i + 64 * 15 < n; i += 64 * 16) {
            float x[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) x[k] = at(i + 64 * k);
#pragma unroll
            for (int k = 0; k < 16; ++k) t += (double)x[k];
        }
        for (; i < n; i += 64) t += (double)at(i);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
        if (lane == 0) out[s] = t;
    }
}

// est[s] = sum over r < s of (a[r] + b[r]) (exclusive prefix, unwrapped),
// one wave, 64 symbols per pass
__device__ __forceinline__ void mf_scan(double* est, const double* a, const double* b, int ns, int lane) {
    double carry = 0.0;
    for (int s0 = 0; s0 < ns; s0 += 64) {
        const int s = s0 + lane;
        const double v = s < ns ? a[s] + (b ? b[s] : 0.0) : 0.0;
        double x = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (s < ns) est[s] = carry + (x - v);
        carry += __shfl(x, 63, 64);
    }
}

#ifdef LPHY_MODFAST_CLOCKS  // timing aid only: per-phase wall clock sums into the clock counters
#define MF_T(k)                                                                   \
    if (tid == 0) {                                                               \
        const unsigned long long now = wall_clock64();                            \
        if (k > 0) atomicAdd(A.slow - kCtrModSerial + kCtrClocks + k - 1, now - mf_t); \
        mf_t = now;                                                               \
    }
#else
#define MF_T(k)
#endif
// PART (GROWS only): 0 the whole walk in this launch; 1 steps 1-5, handing
// the windows, pivots and chain start to A.mfg; 3 steps 7-8 from A.mfg and
// the T that k_mod_cand (step 6, spread over the GPU) wrote to A.mft.
template <bool GROWS, int PART = 0>
__global__ __launch_bounds__(kModFastThreads) void k_mod_fast(ModArgs A, int stride) {
    extern __shared__ float4 mod_lds[];
    __shared__ ModFastShared M;
    const unsigned long long f = blockIdx.x;
    const int step = A.N * A.osr;
    const int ns = (int)(A.nsyms + 2);
    const int tid = threadIdx.x;
    float* rows = GROWS ? A.phases + f * (unsigned long long)ns * step : reinterpret_cast<float*>(mod_lds);
    // GROWS (round 6): the frame's rows interleaved by 16-byte groups,
    // element i of row s at ((i / 4) ns + s) 4 + i % 4, so the walks of one
    // row per lane read and write 1 KiB contiguous per instruction (row
    // after row, each lane's 16 bytes were a cache line of their own); rowp
    // and the group stride bs (LDS rows: contiguous, bs = 4)
    const int bs = GROWS ? 4 * ns : 4;
    auto rowp = [&](int s) __attribute__((always_inline)) { return GROWS ? rows + 4 * s : rows + (size_t)s * stride; };
    // T[s][j]: where candidate j of symbol s lands among symbol s+1's, 255 outside
    unsigned char* T = PART != 0 ? A.mft + f * (unsigned long long)(kModFastSyms * kModFastWin)
                       : GROWS   ? reinterpret_cast<unsigned char*>(mod_lds)
                                 : reinterpret_cast<unsigned char*>(rows + (size_t)ns * stride);
    const ChirpWalk W = chirp_walk(A);
    const double two_pi = 2.0 * (double)kPi;
#ifdef LPHY_MODFAST_CLOCKS
    unsigned long long mf_t = 0;
#endif
    if constexpr (PART == 3) {
        // the hand-over of PART 1 (the rows are in A.phases already)
        const ModFastG& G = A.mfg[f];
        for (int s = tid; s < ns; s += blockDim.x) {
            M.base[s] = G.base[s];
            M.kp[s] = G.kp[s];
        }
        if (tid == 0) {
            M.J[0] = G.j0;
            M.ok = G.ok;
        }
#ifdef LPHY_MODFAST_CLOCKS
        if (tid == 0) mf_t = wall_clock64();
#endif
        __syncthreads();
    } else {
    MF_T(0)
    // 1. f rows (ChirpGenerator.hpp:39-40) and their exact sums
    for (int s = tid; s < ns; s += blockDim.x) {
        float fr = W.fmin + mod_f0(A, f, (unsigned long long)s);
        float* row = rowp(s);
        double t = 0.0;
        int i = 0;
        for (; i + 8 <= step; i += 8) {
            float g[8];
            float x = fr;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                x += W.fstep;
                g[k] = x;
            }
            if (g[7] > W.fmax) {  // (f only grows between wraps: ChirpWalk::step8)
                x = fr;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    x += W.fstep;
                    if (x > W.fmax) x -= (W.fmax - W.fmin);
                    g[k] = x;
                }
            }
            fr = g[7];
            if constexpr (GROWS) {  // (two 16-byte groups)
                *reinterpret_cast<float4*>(row + (size_t)(i >> 2) * bs) = float4{g[0], g[1], g[2], g[3]};
                *reinterpret_cast<float4*>(row + (size_t)((i >> 2) + 1) * bs) = float4{g[4], g[5], g[6], g[7]};
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) row[i + k] = g[k];
            }
            if constexpr (!GROWS)
                t += (((double)g[0] + (double)g[1]) + ((double)g[2] + (double)g[3])) +
                     (((double)g[4] + (double)g[5]) + ((double)g[6] + (double)g[7]));  // (an estimate)
        }
        for (; i < step; ++i) {
            fr += W.fstep;
            if (fr > W.fmax) fr -= (W.fmax - W.fmin);
            row[(i >> 2) * bs + (i & 3)] = fr;
            t += (double)fr;
        }
        if constexpr (!GROWS) M.tot[s] = t;
    }
    __syncthreads();
    if constexpr (GROWS) {  // (the exact sums by the whole workgroup, off the walks' chains)
        mf_row_sums(M.tot, rows, ns, tid, [&](int) { return step; });
        __syncthreads();
    }
    MF_T(1)
    // 2. first estimates of the starts: unwrapped running sums (one add per
    //    symbol in order), wrapped per symbol in parallel
    if (tid < 64) mf_scan(M.est, M.tot, nullptr, ns, tid);
    if (tid == 0) M.ok = A.force_serial ? 0 : 1;  // (force_serial: test build, the fallback's tests)
    __syncthreads();
    MF_T(2)
    // 3. each row walked in float from its estimate: its rounding error, and
    //    the pivot (largest |phase| among every 8th sample) with the exact
    //    partial sum up to it
    for (int s = tid; s < ns; s += blockDim.x) {
        const float* row = rowp(s);
        const double e = M.est[s];
        const float x0 = (float)(e - floor(e * (1.0 / two_pi)) * two_pi);
        float p = x0;
        double q = 0.0, qb = 0.0;
        float best = -1.0f;
        int kb = 0;
        int i = 0;
        if constexpr (GROWS) {
            // the walk alone (the pivot's partial sum: mf_row_sums below)
            row_blocks<true>(row, bs, 0, step, [&](int k, float x) {
                p += x;
                if ((k & 7) == 7) {
                    const float a = fabsf(p);
                    if (a > best) {
                        best = a;
                        kb = k;
                    }
                }
            });
            i = step;
        }
        for (; i + 8 <= step; i += 8) {
            float b[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) b[k] = row[i + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) p += b[k];
            q += (((double)b[0] + (double)b[1]) + ((double)b[2] + (double)b[3])) +
                 (((double)b[4] + (double)b[5]) + ((double)b[6] + (double)b[7]));
            const float a = fabsf(p);
            if (a > best) {
                best = a;
                kb = i + 7;
                qb = q;
            }
        }
        for (; i < step; ++i) {
            p += row[i];
            q += (double)row[i];
            if (fabsf(p) > best) {
                best = fabsf(p);
                kb = i;
                qb = q;
            }
        }
        M.err[s] = (double)p - ((double)x0 + M.tot[s]);
        M.kp[s] = kb;
        M.piv[s] = qb;
    }
    __syncthreads();
    if constexpr (GROWS) {
        mf_row_sums(M.piv, rows, ns, tid, [&](int s) { return M.kp[s] + 1; });
        __syncthreads();
    }
    MF_T(3)
    // 4. corrected estimates (unwrapped, in order); 5. the windows, and
    //    symbol 0's pivot walked exactly from 0
    if (tid < 64) mf_scan(M.est, M.tot, M.err, ns, tid);
    __syncthreads();
    for (int s = tid; s < ns; s += blockDim.x) {
        const double e = M.est[s];
        M.base[s] = f_ord((float)(e - floor(e * (1.0 / two_pi)) * two_pi + M.piv[s])) - kModFastWin / 2;
    }
    __syncthreads();
    if (tid == 0) {
        float p = 0.0f;
        row_blocks<GROWS>(rowp(0), bs, 0, M.kp[0] + 1, [&](int, float x) { p += x; });
        const int j = f_ord(p) - M.base[0];
        M.J[0] = j;
        if (j < 0 || j >= kModFastWin) M.ok = 0;
    }
    MF_T(4)
    if constexpr (PART == 1) {
        __syncthreads();
        ModFastG& G = A.mfg[f];
        for (int s = tid; s < ns; s += blockDim.x) {
            G.base[s] = M.base[s];
            G.kp[s] = M.kp[s];
        }
        if (tid == 0) {
            G.j0 = M.J[0];
            G.ok = M.ok;
        }
        return;
    }
    // 6. every candidate of every symbol walked to the next symbol's pivot,
    //    kPer candidates (j = g, g + kGroups, ...) per thread: one read of
    //    the row feeds kPer independent chains (8 from LDS, 16 from GROWS)
    constexpr int kPer = GROWS ? 16 : 8, kGroups = kModFastWin / kPer;
    for (int idx = tid; idx < (PART == 0 ? (ns - 1) * kGroups : 0); idx += blockDim.x) {
        const int s = idx / kGroups, g = idx - s * kGroups;
        const float* row = rowp(s);
        float p[kPer];
#pragma unroll
        for (int m = 0; m < kPer; ++m) p[m] = f_unord(M.base[s] + g + kGroups * m);
        row_blocks<GROWS>(row, bs, M.kp[s] + 1, step, [&](int, float x) {
#pragma unroll
            for (int m = 0; m < kPer; ++m) p[m] += x;
        });
#pragma unroll
        for (int m = 0; m < kPer; ++m) p[m] = wrap_phase(p[m]);
        const float* nrow = rowp(s + 1);
        const int kn = M.kp[s + 1];
        row_blocks<GROWS>(nrow, bs, 0, kn + 1, [&](int, float x) {
#pragma unroll
            for (int m = 0; m < kPer; ++m) p[m] += x;
        });
        const int b1 = M.base[s + 1];
#pragma unroll
        for (int m = 0; m < kPer; ++m) {
            const int jj = f_ord(p[m]) - b1;
            T[s * kModFastWin + g + kGroups * m] = (jj >= 0 && jj < kModFastWin) ? (unsigned char)jj : (unsigned char)255;
        }
    }
    __syncthreads();
    MF_T(5)
    }  // (PART != 3)
    // 7. the chain, one wave: lane j holds T[s][j], the next candidate is a
    //    lane read at the current one (uniform); T rows read 16 at a time
    if (tid < 64 && M.ok) {
        int j = M.J[0];
        int bad = 0;
        for (int s0 = 0; s0 + 1 < ns; s0 += 16) {
            int t[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) t[k] = s0 + k + 1 < ns ? T[(s0 + k) * kModFastWin + tid] : 0;
            int jv = 0;  // lane k: the candidate of symbol s0 + k + 1
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (s0 + k + 1 < ns) {
                    j = __builtin_amdgcn_readlane(t[k], j & 63);
                    bad |= j == 255;
                    jv = tid == k ? j : jv;
                }
            }
            if (tid < 16 && s0 + tid + 1 < ns) M.J[s0 + tid + 1] = jv;
        }
        if (bad && tid == 0) M.ok = 0;
    }
    __syncthreads();
    MF_T(6)
    if (M.ok) {
        // 8. the rows from their exact pivots: each symbol's tail (after the
        //    pivot) and, from the start that tail's wrap gives the next
        //    symbol, each symbol's head (up to its pivot)
        for (int s = tid; s < ns; s += blockDim.x) {
            float* row = rowp(s);
            float p = f_unord(M.base[s] + M.J[s]);
            if constexpr (GROWS) {
                p = walk_store(row, bs, M.kp[s] + 1, step, p);
            } else {
                row_blocks(row, bs, M.kp[s] + 1, step, [&](int i, float x) {
                    p += x;
                    row[i] = p;
                });
            }
            M.xs[s + 1 < ns ? s + 1 : 0] = s + 1 < ns ? wrap_phase(p) : 0.0f;
        }
        __syncthreads();
        for (int s = tid; s < ns; s += blockDim.x) {
            float* row = rowp(s);
            float p = M.xs[s];
            if constexpr (GROWS) {
                walk_store(row, bs, 0, M.kp[s] + 1, p);
            } else {
                row_blocks(row, bs, 0, M.kp[s] + 1, [&](int i, float x) {
                    p += x;
                    row[i] = p;
                });
            }
        }
    } else if (tid == 0) {
        // the serial walk (k_mod_accumulate's order)
        if (A.slow) atomicAdd(A.slow, 1ull);
        float phase = 0.0f;
        for (int s = 0; s < ns; ++s) {
            float* row = rowp(s);
            for (int i = 0; i < step; ++i) {
                float& x = row[(i >> 2) * bs + (i & 3)];
                phase += x;
                x = phase;
            }
            phase = wrap_phase(phase);
        }
    }
    __syncthreads();
    // 9. the phases out, row after row (k_mod_sincos, GPU-wide, turns them
    //    into IQ: one CU's sincos would be the longest phase); GROWS: they
    //    are there already
    if constexpr (GROWS) {
        MF_T(7)
        return;
    }
    const int count = ns * step;
    float* out = A.phases + f * (unsigned long long)count;
    for (int g = tid; g < count; g += blockDim.x) {
        const int s = g / step;
        out[g] = rows[(size_t)s * stride + (g - s * step)];
    }
    MF_T(7)
}
#undef MF_T

// Step 6 of the split GROWS form across the GPU: one thread per candidate
// (frame f, symbol s < ns - 1, candidate j), a wave per symbol, so the row
// reads are wave-uniform (scalar loads) and the 64 walks of a symbol run
// side by side; each walks its candidate from symbol s's pivot through the
// symbol-end wrap to symbol s + 1's pivot in the reference's float order and
// records where it lands (T).  Four symbols per 256-thread workgroup; 8
// chunks of 16 floats in flight per walk (row_blocks).
__global__ __launch_bounds__(256) void k_mod_cand(ModArgs A) {
    const int ns = (int)(A.nsyms + 2);
    const int per = (ns - 1 + 3) / 4;  // workgroups per frame
    const unsigned long long f = blockIdx.x / (unsigned)per;
    const int s = (int)(blockIdx.x % (unsigned)per) * 4 + (int)(threadIdx.x >> 6);
    const int j = (int)(threadIdx.x & 63);
    if (s >= ns - 1) return;  // (wave-uniform)
    const int step = A.N * A.osr;
    const ModFastG& G = A.mfg[f];
    // (the frame's rows interleaved by 16-byte groups, as k_mod_fast<true> writes them)
    const float* rows = A.phases + f * (unsigned long long)ns * (unsigned)step;
    float p = f_unord(G.base[s] + j);
    row_blocks<true, 8>(rows + 4 * s, 4 * ns, G.kp[s] + 1, step, [&](int, float x) { p += x; });
    p = wrap_phase(p);
    row_blocks<true, 8>(rows + 4 * (s + 1), 4 * ns, 0, G.kp[s + 1] + 1, [&](int, float x) { p += x; });
    const int jj = f_ord(p) - G.base[s + 1];
    A.mft[f * (unsigned long long)(kModFastSyms * kModFastWin) + (unsigned)(s * kModFastWin + j)] =
        (jj >= 0 && jj < kModFastWin) ? (unsigned char)jj : (unsigned char)255;
}

__global__ void k_mod_samples(ModArgs A) {
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long ns = A.nsyms + 2;
    if (g >= A.frames * ns) return;
    const unsigned long long f = g / ns, s = g % ns;
    const ChirpWalk W = chirp_walk(A);
    const int step = A.N * A.osr;
    float phase = A.phase0[g];
    float fr = W.fmin + mod_f0(A, f, s);
    cf32* out = A.iq + (f * ns + s) * (unsigned long long)step;
    for (int i = 0; i < step; ++i) {
        W.step1(fr, phase);
        float sn, cs;
        lphy_libm::sincosf_exact(phase, &sn, &cs);
        out[i] = cf32{A.ampl * cs, A.ampl * sn};  // std::polar(ampl, phase)
    }
}

__global__ void k_mod_sincos(ModArgs A, unsigned long long count) {
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    unsigned long long src = g;
    if (A.blk) {  // (the split form's interleaved rows: k_mod_fast<true>)
        const unsigned long long step = (unsigned long long)A.N * A.osr, fs = step * (unsigned)A.blk;
        const unsigned long long fb = g / fs * fs, r = g - fb, s = r / step, i = r - s * step;
        src = fb + ((i >> 2) * (unsigned)A.blk + s) * 4 + (i & 3);
    }
    float sn, cs;
    lphy_libm::sincosf_exact(A.phases[src], &sn, &cs);
    A.iq[g] = cf32{A.ampl * cs, A.ampl * sn};
}

// compensate_offsets (phy.cpp:150-180): rotation then integer time shift.
__global__ void k_comp_rotate(cf32* out, const cf32* in, unsigned long long count,
                              float rate) {
    const unsigned long long n = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= count) return;
    const float ph = rate * (float)n;
    float sn, cs;
    lphy_libm::sincosf_exact(ph, &sn, &cs);
    out[n] = cmul_x(in[n], cf32{cs, sn});  // samples[n] *= complex (phy.cpp:163)
}

__global__ void k_comp_shift(cf32* out, const cf32* in, unsigned long long count,
                             long long offset) {
    const unsigned long long n = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= count) return;
    const long long src = (long long)n - offset;
    out[n] = (src >= 0 && src < (long long)count) ? in[src] : czero();
}

// ---------------------------------------------------------------------------
// compensate_offsets for every frame of a batch in one pass
// (lphy_hip_compensate_batch / _ragged): frame f rotates by its own
// meta[f].cfo and shifts by its own meta[f].time_offset, both read here, so
// an estimate on the same stream feeds it without a host copy.  Rotation and
// shift fuse into  out[n] = in[n - off] * cis(rate * (n - off))  (0 where
// n - off leaves the frame): 16 B of traffic per sample and no scratch.
//
// The frame geometry is the template argument: CompUniform (frame f at
// f * frame_samples) or CompRagged (the frame's lphy_ragged_desc).
//
// A tile is kCompTile samples: kTile threads x kCompPairs pairs of two
// samples.  Pairs are cut where the destination is 16-byte aligned (`lead`
// is 1 when the frame's first output sample is not), so a whole pair goes out
// in one 16-byte store; the shift makes the source the unaligned side, read
// with one 16-byte load where its address allows and two 8-byte loads where
// not.  The frame's first and last sample may form half a pair.
//
// Work item w = (frame, slot) = (w / slots, w % slots); a slot takes the
// frame's tiles slot, slot + slots, ...; the grid strides over the items.
//   ORDERED = false (out of place): tiles are independent; the uniform form
//     launches one slot per tile, a flat grid over (frame, tile).
//   ORDERED = true (in place, out == in): one slot, so one workgroup owns the
//     frame and walks its tiles in memmove order - descending n for off > 0,
//     ascending for off < 0 - and per tile loads and rotates the sources into
//     registers, __syncthreads(), stores.  Why that is enough, for off > 0
//     (off < 0 mirrors it): tile t stores n in [t*T - lead, (t+1)*T - lead)
//     and reads n - off; every tile walked after it, t' < t, reads indices
//     below (t'+1)*T - lead - off <= t*T - lead - off < t*T - lead, the
//     least index tile t stores, so no store lands on a source still to be
//     read by a later tile; the sources of tile t itself, which its own
//     stores may cover when off < T, are all in registers before the barrier
//     lets any store go.  A frame with off == 0 or no shift is elementwise
//     (each thread stores what it loaded) and needs no order.  In-place
//     parallelism is therefore per frame: a batch of many frames fills the
//     GPU, a single very long buffer is lphy_hip_compensate's case.
// ---------------------------------------------------------------------------
constexpr int kCompPairs = 2;
constexpr int kCompTile = kTile * 2 * kCompPairs;  // samples per tile (1024)
constexpr unsigned kCompRaggedSlots = 8;           // out of place, ragged: workgroups per frame

struct CompUniform {
    unsigned long long frame_samples;
    __device__ __forceinline__ void frame(unsigned long long f, unsigned long long& base,
                                          unsigned long long& count) const {
        base = f * frame_samples;
        count = frame_samples;
    }
};

struct CompRagged {
    const lphy_ragged_desc* __restrict__ desc;  // sym_offset, unit_offset and record [frames] are not read
    __device__ __forceinline__ void frame(unsigned long long f, unsigned long long& base,
                                          unsigned long long& count) const {
        base = desc[f].iq_offset;
        count = desc[f].samples;
    }
};

// samples[src] * complex(cos(ph), sin(ph)), ph = rate * (float)src (phy.cpp:162-165)
__device__ __forceinline__ cf32 comp_rotate(cf32 x, float rate, long long src) {
    const float ph = rate * (float)(unsigned long long)src;
    float sn, cs;
    lphy_libm::sincosf_exact(ph, &sn, &cs);
    return cmul_x(x, cf32{cs, sn});
}

template <class GEO, bool ORDERED>
__global__ __launch_bounds__(kTile) void k_comp_batch(const cf32* in, cf32* out, GEO geo,
                                                      const lphy_frame_meta* __restrict__ meta,
                                                      unsigned long long frames, unsigned slots, int N,
                                                      int osr) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const unsigned long long work = frames * slots;
    for (unsigned long long w = blockIdx.x; w < work; w += gridDim.x) {
        // (everything down to the tile loop is the same in every lane: the
        // frame's record and descriptor are read once per workgroup)
        const unsigned long long f = w / slots;
        unsigned long long base, count;
        geo.frame(f, base, count);
        if (count == 0) continue;
        // phy.cpp:159-160 and :167 as x86-64 evaluates them
        const float rate = -2.0f * kPi * meta[f].cfo / ((float)N * (float)osr);
        long long off = round_to_int(meta[f].time_offset);
        const unsigned long long mag = (unsigned long long)(off < 0 ? -off : off);
        if (off == (long long)(int)0x80000000u || mag >= count) off = 0;  // phy.cpp:168,173: no shift
        const cf32* src_fr = in + base;
        cf32* dst_fr = out + base;
        const long long lead = (long long)(((unsigned long long)dst_fr >> 3) & 1u);
        const unsigned long long tiles = (count + (unsigned long long)lead + kCompTile - 1) / kCompTile;
        for (unsigned long long i = w % slots; i < tiles; i += slots) {
            const unsigned long long t = (ORDERED && off > 0) ? tiles - 1 - i : i;
            cf32 v[kCompPairs][2];
#pragma unroll
            for (int p = 0; p < kCompPairs; ++p) {
                const long long n0 = (long long)(t * kCompTile + 2u * (threadIdx.x + (unsigned)p * kTile)) - lead;
                const long long s0 = n0 - off, s1 = s0 + 1;
                const bool ok0 = n0 >= 0 && n0 < (long long)count && s0 >= 0 && s0 < (long long)count;
                const bool ok1 = n0 + 1 < (long long)count && s1 >= 0 && s1 < (long long)count;
                cf32 x0 = czero(), x1 = czero();
                if (ok0 && ok1 && (((unsigned long long)(src_fr + s0)) & 15u) == 0) {
                    const f4 q = *reinterpret_cast<const f4*>(src_fr + s0);
                    x0 = q.xy;
                    x1 = q.zw;
                } else {
                    if (ok0) x0 = src_fr[s0];
                    if (ok1) x1 = src_fr[s1];
                }
                v[p][0] = ok0 ? comp_rotate(x0, rate, s0) : czero();
                v[p][1] = ok1 ? comp_rotate(x1, rate, s1) : czero();
            }
            if (ORDERED) __syncthreads();
#pragma unroll
            for (int p = 0; p < kCompPairs; ++p) {
                const long long n0 = (long long)(t * kCompTile + 2u * (threadIdx.x + (unsigned)p * kTile)) - lead;
                const bool w0 = n0 >= 0 && n0 < (long long)count, w1 = n0 + 1 < (long long)count;
                if (w0 && w1) {
                    f4 q;
                    q.xy = v[p][0];
                    q.zw = v[p][1];
                    *reinterpret_cast<f4*>(dst_fr + n0) = q;
                } else {
                    if (w0) dst_fr[n0] = v[p][0];
                    if (w1) dst_fr[n0 + 1] = v[p][1];
                }
            }
        }
    }
}

}  // namespace
