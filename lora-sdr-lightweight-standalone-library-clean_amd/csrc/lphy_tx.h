// lphy_tx.h — the ragged transmit path (lphy_hip_modulate_ragged,
// lphy_hip_tx_ragged): lora_modulate (LoRaMod.cpp:8-43), optionally with
// lora_encode (LoRaEncoder.cpp:6-18) fused in front, for frames of different
// lengths in one call.  Bit-exact with the reference like the batch modulator
// of lphy_mod.h, whose recurrence (ChirpWalk, wrap_phase) it reuses; built for
// throughput - a single packet is lphy_hip_modulate_host's case (k_mod_fast).
// Only lphy_hip.hip includes it.
//
// The frame geometry is the caller's lphy_ragged_desc table; the symbol source
// is the template argument: TxSymbols (uint16 symbols at sym_offset) or
// TxBytes (bytes at sym_offset / 2 through encodeHamming84sx).  A frame of
// total = samples / (N osr) whole symbols modulates 2 + SRC::count(total - 2)
// symbols (none when total < 2) at iq_offset: sync 0, sync 1, the data.
//
// Two launches, no scratch:
//   k_tx_walk     one thread per frame walks the frame's phase recurrence in
//                 order (it is one float chain through the frame) and parks
//                 the phase at each symbol's start in the real part of that
//                 symbol's own first output sample;
//   k_tx_samples  persistent grid over tiles of kTile units (symbols); a lane
//                 finds its unit's frame by binary search over unit_offset
//                 (ragged_unit, lphy_ragged_unit.h),
//                 reads its parked phase, and the wave then regenerates its 64
//                 symbols chunk by chunk: every lane walks kTxChunk phases of
//                 its own symbol into its LDS row, then the lanes regroup
//                 along the rows, kTxChunk / 2 lanes per row and two samples
//                 per lane, so a store instruction writes 16 bytes per lane and
//                 256 contiguous bytes per row (k_mod_samples stores 8 bytes
//                 per lane to 64 rows a symbol apart).
// Why the parked phase is safe (DESIGN "Ragged transmit"): the slot belongs to
// one unit; k_tx_walk writes it, and in k_tx_samples only the wave that owns
// the unit stores to the unit's row, after the barrier that follows the read.
#pragma once
#include "lphy_mod.h"
#include "lphy_ragged_unit.h"

namespace {

constexpr int kTxChunk = 32;                       // samples of a symbol staged per round
constexpr int kTxRow = kTxChunk + 1;               // floats per LDS row: the carry, then the chunk
constexpr int kTxRowLanes = kTxChunk / 2;          // lanes along a row in the store phase
constexpr int kTxStoreRows = 64 / kTxRowLanes;     // rows a store instruction covers

struct TxArgs {
    const lphy_ragged_desc* __restrict__ desc;  // frames + 1 records
    cf32* iq;
    uint16_t* syms_out;  // (TxBytes) the encoded symbols at sym_offset, or null
    unsigned frames;
    int N, osr;
    int shift;  // sf - 4: the sync nibbles' position (LoRaMod.cpp:21-24)
    float bws, ampl;
    uint8_t sync;
};

// encodeHamming84sx (LoRaCodes.hpp:229-242) of a nibble
__device__ __forceinline__ unsigned tx_enc84(unsigned x) {
    auto par = [](unsigned v) { return (unsigned)__popc(v) & 1u; };
    return (x & 0xF) | (par(x & 0x7) << 4) | (par(x & 0xE) << 5) | (par(x & 0xB) << 6) | (par(x & 0xD) << 7);
}

struct TxSymbols {
    const uint16_t* __restrict__ syms;
    // data symbols modulated of the frame's nsyms
    __device__ static unsigned long long count(unsigned long long nsyms) { return nsyms; }
    __device__ __forceinline__ unsigned get(const lphy_ragged_desc& d, unsigned long long k) const {
        return syms[d.sym_offset + k];
    }
};

struct TxBytes {
    const uint8_t* __restrict__ bytes;
    __device__ static unsigned long long count(unsigned long long nsyms) { return nsyms & ~1ull; }
    // byte j gives symbols 2j (high nibble) and 2j + 1 (low nibble)
    __device__ __forceinline__ unsigned get(const lphy_ragged_desc& d, unsigned long long k) const {
        const unsigned b = bytes[d.sym_offset / 2 + k / 2];
        return tx_enc84((k & 1) ? (b & 0xF) : (b >> 4));
    }
};

// symbols the frame modulates, the two sync symbols included
template <class SRC>
__device__ __forceinline__ unsigned long long tx_symbols(const lphy_ragged_desc& d, unsigned step) {
    const unsigned long long total = d.samples / step;
    return total < 2 ? 0 : 2 + SRC::count(total - 2);
}

// symbol s of the frame: its value and its start frequency (mod_f0)
template <class SRC>
__device__ __forceinline__ float tx_f0(const TxArgs& A, const SRC& src, const lphy_ragged_desc& d,
                                       unsigned long long s, uint16_t& v) {
    if (s == 0) v = (uint16_t)((A.sync >> 4) << A.shift);
    else if (s == 1) v = (uint16_t)((A.sync & 0x0f) << A.shift);
    else v = (uint16_t)src.get(d, s - 2);
    return (2.0f * kPi * (float)v * A.bws) / ((float)A.N * (float)A.osr);
}

// Pass 1: the phase at every symbol start, parked where pass 2 finds it.
// (The frames of a wave differ in length; the lanes that finish early idle.)
template <class SRC>
__global__ __launch_bounds__(64) void k_tx_walk(TxArgs A, SRC src) {
    const unsigned long long f = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= A.frames) return;
    const lphy_ragged_desc d = A.desc[f];
    const unsigned step = (unsigned)A.N * (unsigned)A.osr;
    const unsigned long long ns = tx_symbols<SRC>(d, step);
    const ChirpWalk W = chirp_walk(A);
    cf32* fr_iq = A.iq + d.iq_offset;
    float phase = 0.0f;
    for (unsigned long long s = 0; s < ns; ++s) {
        reinterpret_cast<float*>(fr_iq + s * step)[0] = phase;
        if (s + 1 == ns) break;  // (nothing starts after the last symbol)
        uint16_t v;
        float fr = W.fmin + tx_f0(A, src, d, s, v);
        unsigned i = 0;
        for (; i + 8 <= step; i += 8) {
            float p[8];
            W.step8(fr, phase, p);
        }
        for (; i < step; ++i) W.step1(fr, phase);
        phase = wrap_phase(phase);
    }
}

// (a wave's LDS operations execute in issue order: only compiler motion
// across the point has to stop, as team_sync does inside one wavefront)
__device__ __forceinline__ void tx_wave_sync() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// std::polar(ampl, phase) for two consecutive samples
__device__ __forceinline__ void tx_polar2(float ampl, float p0, float p1, cf32& x0, cf32& x1) {
    float sn, cs;
    lphy_libm::sincosf_exact(p0, &sn, &cs);
    x0 = cf32{ampl * cs, ampl * sn};
    lphy_libm::sincosf_exact(p1, &sn, &cs);
    x1 = cf32{ampl * cs, ampl * sn};
}

// Pass 2.  Row l of a wave's LDS block holds, for lane l's symbol, the phase
// of the sample before the chunk (the carry) and the chunk's kTxChunk phases:
// kTxRow = 33 floats, an odd stride, so the 64 lanes' 4-byte writes of one
// column fall into distinct banks.  Output pairs are cut where the
// destination is 16-byte aligned: a frame at an odd iq_offset (`lead`, as in
// k_comp_batch) pairs samples (2j - 1, 2j), the first of which is the carry
// for j = 0; its sample 0 goes out alone with the first chunk and its last
// sample alone after the last one.  step is a multiple of kTxChunk (SF >= 7).
template <class SRC>
__global__ __launch_bounds__(kTile) void k_tx_samples(TxArgs A, SRC src) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    __shared__ float lds[kTile * kTxRow];
    __shared__ cf32* dstp[kTile];  // each unit's row in the IQ, null for a unit with nothing to do

    const unsigned nframes = A.frames;
    const lphy_ragged_desc* __restrict__ desc = A.desc;
    const unsigned long long units = desc[nframes].unit_offset;
    const unsigned step = (unsigned)A.N * (unsigned)A.osr;
    const ChirpWalk W = chirp_walk(A);
    const int tid = threadIdx.x, lane = tid & 63, wave0 = tid - lane;
    float* rows = lds + wave0 * kTxRow;  // this wave's 64 rows
    float* mine = rows + lane * kTxRow;
    const int rr = lane / kTxRowLanes, rj = lane % kTxRowLanes;  // store phase: row within the group, pair within the row
    const unsigned long long stride = (unsigned long long)gridDim.x * kTile;
    for (unsigned long long t0 = (unsigned long long)blockIdx.x * kTile; t0 < units; t0 += stride) {
        const RaggedUnit ru = ragged_unit<false>(desc, nframes, units, t0 + (unsigned)tid);
        const lphy_ragged_desc& d = ru.d;
        const unsigned long long s = ru.s;
        // (the byte form's odd last symbol is not modulated)
        const bool live = ru.live && s < tx_symbols<SRC>(d, step);
        cf32* row = live ? A.iq + d.iq_offset + s * step : nullptr;
        float phase = 0.0f, fr = 0.0f;
        if (live) {
            phase = reinterpret_cast<const float*>(row)[0];  // parked by k_tx_walk
            uint16_t v;
            fr = W.fmin + tx_f0(A, src, d, s, v);
            if (A.syms_out && s >= 2) A.syms_out[d.sym_offset + (s - 2)] = v;
        }
        dstp[tid] = row;
        // every parked phase of the tile is in a register before any lane of
        // the workgroup stores a sample
        __syncthreads();
        if (__ballot(live) == 0) continue;  // (a wave of tail units)
        const bool lead = (((unsigned long long)row >> 3) & 1u) != 0;
        for (unsigned c0 = 0; c0 < step; c0 += kTxChunk) {
            mine[0] = phase;  // sample c0 - 1 (before the first chunk: unused)
#pragma unroll
            for (int b = 0; b < kTxChunk / 8; ++b) {
                float p[8];
                W.step8(fr, phase, p);
#pragma unroll
                for (int k = 0; k < 8; ++k) mine[1 + 8 * b + k] = p[k];
            }
            tx_wave_sync();
#pragma unroll 1
            for (int g = 0; g < 64 / kTxStoreRows; ++g) {
                const int r = g * kTxStoreRows + rr;
                cf32* o = dstp[wave0 + r];
                if (!o) continue;
                const int ld = (int)(((unsigned long long)o >> 3) & 1u);
                const float* ph = rows + r * kTxRow + 2 * rj + 1 - ld;  // samples n0, n0 + 1
                const long long n0 = (long long)c0 + 2 * rj - ld;
                cf32 x0, x1;
                tx_polar2(A.ampl, ph[0], ph[1], x0, x1);
                if (n0 >= 0) {
                    f4 q;
                    q.xy = x0;
                    q.zw = x1;
                    *reinterpret_cast<f4*>(o + n0) = q;
                } else {
                    o[0] = x1;  // (a lead row's sample 0: half a pair)
                }
            }
            tx_wave_sync();  // the rows are read before the next chunk overwrites them
        }
        if (live && lead) {  // a lead row's last sample: half a pair
            float sn, cs;
            lphy_libm::sincosf_exact(phase, &sn, &cs);
            row[step - 1] = cf32{A.ampl * cs, A.ampl * sn};
        }
    }
}

}  // namespace
