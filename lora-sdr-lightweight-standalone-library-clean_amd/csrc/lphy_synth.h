// lphy_synth.h — the synthesiser (lphy_hip_synthesize), the channeliser's
// mirror: `channels` narrow streams in, one wideband stream out, by the
// definition in include/lphy_hip.h: per (output, channel) one sequential chain
// of up to ceil(T / U) complex multiply-accumulates in separate float32
// operations over rotated narrow samples, the channels' sums added in channel
// order.  The geometry and the argument check are lphy_resample_plan.h.  Only
// lphy_hip.hip includes it.
//
// One launch, one workgroup of kTile threads per tile of kSynthTile consecutive
// outputs; a lane owns one output w = first + n, its q = w / U and p = w % U.
// The channels go in groups of CG (res_group: 1, 2, 4 or 8), so a lane runs
// 2 * CG independent chains; no chain is split.
//   LDS path (synth_lds_path: one group's image fits kResLdsBytes): per group
//     the workgroup stages the span of synth_tile_span, already rotated and
//     with (+0, +0) where j is outside the stream, so the rotation (and its
//     index modulo R) costs per input sample, not per tap.  A lane then reads x
//     from LDS - nearly wave-uniform addresses, consecutive where they differ -
//     and its tap taps[c*T + i*U + p] from global memory: consecutive lanes
//     read consecutive taps until p wraps, so a wave's read is one or a few
//     whole lines that L1 serves, and at most T * CG taps are live per tile.
//   global path (every other plan): a lane reads and rotates its own samples.
// No workgroup waits on another, no atomic, vector stores only.
#pragma once
#include "lphy_args.h"
#include "lphy_resample_plan.h"

namespace {

static_assert((int)kSynthTile == (int)kTile, "a tile is one output per thread");

struct SynthArgs {
    unsigned long long first, outputs, in_samples, in_stride;
    unsigned channels, T, U, R;
    unsigned rot_base;  // rot_first % R
};

template <int CG, bool LDS>
__global__ __launch_bounds__(kTile) void k_synth(const float2* __restrict__ in, const float2* __restrict__ taps,
                                                 const float2* __restrict__ rot, float2* __restrict__ out,
                                                 SynthArgs A) {
    extern __shared__ float2 synth_lds[];
    const unsigned tid = threadIdx.x;
    const SynthSpan sp = synth_tile_span(A.first, A.U, A.T, A.outputs, blockIdx.x);
    const unsigned S = synth_lds_slots(A.U, A.T);  // one channel's slots in the image
    // the lane's output: q = sp.q0 + dq, p, and the taps of its chains, k = i*U + p < T
    const unsigned t = sp.p0 + tid, dq = t / A.U, p = t % A.U;
    const unsigned ni = p < A.T ? (A.T - 1 - p) / A.U + 1 : 0;
    const unsigned back = synth_chain(A.T, A.U) - 1;  // slot of j = q - i: back + dq - i
    const bool live = tid < sp.nout;

    // LDS path: which slots hold a sample (synth_stage) and the rotation index
    // of the first that can, j0 at slot zeros; slot s >= zeros then has index
    // (rb + s - zeros) % R.  global path: the rotation index of the lane's own j = q.
    unsigned rb = 0;
    const SynthStage stg = synth_stage(sp);
    if constexpr (LDS) {
        rb = (unsigned)((A.rot_base + stg.j0 % A.R) % A.R);
    } else {
        rb = (unsigned)((A.rot_base + (sp.q0 + dq) % A.R) % A.R);
    }

    float yr = 0.0f, yi = 0.0f;
    for (unsigned c0 = 0; c0 < A.channels; c0 += CG) {
        unsigned ch[CG];
#pragma unroll
        for (int g = 0; g < CG; ++g) ch[g] = min(c0 + g, A.channels - 1);
        if constexpr (LDS) {
            if (c0) __syncthreads();  // the previous group's image has been read
            for (unsigned s = tid; s < sp.samples; s += kTile) {
                uint64_t j;
                const bool have = synth_slot_sample(stg, s, A.in_samples, &j);
                const unsigned ri = have ? (rb + (s - stg.zeros)) % A.R : 0u;
#pragma unroll
                for (int g = 0; g < CG; ++g) {
                    float2 v = make_float2(0.0f, 0.0f);
                    if (have) {
                        const float2 x = in[(unsigned long long)ch[g] * A.in_stride + (unsigned long long)j];
                        const float2 r = rot[(size_t)ch[g] * A.R + ri];
                        v = make_float2(x.x * r.x - x.y * r.y, x.x * r.y + x.y * r.x);
                    }
                    synth_lds[g * S + s] = v;
                }
            }
            __syncthreads();
        }
        float ar[CG], ai[CG];
#pragma unroll
        for (int g = 0; g < CG; ++g) ar[g] = ai[g] = 0.0f;
        if (live) {
            unsigned ri = rb;  // global path: the index of j = q - i, one down per tap
#pragma unroll 2
            for (unsigned i = 0; i < ni; ++i) {
                const unsigned k = i * A.U + p;
                float2 x[CG];
                if constexpr (LDS) {
#pragma unroll
                    for (int g = 0; g < CG; ++g) x[g] = synth_lds[g * S + back + dq - i];
                } else {
                    const unsigned long long q = sp.q0 + dq;
                    const bool have = q >= i && q - i < A.in_samples;
#pragma unroll
                    for (int g = 0; g < CG; ++g) {
                        x[g] = make_float2(0.0f, 0.0f);
                        if (have) {
                            const float2 v = in[(unsigned long long)ch[g] * A.in_stride + (q - i)];
                            const float2 r = rot[(size_t)ch[g] * A.R + ri];
                            x[g] = make_float2(v.x * r.x - v.y * r.y, v.x * r.y + v.y * r.x);
                        }
                    }
                    ri = ri ? ri - 1 : A.R - 1;
                }
#pragma unroll
                for (int g = 0; g < CG; ++g) {
                    const float2 h = taps[(size_t)ch[g] * A.T + k];
                    const float pr = x[g].x * h.x - x[g].y * h.y;
                    const float pi = x[g].x * h.y + x[g].y * h.x;
                    ar[g] = ar[g] + pr;
                    ai[g] = ai[g] + pi;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < CG; ++g) {
            if (c0 + g < A.channels) {  // uniform: a channel past the last adds nothing, not even +0
                yr = yr + ar[g];
                yi = yi + ai[g];
            }
        }
    }
    if (live) out[(unsigned long long)blockIdx.x * kSynthTile + tid] = make_float2(yr, yi);
}

// The launch; the plan has passed synth_args and has outputs > 0.
template <int CG>
void synth_launch_group(bool lds, dim3 grid, size_t lds_bytes, hipStream_t st, const float2* in, const float2* taps,
                        const float2* rot, float2* out, const SynthArgs& A) {
    if (lds) hipLaunchKernelGGL((k_synth<CG, true>), grid, dim3(kTile), lds_bytes, st, in, taps, rot, out, A);
    else hipLaunchKernelGGL((k_synth<CG, false>), grid, dim3(kTile), 0, st, in, taps, rot, out, A);
}

inline void resample_launch(const lphy_synth_plan& p, const float* d_in, const float* d_taps, const float* d_rot,
                            float* d_out, hipStream_t st) {
    const SynthArgs A{p.first,  p.outputs, p.in_samples, p.in_stride, p.channels,
                      p.taps,   p.interp,  p.rot_period, (unsigned)(p.rot_first % p.rot_period)};
    const bool lds = synth_lds_path(p.channels, p.interp, p.taps);
    const size_t lds_bytes = lds ? (size_t)synth_lds_bytes(p.channels, p.interp, p.taps) : 0;
    const dim3 grid((unsigned)res_tiles(p.outputs));
    const float2* in = reinterpret_cast<const float2*>(d_in);
    const float2* taps = reinterpret_cast<const float2*>(d_taps);
    const float2* rot = reinterpret_cast<const float2*>(d_rot);
    float2* out = reinterpret_cast<float2*>(d_out);
    switch (res_group(p.channels)) {
        // one channel's image always fits (synth_lds_path; 34,824 bytes at most): no k_synth<1, false>
        case 1: hipLaunchKernelGGL((k_synth<1, true>), grid, dim3(kTile), lds_bytes, st, in, taps, rot, out, A); break;
        case 2: synth_launch_group<2>(lds, grid, lds_bytes, st, in, taps, rot, out, A); break;
        case 4: synth_launch_group<4>(lds, grid, lds_bytes, st, in, taps, rot, out, A); break;
        default: synth_launch_group<8>(lds, grid, lds_bytes, st, in, taps, rot, out, A); break;
    }
}

}  // namespace
