// lphy_chan.h — the channeliser (lphy_hip_channelize): one wideband capture
// in, `channels` mixed, filtered and decimated streams out, by the definition
// in include/lphy_hip.h: per (channel, output) one sequential chain of T
// complex multiply-accumulates in separate float32 operations, then one
// rotation.  The geometry and the argument check are lphy_resample_plan.h.  Only
// lphy_hip.hip includes it.
//
// One launch, one workgroup of kTile threads per tile of kChanTile consecutive
// outputs of every channel; a lane owns one output m of the tile.
//   LDS path (chan_lds_path: a full tile's padded span fits kResLdsBytes):
//     the workgroup stages the tile's span, (nout - 1) * D + T samples, once,
//     with 16-byte loads between an 8-byte head and tail (`first` may be odd),
//     into the padded image of chan_lds_slot.  Every sample then comes from
//     HBM once per tile, whatever the number of channels.
//   global path (every other plan: a long filter at a large D): the lanes read
//     their samples from global memory.
// Either way the channels go in groups of CG (res_group: 1, 2, 4 or 8): per
// tap one 8-byte read of x and, per channel of the group, the tap g from a
// wave-uniform address (a scalar load) and 8 VALU operations on the channel's
// own accumulator pair, so a lane runs 2 * CG independent chains.  No chain is
// split: that is what the definition requires.  No workgroup waits on another,
// no atomic, vector stores only.
//
// The capture's format (lphy_hip_channelize_raw) is a template parameter.
// LPHY_FMT_CF32 is the kernel above.  An integer capture is converted to
// float32 where it is staged, (float) of the integer and for CU8 one
// subtraction of 127.5f, all exact, and stored as float2 into the same padded
// image, so the loop and its order of operations are the float path's and so
// are the bits:
//   LDS path: 16-byte loads of 4 (SC16) or 8 (8-bit) samples between a head
//     and a tail of single samples (chan_stage_split);
//   global path: the lane converts its own sample in the loop.
#pragma once
#include "lphy_args.h"
#include "lphy_resample_plan.h"

namespace {

static_assert((int)kChanTile == (int)kTile, "a tile is one output per thread");

struct ChanArgs {
    unsigned long long first, outputs, out_stride;
    unsigned channels, T, D, R;
    unsigned rot_base;  // rot_first % R
};

// One sample of a capture in format FMT as it lies in memory, and its float32 value.
template <int FMT>
struct ChanFmt;
template <>
struct ChanFmt<LPHY_FMT_CF32> {
    using sample = float2;
    static __device__ __forceinline__ float2 value(float2 s) { return s; }
};
template <>
struct ChanFmt<LPHY_FMT_SC16> {
    using sample = short2;
    static __device__ __forceinline__ float2 value(short2 s) { return make_float2((float)s.x, (float)s.y); }
};
template <>
struct ChanFmt<LPHY_FMT_SC8> {
    using sample = char2;
    static __device__ __forceinline__ float2 value(char2 s) { return make_float2((float)s.x, (float)s.y); }
};
template <>
struct ChanFmt<LPHY_FMT_CU8> {
    using sample = uchar2;
    static __device__ __forceinline__ float2 value(uchar2 s) {
        return make_float2((float)s.x - 127.5f, (float)s.y - 127.5f);
    }
};

template <int CG, bool LDS, int FMT>
__global__ __launch_bounds__(kTile) void k_chan(const typename ChanFmt<FMT>::sample* __restrict__ in,
                                                const float2* __restrict__ taps, const float2* __restrict__ rot,
                                                float2* __restrict__ out, ChanArgs A) {
    using Fmt = ChanFmt<FMT>;
    extern __shared__ float2 chan_lds[];
    const unsigned tid = threadIdx.x;
    const ChanSpan sp = chan_tile_span(A.first, A.D, A.T, A.outputs, blockIdx.x);
    const typename Fmt::sample* __restrict__ src = in + sp.begin;
    if constexpr (LDS && FMT != LPHY_FMT_CF32) {
        // sp.samples < 2^24 on this path
        constexpr unsigned kPer = 16 / sizeof(typename Fmt::sample);
        const ChanStage st = chan_stage_split((uintptr_t)src, (unsigned)sp.samples, sizeof(typename Fmt::sample));
        if (tid < st.head) chan_lds[chan_lds_slot(tid)] = Fmt::value(src[tid]);
        for (unsigned v = tid; v < st.vectors; v += kTile) {
            const unsigned i = st.head + kPer * v;
            const uint4 w = *reinterpret_cast<const uint4*>(src + i);  // kPer samples in one load
            typename Fmt::sample s[kPer];
            __builtin_memcpy(s, &w, 16);
#pragma unroll
            for (unsigned j = 0; j < kPer; ++j) chan_lds[chan_lds_slot(i + j)] = Fmt::value(s[j]);
        }
        if (tid < st.tail) {
            const unsigned i = st.head + kPer * st.vectors + tid;
            chan_lds[chan_lds_slot(i)] = Fmt::value(src[i]);
        }
        __syncthreads();
    } else if constexpr (LDS) {
        // sp.samples < 2^24 on this path
        const unsigned n = (unsigned)sp.samples;
        const unsigned head = (unsigned)(((uintptr_t)src >> 3) & 1);  // samples in front of a 16-byte boundary
        const unsigned pairs = (n - head) >> 1;                       // n >= 1 = the most head can be
        if (tid == 0 && head) chan_lds[0] = src[0];
        for (unsigned p = tid; p < pairs; p += kTile) {
            const unsigned i = head + 2 * p;
            const float4 v = *reinterpret_cast<const float4*>(src + i);
            chan_lds[chan_lds_slot(i)] = make_float2(v.x, v.y);
            chan_lds[chan_lds_slot(i + 1)] = make_float2(v.z, v.w);
        }
        if (tid == kTile - 1 && ((n - head) & 1)) chan_lds[chan_lds_slot(n - 1)] = src[n - 1];
        __syncthreads();
    }
    if (tid >= sp.nout) return;  // the last tile's lanes past the outputs: nothing staged for them, nothing to store
    const unsigned m = blockIdx.x * kChanTile + tid;  // outputs < 2^32
    const unsigned x0 = tid * A.D;                     // this lane's first sample in the span
    const unsigned ri = (A.rot_base + m % A.R) % A.R;
    for (unsigned c0 = 0; c0 < A.channels; c0 += CG) {
        const float2* __restrict__ tp[CG];
#pragma unroll
        for (int j = 0; j < CG; ++j) tp[j] = taps + (size_t)min(c0 + j, A.channels - 1) * A.T;
        float ar[CG], ai[CG];
#pragma unroll
        for (int j = 0; j < CG; ++j) ar[j] = ai[j] = 0.0f;
#pragma unroll 2
        for (unsigned k = 0; k < A.T; ++k) {
            float2 x;
            if constexpr (LDS) x = chan_lds[chan_lds_slot(x0 + k)];
            else x = Fmt::value(src[(unsigned long long)tid * A.D + k]);
#pragma unroll
            for (int j = 0; j < CG; ++j) {
                const float2 g = tp[j][k];
                const float pr = x.x * g.x - x.y * g.y;
                const float pi = x.x * g.y + x.y * g.x;
                ar[j] = ar[j] + pr;
                ai[j] = ai[j] + pi;
            }
        }
#pragma unroll
        for (int j = 0; j < CG; ++j) {
            const unsigned c = c0 + j;
            if (c < A.channels) {
                const float2 r = rot[(size_t)c * A.R + ri];
                out[(unsigned long long)c * A.out_stride + m] =
                    make_float2(ar[j] * r.x - ai[j] * r.y, ar[j] * r.y + ai[j] * r.x);
            }
        }
    }
}

// The launch; the plan has passed chan_args and has outputs > 0.
template <int CG, int FMT>
void chan_launch_group(bool lds, dim3 grid, size_t lds_bytes, hipStream_t st, const typename ChanFmt<FMT>::sample* in,
                       const float2* taps, const float2* rot, float2* out, const ChanArgs& A) {
    if (lds) hipLaunchKernelGGL((k_chan<CG, true, FMT>), grid, dim3(kTile), lds_bytes, st, in, taps, rot, out, A);
    else hipLaunchKernelGGL((k_chan<CG, false, FMT>), grid, dim3(kTile), 0, st, in, taps, rot, out, A);
}

template <int FMT>
void chan_launch_format(const lphy_chan_plan& p, const void* d_in, const float* d_taps, const float* d_rot,
                        float* d_out, hipStream_t st) {
    const ChanArgs A{p.first, p.outputs, p.out_stride, p.channels, p.taps, p.decim, p.rot_period,
                     (unsigned)(p.rot_first % p.rot_period)};
    const bool lds = chan_lds_path(p.decim, p.taps);
    const size_t lds_bytes = lds ? (size_t)chan_lds_slots(p.decim, p.taps) * 8 : 0;
    const dim3 grid((unsigned)res_tiles(p.outputs));
    const auto* in = static_cast<const typename ChanFmt<FMT>::sample*>(d_in);
    const float2* taps = reinterpret_cast<const float2*>(d_taps);
    const float2* rot = reinterpret_cast<const float2*>(d_rot);
    float2* out = reinterpret_cast<float2*>(d_out);
    switch (res_group(p.channels)) {
        case 1: chan_launch_group<1, FMT>(lds, grid, lds_bytes, st, in, taps, rot, out, A); break;
        case 2: chan_launch_group<2, FMT>(lds, grid, lds_bytes, st, in, taps, rot, out, A); break;
        case 4: chan_launch_group<4, FMT>(lds, grid, lds_bytes, st, in, taps, rot, out, A); break;
        default: chan_launch_group<8, FMT>(lds, grid, lds_bytes, st, in, taps, rot, out, A); break;
    }
}

// `format` is one of the four (chan_raw_aligned)
inline void chan_launch(const lphy_chan_plan& p, const void* d_in, int format, const float* d_taps,
                        const float* d_rot, float* d_out, hipStream_t st) {
    switch (format) {
        case LPHY_FMT_SC16: chan_launch_format<LPHY_FMT_SC16>(p, d_in, d_taps, d_rot, d_out, st); break;
        case LPHY_FMT_SC8: chan_launch_format<LPHY_FMT_SC8>(p, d_in, d_taps, d_rot, d_out, st); break;
        case LPHY_FMT_CU8: chan_launch_format<LPHY_FMT_CU8>(p, d_in, d_taps, d_rot, d_out, st); break;
        default: chan_launch_format<LPHY_FMT_CF32>(p, d_in, d_taps, d_rot, d_out, st); break;
    }
}

inline void resample_launch(const lphy_chan_plan& p, const float* d_in, const float* d_taps, const float* d_rot,
                            float* d_out, hipStream_t st) {
    chan_launch_format<LPHY_FMT_CF32>(p, d_in, d_taps, d_rot, d_out, st);
}

}  // namespace
