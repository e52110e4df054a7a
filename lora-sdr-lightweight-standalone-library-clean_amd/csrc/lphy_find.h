// lphy_find.h — the frame search (lphy_hip_find_frames): detector records in,
// the ragged table of the bursts found out.  A scan and a compaction over up to
// 2^32 records, as reduce-then-scan over tiles of kFindTile windows: no
// workgroup waits on another, the order between the passes is the order of
// the launches.  The integer logic (the summary operator, burst -> record, the
// workspace) is lphy_find_scan.h.  Only lphy_hip.hip includes it.
//
// The items are the windows and one more: item w < windows is window w, item
// `windows` stands for a window far behind the capture.  An item closes a burst
// when it starts the next one (or is the last item) and an active window lies
// in front of it: the burst is (last start, last active window) of the items in
// front, so a burst needs nothing behind the item that closes it, and the
// bursts come out in the order of their first windows.
//
// Six launches (d_work's parts in brackets):
//   k_find_flags   persistent grid over tiles: one 16-byte load per record, the
//                  activity of every window as one bit [bits] and the tile's
//                  summary FindSum [sums];
//   k_find_carry   one workgroup: the exclusive scan of the summaries with
//                  find_join, so every tile knows the last active window and
//                  the last burst start in front of it [carry];
//   k_find_count   persistent grid: the bursts that every tile's items close,
//                  counted by their fate, with the units and output symbols of
//                  the kept ones [counts];
//   k_find_offsets one workgroup: the exclusive prefix of kept / units / syms
//                  per tile [prefix], d_info, the call's totals [totals];
//   k_find_write   persistent grid: k_find_count's walk again, now with every
//                  kept burst's rank and offsets: record k for k < max_frames,
//                  and the totals record from the last frame written [totals];
//   k_find_pad     persistent grid: records frames .. max_frames.
// The record passes after the first read one bit per window, not the record.
#pragma once
#include "lphy_args.h"
#include "lphy_find_scan.h"

namespace {

struct FindArgs {
    const uint4* __restrict__ rec;  // lphy_detect_rec, 16 bytes
    unsigned long long windows;
    FindGeo geo;
    float threshold;
    unsigned max_frames;
    lphy_ragged_desc* desc;
    lphy_find_info* info;
    // d_work (find_layout)
    unsigned long long tiles;
    FindTotals* totals;
    unsigned long long* bits;
    FindSum* sums;
    uint2* carry;  // {last active window, last burst start} in front of a tile
    FindTileCount* counts;
    FindTilePrefix* prefix;
};

static_assert((int)kFindChunk == (int)kTile && kFindChunk == 4 * 64, "a chunk is one item per thread of a 4-wave workgroup");
constexpr int kFindWaves = kFindChunk / 64;
constexpr int kFindChunks = kFindTile / kFindChunk;

// Index of the last item of the workgroup's chunk in front of this lane for
// which `pred` holds, `carry` when there is none; idx: this lane's item (low 32
// bits: only an index of an item with pred is ever formed).  carry becomes the
// same for the item behind the chunk.  lds: kFindWaves slots.  Two barriers.
__device__ __forceinline__ uint32_t find_last_before(bool pred, uint32_t idx, uint32_t& carry, uint32_t* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(pred);
    const uint32_t wave0 = idx - (uint32_t)lane;
    if (lane == 0) lds[wave] = mask ? wave0 + 63u - (uint32_t)__clzll((long long)mask) : kFindNone;
    __syncthreads();
    uint32_t before = carry, all = carry;
#pragma unroll
    for (int v = 0; v < kFindWaves; ++v) {
        const uint32_t x = lds[v];
        if (x != kFindNone) {
            all = x;
            if (v < wave) before = x;
        }
    }
    __syncthreads();
    carry = all;
    const unsigned long long lower = mask & ((1ull << lane) - 1ull);
    return lower ? wave0 + 63u - (uint32_t)__clzll((long long)lower) : before;
}

// The first item of the chunk with pred, kFindNone when there is none.
__device__ __forceinline__ uint32_t find_first_in_chunk(bool pred, uint32_t idx, uint32_t* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(pred);
    if (lane == 0) lds[wave] = mask ? idx - (uint32_t)lane + (uint32_t)__builtin_ctzll(mask) : kFindNone;
    __syncthreads();
    uint32_t first = kFindNone;
#pragma unroll
    for (int v = kFindWaves - 1; v >= 0; --v)
        if (lds[v] != kFindNone) first = lds[v];
    __syncthreads();
    return first;
}

struct FindSum3 {
    unsigned long long kept, units, syms;
};
__device__ __forceinline__ FindSum3 operator+(const FindSum3& a, const FindSum3& b) {
    return FindSum3{a.kept + b.kept, a.units + b.units, a.syms + b.syms};
}

// Exclusive prefix of v over the workgroup's 256 lanes; total: the sum.  A
// wave whose lanes all hold zeros (most: bursts are sparse) skips its scan.
// lds: kFindWaves slots.  Two barriers.
__device__ __forceinline__ FindSum3 find_scan3(const FindSum3& v, FindSum3& total, FindSum3* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    FindSum3 incl = v;
    if (__ballot((v.kept | v.units | v.syms) != 0) != 0) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const FindSum3 o{__shfl_up(incl.kept, d), __shfl_up(incl.units, d), __shfl_up(incl.syms, d)};
            if (lane >= d) incl = o + incl;
        }
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    FindSum3 before{0, 0, 0}, all{0, 0, 0};
#pragma unroll
    for (int w = 0; w < kFindWaves; ++w) {
        const FindSum3 x = lds[w];
        all = all + x;
        if (w < wave) before = before + x;
    }
    __syncthreads();
    total = all;
    return FindSum3{before.kept + incl.kept - v.kept, before.units + incl.units - v.units,
                    before.syms + incl.syms - v.syms};
}

// ---- pass 1: activity bits and tile summaries -------------------------------
__global__ __launch_bounds__(kTile) void k_find_flags(FindArgs A) {
    __shared__ uint32_t lds[kFindWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned long long t = blockIdx.x; t < A.tiles; t += gridDim.x) {
        uint32_t last = kFindNone, start = kFindNone, first = kFindNone;
        for (int c = 0; c < kFindChunks; ++c) {
            const unsigned long long i = t * kFindTile + (unsigned)c * kFindChunk + threadIdx.x;
            bool act = false;
            if (i < A.windows) {
                const uint4 r = A.rec[i];
                act = (__uint_as_float(r.x) - __uint_as_float(r.y)) >= A.threshold;
            }
            const unsigned long long mask = __ballot(act);
            if (lane == 0) A.bits[t * (kFindTile / 64) + (unsigned)c * kFindWaves + wave] = mask;
            const uint32_t f = find_first_in_chunk(act, (uint32_t)i, lds);
            if (first == kFindNone) first = f;
            // within the tile: the tile's first active window taken as a start
            const uint32_t before = find_last_before(act, (uint32_t)i, last, lds);
            const bool is_start = act && (before == kFindNone || (uint32_t)i - before - 1 > A.geo.max_gap);
            (void)find_last_before(is_start, (uint32_t)i, start, lds);
        }
        if (threadIdx.x == 0) A.sums[t] = FindSum{first, last, start};
    }
}

// ---- pass 2: what lies in front of every tile -------------------------------
__device__ __forceinline__ FindSum find_shfl_up(const FindSum& s, int d) {
    return FindSum{__shfl_up(s.first, d), __shfl_up(s.last, d), __shfl_up(s.start, d)};
}

__global__ __launch_bounds__(kTile) void k_find_carry(FindArgs A) {
    __shared__ FindSum lds[kFindWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t gap = A.geo.max_gap;
    FindSum carry = kFindEmpty;
    for (unsigned long long base = 0; base < A.tiles; base += kTile) {
        const unsigned long long t = base + threadIdx.x;
        FindSum incl = t < A.tiles ? A.sums[t] : kFindEmpty;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const FindSum o = find_shfl_up(incl, d);
            if (lane >= d) incl = find_join(o, incl, gap);
        }
        FindSum excl = find_shfl_up(incl, 1);
        if (lane == 0) excl = kFindEmpty;
        if (lane == 63) lds[wave] = incl;
        __syncthreads();
        FindSum before = carry, all = carry;
#pragma unroll
        for (int w = 0; w < kFindWaves; ++w) {
            all = find_join(all, lds[w], gap);
            if (w < wave) before = all;
        }
        __syncthreads();
        before = find_join(before, excl, gap);
        if (t < A.tiles) A.carry[t] = make_uint2(before.last, before.start);
        carry = all;
    }
}

// ---- the walk of passes 3 and 5 ---------------------------------------------
// Item i of a chunk: whether it closes a burst, and which.  last / start: the
// last active window and the last burst start in front of the chunk, advanced
// to the chunk behind.
struct FindClose {
    bool closes;
    FindBurst b;
};

__device__ __forceinline__ FindClose find_item(const FindArgs& A, unsigned long long i, bool act, uint32_t& last,
                                               uint32_t& start, uint32_t* lds) {
    const uint32_t before = find_last_before(act, (uint32_t)i, last, lds);
    const bool is_start = act && (before == kFindNone || (uint32_t)i - before - 1 > A.geo.max_gap);
    const uint32_t from = find_last_before(is_start, (uint32_t)i, start, lds);
    FindClose r;
    r.closes = before != kFindNone && (is_start || i == A.windows);
    r.b = FindBurst{0, 0, 0, kFindShort};
    if (r.closes) r.b = find_burst(A.geo, from, before);
    return r;
}

// the activity bit of item i (tile t, chunk c): one 8-byte load per wave
__device__ __forceinline__ bool find_bit(const FindArgs& A, unsigned long long t, int c, unsigned long long& mask) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    mask = A.bits[t * (kFindTile / 64) + (unsigned)c * kFindWaves + wave];
    return (mask >> lane) & 1ull;
}

// ---- pass 3: what every tile's items close ----------------------------------
__global__ __launch_bounds__(kTile) void k_find_count(FindArgs A) {
    __shared__ uint32_t lds[kFindWaves];
    __shared__ FindSum3 lds3[kFindWaves];
    __shared__ uint32_t cnt[kFindWaves][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned long long t = blockIdx.x; t < A.tiles; t += gridDim.x) {
        const uint2 cy = A.carry[t];
        uint32_t last = cy.x, start = cy.y;
        FindSum3 mine{0, 0, 0};
        uint32_t bursts = 0, n_short = 0, n_long = 0, active = 0;  // of this wave
        for (int c = 0; c < kFindChunks; ++c) {
            const unsigned long long i = t * kFindTile + (unsigned)c * kFindChunk + threadIdx.x;
            unsigned long long mask;
            const bool act = find_bit(A, t, c, mask);
            active += (uint32_t)__popcll(mask);
            const FindClose x = find_item(A, i, act, last, start, lds);
            bursts += (uint32_t)__popcll(__ballot(x.closes));
            n_short += (uint32_t)__popcll(__ballot(x.closes && x.b.fate == kFindShort));
            n_long += (uint32_t)__popcll(__ballot(x.closes && x.b.fate == kFindLong));
            if (x.closes && x.b.fate == kFindKept) mine = mine + FindSum3{1, x.b.total, x.b.out_syms};
        }
        FindSum3 total;
        (void)find_scan3(mine, total, lds3);
        if (lane == 0) {
            cnt[wave][0] = bursts;
            cnt[wave][1] = n_short;
            cnt[wave][2] = n_long;
            cnt[wave][3] = active;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            FindTileCount o{};
            o.units = total.units;
            o.syms = total.syms;
            o.kept = (uint32_t)total.kept;
            for (int w = 0; w < kFindWaves; ++w) {
                o.bursts += cnt[w][0];
                o.dropped_short += cnt[w][1];
                o.dropped_long += cnt[w][2];
                o.active += cnt[w][3];
            }
            A.counts[t] = o;
        }
        __syncthreads();  // cnt is read before the next tile overwrites it
    }
}

// ---- pass 4: the tiles' offsets, the call's info and totals -----------------
__global__ __launch_bounds__(kTile) void k_find_offsets(FindArgs A) {
    __shared__ FindSum3 lds3[kFindWaves];
    FindSum3 carry{0, 0, 0};
    // this thread's share of what is only summed: {bursts, dropped_short}, dropped_long, active
    FindSum3 rest{0, 0, 0};
    unsigned long long n_long = 0, active = 0;
    for (unsigned long long base = 0; base < A.tiles; base += kTile) {
        const unsigned long long t = base + threadIdx.x;
        FindTileCount c{};
        if (t < A.tiles) c = A.counts[t];
        FindSum3 total;
        const FindSum3 before = find_scan3(FindSum3{c.kept, c.units, c.syms}, total, lds3);
        if (t < A.tiles) {
            FindTilePrefix p{};
            p.units = carry.units + before.units;
            p.syms = carry.syms + before.syms;
            p.kept = (uint32_t)(carry.kept + before.kept);
            A.prefix[t] = p;
        }
        carry = carry + total;
        rest = rest + FindSum3{c.bursts, c.dropped_short, 0};
        n_long += c.dropped_long;
        active += c.active;
    }
    FindSum3 sum_rest, sum_more;
    (void)find_scan3(rest, sum_rest, lds3);
    (void)find_scan3(FindSum3{n_long, active, 0}, sum_more, lds3);
    if (threadIdx.x == 0) {
        const uint32_t kept = (uint32_t)carry.kept;
        const uint32_t frames = kept < A.max_frames ? kept : A.max_frames;
        lphy_find_info o{};
        o.frames = frames;
        o.bursts = (uint32_t)sum_rest.kept;
        o.dropped_short = (uint32_t)sum_rest.units;
        o.dropped_long = (uint32_t)sum_more.kept;
        o.overflow = kept - frames;
        o.active = (uint32_t)sum_more.units;
        *A.info = o;
        FindTotals tt{};  // (no frame: the padding is all zero; else k_find_write fills pad_rec)
        tt.kept = kept;
        *A.totals = tt;
    }
}

// ---- pass 5: the frames' records --------------------------------------------
__global__ __launch_bounds__(kTile) void k_find_write(FindArgs A) {
    __shared__ uint32_t lds[kFindWaves];
    __shared__ FindSum3 lds3[kFindWaves];
    const uint32_t kept = A.totals->kept;
    const uint32_t frames = kept < A.max_frames ? kept : A.max_frames;
    for (unsigned long long t = blockIdx.x; t < A.tiles; t += gridDim.x) {
        if (A.counts[t].kept == 0) continue;  // (uniform: nothing of this tile is written)
        const uint2 cy = A.carry[t];
        uint32_t last = cy.x, start = cy.y;
        const FindTilePrefix p = A.prefix[t];
        FindSum3 at{p.kept, p.units, p.syms};
        for (int c = 0; c < kFindChunks; ++c) {
            const unsigned long long i = t * kFindTile + (unsigned)c * kFindChunk + threadIdx.x;
            unsigned long long mask;
            const bool act = find_bit(A, t, c, mask);
            const FindClose x = find_item(A, i, act, last, start, lds);
            const bool keep = x.closes && x.b.fate == kFindKept;
            FindSum3 total;
            const FindSum3 before = find_scan3(keep ? FindSum3{1, x.b.total, x.b.out_syms} : FindSum3{0, 0, 0}, total, lds3);
            const FindSum3 me = at + before;
            at = at + total;
            if (keep && me.kept < frames) {
                const uint64_t samples = x.b.total * A.geo.step;
                A.desc[me.kept] = lphy_ragged_desc{x.b.start, samples, me.syms, me.units};
                if (me.kept + 1 == frames)
                    A.totals->pad_rec =
                        lphy_ragged_desc{x.b.start + samples, 0, me.syms + x.b.out_syms, me.units + x.b.total};
            }
        }
    }
}

// ---- pass 6: records frames .. max_frames -----------------------------------
__global__ __launch_bounds__(kTile) void k_find_pad(FindArgs A) {
    const uint32_t kept = A.totals->kept;
    const unsigned long long frames = kept < A.max_frames ? kept : A.max_frames;
    const lphy_ragged_desc rec = A.totals->pad_rec;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTile;
    for (unsigned long long r = frames + (unsigned long long)blockIdx.x * kTile + threadIdx.x; r <= A.max_frames;
         r += stride)
        A.desc[r] = rec;
}

}  // namespace
