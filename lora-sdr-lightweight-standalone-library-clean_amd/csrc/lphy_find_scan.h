// lphy_find_scan.h — the integer logic of the frame search
// (lphy_hip_find_frames, kernels in lphy_find.h): the summary of a segment of
// windows and the operator that joins two of them, the record of a burst, and
// the sizes of the workspace.  A host compiler takes it too
// (tests/cpp/find_frames_check.cpp); the argument checks are with the other
// entry points' in lphy_ragged_layout.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "lphy_ragged_layout.h"
#include "lphy_hd.h"

namespace lphy {

constexpr uint32_t kFindNone = 0xffffffffu;  // no window: never an index (windows < 2^32)
constexpr unsigned kFindChunk = 256;         // windows a workgroup takes at a time, one per thread
constexpr unsigned kFindTile = 1024;         // windows per tile summary: 4 chunks

// A segment of consecutive windows as the burst rule sees it from outside:
// its first and last active window, and the window at which its last burst
// starts when its own first active window is taken to start one (whether it
// does is known only once the segment in front of it is).  All kFindNone for a
// segment without an active window.
struct FindSum {
    uint32_t first, last, start;
};

constexpr FindSum kFindEmpty = {kFindNone, kFindNone, kFindNone};

// one window
LPHY_HD FindSum find_leaf(uint32_t w, bool active) { return active ? FindSum{w, w, w} : kFindEmpty; }

// Segment A followed by segment B.  The gap between A's last and B's first
// active window decides whether B's first window really starts a burst; if it
// does not and B has no later start, the last start is A's.  Associative.
LPHY_HD FindSum find_join(const FindSum& a, const FindSum& b, uint32_t max_gap) {
    if (a.first == kFindNone) return b;
    if (b.first == kFindNone) return a;
    const bool bridged = b.first - a.last - 1 <= max_gap;
    return FindSum{a.first, b.last, (bridged && b.start == b.first) ? a.start : b.start};
}

// What the search needs of lphy_find_params on the device, with the symbol
// length and the output rule.
struct FindGeo {
    uint64_t first, hop, lead, total_samples, step;  // step = S = N * osr
    uint32_t max_gap, min_symbols;
    int mode;
};

enum FindFate : int { kFindKept = 0, kFindShort = 1, kFindLong = 2 };

struct FindBurst {
    uint64_t start, total;  // the frame: total whole symbols at sample `start`
    uint64_t out_syms;      // its slot in the output symbols, (ragged_out_syms + 1) & ~1
    int fate;
};

// The burst of windows a .. b (lphy_hip.h, "Frame search", 3 and 4).  No sum
// wraps for arguments that passed find_frames_args: first + lead + windows *
// hop <= 2^48 and windows * hop / step < 2^32.
LPHY_HD FindBurst find_burst(const FindGeo& g, uint32_t a, uint32_t b) {
    FindBurst r;
    r.start = g.first + g.lead + (uint64_t)a * g.hop;
    uint64_t extent = 0;
    if (r.start < g.total_samples) {
        extent = ((uint64_t)(b - a) + 1) * g.hop;
        if (extent > g.total_samples - r.start) extent = g.total_samples - r.start;
    }
    r.total = extent / g.step;
    r.out_syms = (ragged_out_syms(r.total, g.mode) + 1) & ~uint64_t(1);
    r.fate = r.total < g.min_symbols ? kFindShort : (r.total * g.step >= kRaggedMaxSamples ? kFindLong : kFindKept);
    return r;
}

// ---- the workspace (d_work), every part 16-byte aligned --------------------
// The passes take the windows and one item more: item `windows` closes the
// last burst.
struct FindTileCount {  // what the bursts that end in a tile add
    uint64_t units, syms;
    uint32_t kept, bursts, dropped_short, dropped_long, active, pad[3];
};
struct FindTilePrefix {  // the kept bursts in front of a tile
    uint64_t units, syms;
    uint32_t kept, pad[3];
};
struct FindTotals {  // the call's totals, and the record the padding repeats
    lphy_ragged_desc pad_rec;
    uint32_t kept, pad[7];
};

struct FindLayout {
    uint64_t tiles;
    size_t totals, bits, sums, carry, counts, prefix, bytes;  // offsets, and the size
};

constexpr size_t find_align(size_t x) { return (x + 15) & ~size_t(15); }

inline FindLayout find_layout(uint64_t windows) {
    FindLayout l{};
    l.tiles = windows / kFindTile + 1;  // of windows + 1 items
    size_t at = 0;
    l.totals = at, at += find_align(sizeof(FindTotals));
    l.bits = at, at += find_align((size_t)l.tiles * (kFindTile / 64) * sizeof(uint64_t));
    l.sums = at, at += find_align((size_t)l.tiles * sizeof(FindSum));
    l.carry = at, at += find_align((size_t)l.tiles * 2 * sizeof(uint32_t));
    l.counts = at, at += find_align((size_t)l.tiles * sizeof(FindTileCount));
    l.prefix = at, at += find_align((size_t)l.tiles * sizeof(FindTilePrefix));
    l.bytes = at;
    return l;
}

}  // namespace lphy
