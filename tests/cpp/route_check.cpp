// route_check.cpp — csrc/lphy_route.h over the whole grid of call shapes
// (no GPU):
//   1. route() equals the decision the library made before it had one routing
//      function, written out below as the plain predicates it was then spread
//      over (frames_fit, wave_fit, the `fused` expression, DemodArgs::wave and
//      the per-SF launch template's SF >= 11 rule);
//   2. every shape routed to Frames or Wave has a kernel in the instantiation
//      rule of the per-SF launch templates (no routed shape can reach their
//      defensive -ENOTSUP).
#include <cstdio>

#include "lphy_route.h"

using namespace lphy;

namespace {
// ---- the earlier decision, as it stood ------------------------------------
bool frames_fit(unsigned sf, unsigned osr, int est_units, size_t total) {
    if (sf > 10 || osr != 1 || est_units != 2 || total < 2) return false;
    const size_t E = sf >= 4 ? 16 : ((size_t)1 << sf);
    const size_t lps = ((size_t)1 << sf) / E;
    const size_t wt = 64 / lps;
    return total + 1 >= 2 * wt;
}

bool wave_fit(unsigned sf, unsigned osr, int est_units, size_t total, int mode, bool win, bool exact_rotation,
              bool spec) {
    return sf >= 7 && sf <= 12 && (sf >= 9 || total >= (size_t)(4096u >> sf)) && osr == 1 &&
           !(sf == 12 && win && mode == LPHY_MODE_LORA_DEMODULATE) && est_units == 2 && total >= 2 &&
           !exact_rotation && (mode == LPHY_MODE_DEMODULATE || spec);
}

Path old_route(const RouteArgs& r) {
    const unsigned both = LPHY_F_STAGE_PROLOGUE | LPHY_F_STAGE_SYMBOLS;
    const unsigned stages = r.flags & (LPHY_F_STAGE_PROLOGUE | LPHY_F_STAGE_SYMBOLS | LPHY_F_STAGE_FINAL);
    const bool all = stages == 0;
    const bool wfit = wave_fit(r.sf, r.osr, r.est_units, r.total_syms, r.mode, r.window, r.exact_rotation, r.spec) &&
                      !(r.flags & LPHY_F_FRAMES_KERNEL);
    const bool fused = (all || (stages & both) == both) && !(r.flags & LPHY_F_UNFUSED) && r.frames >= r.fused_min &&
                       (frames_fit(r.sf, r.osr, r.est_units, r.total_syms) || wfit);
    const bool wave = fused && (r.sf >= 11 || wfit);
    if (!fused) return Path::Separate;
    // the launch template: SF 11-12 k_wave; SF 7-10 k_wave when `wave`; else k_frames
    if (r.sf >= 11) return Path::Wave;
    return r.sf >= 7 && wave ? Path::Wave : Path::Frames;
}

// ---- the kernels the per-SF objects hold ----------------------------------
// k_frames<SF, mode [| window]>: SF 1-10, every mode, with and without window
bool has_frames_kernel(unsigned sf) { return sf >= 1 && sf <= 10; }
// k_wave<SF, mode [| window], span>: spanning at SF 7-10; not spanning at
// SF 9-12 (SF 7-8 "spanning only"), without SF 12 mode 1 Hann
bool has_wave_kernel(unsigned sf, int mode, bool win, bool span) {
    if (span) return sf >= 7 && sf <= 10;
    return sf >= 9 && sf <= 12 && !(sf == 12 && win && mode == LPHY_MODE_LORA_DEMODULATE);
}
}  // namespace

int main() {
    const unsigned osrs[] = {1, 2, 4};
    const unsigned stage_masks[] = {0, LPHY_F_STAGE_PROLOGUE | LPHY_F_STAGE_SYMBOLS, LPHY_F_STAGE_SYMBOLS};
    unsigned long long shapes = 0, bad = 0, n_frames = 0, n_wave = 0, n_span = 0;
    for (unsigned sf = 1; sf <= 12; ++sf) {
        const size_t spw = sf >= 7 ? (size_t)(4096u >> sf) : 64;
        const size_t fused_min = sf >= 11 ? 384 : 256;
        const size_t totals[] = {0, 1, 2, 3, spw - 1, spw, spw + 1, 64};
        const size_t frames[] = {1, fused_min - 1, fused_min};
        for (unsigned osr : osrs)
        for (int mode = 0; mode <= 2; ++mode)
        for (int win = 0; win <= 1; ++win)
        for (size_t total : totals)
        for (size_t nf : frames)
        for (int spec = 0; spec <= 1; ++spec)
        for (int exact = 0; exact <= 1; ++exact)
        for (int unfused = 0; unfused <= 1; ++unfused)
        for (int fk = 0; fk <= 1; ++fk)
        for (unsigned sm : stage_masks) {
            RouteArgs r{};
            r.sf = sf;
            r.osr = osr;
            r.mode = mode;
            r.window = win != 0;
            r.total_syms = total;
            // lphy_hip_demod_batch: two estimate symbols (mode 0 always), osr units each
            r.est_units = (int)((mode == LPHY_MODE_DEMODULATE ? 2 : (total < 2 ? total : 2)) * osr);
            r.frames = nf;
            r.fused_min = fused_min;
            r.spec = spec != 0;
            r.exact_rotation = exact != 0;
            r.flags = sm | (unfused ? (unsigned)LPHY_F_UNFUSED : 0u) | (fk ? (unsigned)LPHY_F_FRAMES_KERNEL : 0u);
            ++shapes;
            const Path p = route(r), q = old_route(r);
            bool ok = p == q;
            if (p == Path::Frames) {
                ++n_frames;
                ok = ok && has_frames_kernel(sf) && frames_kernel(sf);
            } else if (p == Path::Wave) {
                ++n_wave;
                const bool span = wave_spans(sf, total);
                n_span += span;
                ok = ok && has_wave_kernel(sf, mode, r.window, span) && wave_kernel(sf, mode, r.window, span);
            }
            if (!ok && bad++ < 20)
                std::printf("MISMATCH sf=%u osr=%u mode=%d win=%d total=%zu frames=%zu spec=%d exact=%d flags=%#x: "
                            "route %d, before %d\n",
                            sf, osr, mode, win, total, nf, spec, exact, r.flags, (int)p, (int)q);
        }
        // the table against the arithmetic it replaced
        const int lps = (1 << sf) / (sf >= 4 ? 16 : (1 << sf));
        if (route_lps(sf) != lps || (sf >= 7 && (size_t)route_spw(sf) != spw) || (sf < 7 && route_spw(sf) != 0)) {
            std::printf("MISMATCH geometry table sf=%u\n", sf);
            ++bad;
        }
    }
    std::printf("shapes=%llu frames=%llu wave=%llu spanning=%llu mismatches=%llu\n", shapes, n_frames, n_wave, n_span,
                bad);
    return bad ? 1 : 0;
}
