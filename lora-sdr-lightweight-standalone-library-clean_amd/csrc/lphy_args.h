// lphy_args.h — what more than one translation unit of the library needs and
// no device code of its own: the kernels' argument structs, the per-SF launch
// tables (SfOps, filled by each lphy_sf.hip object, read by lphy_hip.hip),
// the frame status codes that pass between the launches of one call, the
// MODE template bits, HIP_OK, and the one answer to "how many workgroups of
// kernel K does this device hold at once" (resident_blocks, per device) with
// the one clamp of a persistent grid to it (persistent_grid).
#pragma once
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <mutex>
#include <vector>

#include "../../include/lphy_hip.h"
#include "lphy_fft.h"  // cf32, kTile

using namespace lphy;

namespace lphy {
// Per-launch parameters
struct DemodArgs {
    const cf32* iq;        // frames * frame_samples
    const cf32* tw;        // N twiddles (KISS, forward)
    const cf32* down;      // N down-chirp samples (genChirp, down=true)
    const float* win;        // N window coefficients or nullptr
    uint16_t* syms;          // output symbols
    lphy_frame_meta* meta;   // per-frame meta (prologue -> demod hand-off)
    unsigned long long frames;
    unsigned long long frame_samples;
    unsigned long long total_syms;  // symbols per frame = frame_samples / step
    unsigned long long out_per_frame;
    int osr;
    int mode;
    int no_scratch;
    int est_units;           // estimate units per frame (est_syms * osr)
    int exact_rotation;      // LPHY_F_EXACT_ROTATION: no certified fast path
    float power_scale;       // LoRaDetector.hpp:29, (float)(20*log10((double)N))
    unsigned long long* counters;  // ctx counters: [0] rechecks, [1..4] phase clocks
    int spec;                // k_frames modes 1/2: speculative normalisation (no whole-frame pre-scan)
    // separate launches, SF 11-12 fast path, modes 1/2: the same speculation
    // across workgroups, per frame {max-abs of the two estimate symbols,
    // max-abs of the symbol windows, least certificate ratio (float bits,
    // atomic max / min), flags (1 NaN, 2 symbol left open)}; nullptr = off
    uint4* spec_big;
    int debug_recheck;       // LPHY_F_DEBUG_RECHECK: mark estimated frames kStatusRecheck before k_demod
    int wave;                // the fused k_wave launch ran (it settles its frames itself)
    // persistent demod workers: symbol stride per step split into whole
    // frames + symbols (host-computed, so the kernel never divides)
    unsigned stride_f, stride_s;
};

struct FinalArgs {
    const uint16_t* syms;
    uint8_t* bytes;
    lphy_frame_meta* meta;
    unsigned long long frames;
    unsigned long long nsyms;     // symbols per frame to decode
    unsigned long long sym_stride;
    int shift;                    // sf > 4 ? sf - 4 : 0
    int decode;
    int set_sync;
};

// lphy_hip_demod_ragged (lphy_ragged.h): the call's tables, flags and output
// bases in A; what DemodArgs holds once per call for frames of one length
// (iq, syms, meta, frame_samples, total_syms, out_per_frame, est_units) the
// ragged kernels fill per frame from its descriptor (frame_view).
struct RaggedArgs {
    DemodArgs A;
    const lphy_ragged_desc* desc;  // A.frames + 1 records
    uint8_t* bytes;                // LPHY_F_DECODE output base or nullptr
    unsigned long long units_hint; // whole symbols of the call when the host knows them, else 0
    int shift;                     // sf - 4 (sync word nibbles)
    int decode;
};

// The detector (lphy_detect.h): what both of its forms share ...
struct DetectArgs {
    const cf32* iq;
    const cf32* tw;        // N twiddles (KISS, forward)
    const cf32* down;      // N down-chirp samples
    const float* win;      // N window coefficients or nullptr
    lphy_detect_rec* out;  // one record per unit
    int dechirp;           // LPHY_DET_DECHIRP (the launcher reads it)
    float power_scale;     // LoRaDetector.hpp:29
    unsigned long long* counters;  // ctx counters (kCtrDetectSerial)
};

// ... and the window geometry of each.  lphy_hip_detect_batch: window w feeds
// the detector the N samples iq[first + w * hop + i * step], record out[w]
struct DetLattice {
    unsigned long long first, hop, step, windows, total_samples;
};

// lphy_hip_detect_ragged: symbol s of frame f feeds the detector
// iq[desc[f].iq_offset + s * N * osr + phase + i * osr], record
// out[desc[f].unit_offset + s]
struct DetRagged {
    const lphy_ragged_desc* desc;  // frames + 1 records
    unsigned frames;               // < 2^31
    unsigned osr, phase;           // phase < osr
    unsigned long long units_hint; // as RaggedArgs' (the launcher reads it)
};

// Per-SF launch entry points (one table per lphy_sf.hip instance)
struct SfOps {
    int (*demod)(const DemodArgs&, hipStream_t, bool prologue, bool symbols, int per_cu);
    int (*frames)(const DemodArgs&, hipStream_t);  // k_frames
    int (*wave)(const DemodArgs&, hipStream_t);    // k_wave
    int (*post)(int mode, const DemodArgs&, const FinalArgs&, bool fix, bool fin, hipStream_t);
    int (*estimate)(const DemodArgs&, hipStream_t);
    // debug build: read (and reset) this SF's failed index checks (else null)
    int (*violations)(unsigned long long* out, int reset);
    // lphy_hip_demod_ragged: prologue, symbols and finalisation (SF 7-12);
    // grid_cap > 0 caps the symbol kernel's persistent grid (test build:
    // lphy_hip_test_grid_cap, else 0)
    int (*ragged)(const RaggedArgs&, hipStream_t, unsigned grid_cap);
    // lphy_hip_detect_batch: k_detect over the lattice (SF 7-12); grid_cap as above
    int (*detect)(const DetectArgs&, const DetLattice&, hipStream_t, unsigned grid_cap);
    // lphy_hip_estimate_ragged: k_rg_estimate (SF 7-12); of RaggedArgs it
    // reads A's tables, iq, meta, frames, osr and desc
    int (*estimate_ragged)(const RaggedArgs&, unsigned long long est_samples, hipStream_t);
    // lphy_hip_detect_ragged: k_detect over the table (SF 7-12); grid_cap as above
    int (*detect_ragged)(const DetectArgs&, const DetRagged&, hipStream_t, unsigned grid_cap);
};
extern const SfOps sf_ops_1, sf_ops_2, sf_ops_3, sf_ops_4, sf_ops_5, sf_ops_6,
    sf_ops_7, sf_ops_8, sf_ops_9, sf_ops_10, sf_ops_11, sf_ops_12;
}  // namespace lphy

namespace {

constexpr float kPi = 3.14159265358979323846f;  // lora_phy::PI (phy.hpp:20)
// Kernel MODE template argument: the lphy_mode in bits 0-1, plus kWinBit when
// a window is applied, so the per-sample window multiply is compile-time
// (a runtime branch per sample would split the staging block and serialise
// the 16 independent sincos chains of a lane).
constexpr int kWinBit = 4;
// ... and kOsrBit when osr > 1: k_demod then reads every osr-th sample
// (LoRaDemod.cpp:155, phy.cpp:225); the osr == 1 kernels keep unit-stride
// addressing.
constexpr int kOsrBit = 8;

// Internal frame status between the launches of one lphy_hip_demod_batch:
// the frame holds a non-finite value where the reference's Annex G complex
// product (cmul_x) could differ from the hot kernels' plain one, and is
// re-run exactly by k_post.  Never left in a record after the call.
constexpr int kStatusFixup = 0x7f5a0001;
// ... and: some symbols were left uncertified by the fused kernel's fast
// rotation (value kSymRecheck in the output; k_post recomputes exactly those)
constexpr int kStatusRecheck = 0x7f5a0002;
constexpr uint16_t kSymRecheck = 0xffff;  // never a bin index (N <= 4096)
// ... and: k_frames demodulated the frame with the normalisation of its
// first two symbols, but a later sample raised the frame's max-abs, so the
// estimate must be redone with the exact scale and the symbols' certificates
// re-checked against the exact rate (k_post settle_frames).  The record then
// holds {cfo: the frame's max-abs, time_offset: the symbols' least
// certificate ratio}; the second code also has symbols left open.
constexpr int kStatusSettle = 0x7f5a0003;
constexpr int kStatusSettleRecheck = 0x7f5a0004;

// the fused kernels' (k_frames, k_wave)
struct FrameArgs {
    DemodArgs A;
    unsigned waves;  // wavefronts in the grid
};

// query(device) >= 0, asked once per device and call site (Fn: the site's
// lambda); `other` for a device the runtime does not count.
template <class Fn>
long long per_device(int device, long long other, Fn query) {
    static std::mutex m;
    static std::vector<long long> v;  // -1: not asked yet
    std::lock_guard<std::mutex> g(m);
    if (v.empty()) {
        int n = 0;
        (void)hipGetDeviceCount(&n);
        v.assign(n > 0 ? n : 1, -1);
    }
    if (device < 0 || (size_t)device >= v.size()) return other;
    if (v[device] < 0) v[device] = query(device);
    return v[device];
}

// the device this thread launches on (the entry points set the context's)
inline int current_device() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev;
}

// CUs of `device` ...
inline int device_cus(int device) {
    return (int)per_device(device, 256, [](int d) {
        int n = 0;
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d);
        return n > 0 ? n : 256;
    });
}
// ... and the workgroups of kTile threads of kernel K that `device`, the
// current one, holds at once
template <auto K>
int resident_blocks(int device) {
    return (int)per_device(device, 256, [](int d) {
        int per = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, K, kTile, 0);
        return device_cus(d) * (per > 0 ? per : 1);
    });
}

// Workgroups of a persistent grid: the `resident` ones, no more than the
// call's `tiles` when the host knows them (else 0: the workgroups past the
// last unit leave at once), no more than `cap` when there is one (else 0).
inline unsigned persistent_grid(unsigned long long resident, unsigned long long tiles, unsigned long long cap) {
    unsigned long long grid = resident;
    if (tiles && grid > tiles) grid = tiles;
    if (cap && grid > cap) grid = cap;
    return (unsigned)grid;
}

}  // namespace

#define HIP_OK(x)                                                         \
    do {                                                                  \
        hipError_t e_ = (x);                                              \
        if (e_ != hipSuccess) {                                           \
            fprintf(stderr, "lphy_hip: %s failed: %s (%s:%d)\n", #x,      \
                    hipGetErrorString(e_), __FILE__, __LINE__);           \
            return -EIO;                                                  \
        }                                                                 \
    } while (0)
