// lphy_hip.hip — the C ABI (include/lphy_hip.h) of the MI355X (gfx950) LoRa
// PHY library: contexts and their constant tables, the per-call choice of
// kernels (lphy_route.h) and their launch through the per-SF tables (SfOps:
// the kernels templated on SF are the lphy_sf.hip objects'), and the
// SF-independent kernels themselves: the finalisation (k_finalize), the
// modulator and the compensation (lphy_mod.h), the ragged transmit path
// (lphy_tx.h), the frame search (lphy_find.h), the channeliser (lphy_chan.h),
// the synthesiser (lphy_synth.h), k_mark_recheck.  The host-
// buffer forms (*_host) are lphy_host.h, included at the end.
#include "lphy_args.h"
#include "lphy_final.h"
#include "lphy_mod.h"
#include "lphy_tx.h"
#include "lphy_route.h"
#include "lphy_stage_plan.h"
#include "lphy_lorawan_ragged.h"
#include "lphy_find.h"
#include "lphy_chan.h"
#include "lphy_synth.h"
#include "lphy_testing.h"

#include <climits>
#include <cmath>
#include <complex>
#include <cstring>
#include <memory>
#include <atomic>
#include <mutex>
#include <vector>

#ifndef __HIP_DEVICE_COMPILE__
// Empty launch tables, overridden by every lphy_sf.hip object linked in
// (experiment builds may link only the SF they time: tools/ubench/variants.py)
namespace lphy {
__attribute__((weak)) extern const SfOps sf_ops_1 = {};
__attribute__((weak)) extern const SfOps sf_ops_2 = {};
__attribute__((weak)) extern const SfOps sf_ops_3 = {};
__attribute__((weak)) extern const SfOps sf_ops_4 = {};
__attribute__((weak)) extern const SfOps sf_ops_5 = {};
__attribute__((weak)) extern const SfOps sf_ops_6 = {};
__attribute__((weak)) extern const SfOps sf_ops_7 = {};
__attribute__((weak)) extern const SfOps sf_ops_8 = {};
__attribute__((weak)) extern const SfOps sf_ops_9 = {};
__attribute__((weak)) extern const SfOps sf_ops_10 = {};
__attribute__((weak)) extern const SfOps sf_ops_11 = {};
__attribute__((weak)) extern const SfOps sf_ops_12 = {};
}  // namespace lphy
#endif
// Constant device tables of one (sf, bw, window): KISS twiddles, down-chirp,
// Hann window.  Read-only after creation, so contexts made by
// lphy_hip_ctx_share hold the same tables.
struct lphy_tables {
    int device = 0;
    cf32* d_tw = nullptr;
    cf32* d_down = nullptr;
    float* d_win = nullptr;
    ~lphy_tables() {
        (void)hipSetDevice(device);
        if (d_tw) (void)hipFree(d_tw);
        if (d_down) (void)hipFree(d_down);
        if (d_win) (void)hipFree(d_win);
    }
};

constexpr size_t kPinnedMax = size_t(32) << 20;

struct lphy_hip_ctx {
    int device = 0;
    unsigned sf = 0, N = 0, bw_hz = 0, osr = 1;
    int window = 0;
    float power_scale = 0.0f;
    std::shared_ptr<lphy_tables> tab;
    cf32* d_tw = nullptr;   // tab's
    cf32* d_down = nullptr;
    float* d_win = nullptr;
    // the host convenience entry points (*_host): their own stream, so a
    // call waits for its own work only (hipStreamSynchronize), and staging
    // sized by lphy_hip_ctx_reserve up front; the mutex only orders calls
    // that share this context (one context per workspace / thread: never
    // contended)
    std::mutex mu;
    hipStream_t stream = nullptr;
    void* d_stage = nullptr;
    // pinned mirror of the staging's first h_stage_bytes (up to kPinnedMax):
    // a call whose buffers fit moves them with one DMA copy each way instead
    // of the runtime's pageable path (per-packet latency)
    void* h_stage = nullptr;
    size_t h_stage_bytes = 0;
    unsigned long long* d_counters = nullptr;  // kCounters slots (lphy_testing.h: kCtr*)
    size_t stage_bytes = 0;
    // the streaming entry point's pinned slots and streams (lphy_stream.hip),
    // made by its first call, kept for the next ones, freed with the context
    void* stream_ext = nullptr;
    void (*stream_ext_free)(void*) = nullptr;
    // smallest batch the fused kernels take on this context (-1: the measured
    // per-SF crossover, fused_min_frames; lphy_hip_ctx_set_fused_min_frames)
    std::atomic<long> fused_min{-1};
    std::atomic<int> mod_force_serial{0};  // (test build: lphy_hip_test_mod_force_serial)
    std::atomic<size_t> pinned_max{kPinnedMax};  // (test build: lphy_hip_test_pinned_max)
    std::atomic<unsigned> grid_cap{0};  // (test build: lphy_hip_test_grid_cap)
    // (per-call scratch of the device entry points - the SF 11-12 speculation
    // records, the producer's phases, the compensation's shift buffer - comes
    // from the stream-ordered allocator on the caller's stream, so concurrent
    // calls on different streams or threads of one context never share it)
};

namespace {

// Host-side constant tables with the reference's own libm calls.
void make_twiddles(std::vector<std::complex<float>>& tw, int nfft) {
    // kissfft.hh:24-29: exp(i * (i*phinc)), phinc = -2*acos(-1)/nfft in float
    tw.resize(nfft);
    const float phinc = (-2 * std::acos((float)-1)) / nfft;
    for (int i = 0; i < nfft; ++i) tw[i] = std::exp(std::complex<float>(0, i * phinc));
}

void make_downchirp(std::vector<std::complex<float>>& d, int N, float bw_scale) {
    // genChirp(out, N, 1, N, 0, down=true, 1, phase=0, bw_scale)
    // (ChirpGenerator.hpp:24-51)
    d.resize(N);
    const float fMin = -kPi * bw_scale / 1;
    const float fMax = kPi * bw_scale / 1;
    const float fStep = (2 * kPi * bw_scale) / (N * 1 * 1);
    float f = fMin + 0.0f;
    float phase = 0.0f;
    for (int i = 0; i < N; ++i) {
        f += fStep;
        if (f > fMax) f -= (fMax - fMin);
        phase -= f;
        d[i] = std::polar(1.0f, phase);
    }
}

void make_hann(std::vector<float>& w, int N) {
    // LoRaDemod.cpp:17-21 / phy.cpp:37-42
    w.resize(N);
    for (int i = 0; i < N; ++i)
        w[i] = 0.5f - 0.5f * std::cos(2.0f * kPi * static_cast<float>(i) /
                                      (static_cast<float>(N) - 1.0f));
}

const SfOps* sf_ops(unsigned sf) {
    static const SfOps* const t[13] = {nullptr,    &sf_ops_1, &sf_ops_2, &sf_ops_3,  &sf_ops_4,
                                       &sf_ops_5,  &sf_ops_6, &sf_ops_7, &sf_ops_8,  &sf_ops_9,
                                       &sf_ops_10, &sf_ops_11, &sf_ops_12};
    return sf >= 1 && sf <= 12 && t[sf]->demod ? t[sf] : nullptr;
}

// LPHY_F_DEBUG_RECHECK (tests): every frame the prologue estimated (status
// 0) is marked as if another workgroup had already left a sentinel in it, the
// state a symbol of the separate launches may observe at any time
// (sym_ctx); k_post's recheck then finds no sentinel and clears the mark.
__global__ void k_mark_recheck(lphy_frame_meta* meta, unsigned long long frames) {
    const unsigned long long f = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < frames && meta[f].status == 0) meta[f].status = kStatusRecheck;
}

// lphy_hip_decode_batch: the finalisation alone (k_post runs it after the
// re-runs of a demodulation), a workgroup per 256 frames
__global__ __launch_bounds__(kTile) void k_finalize(FinalArgs A) {
    __shared__ FinStage st;
    if (blockDim.x == kTile && finalize_block(A, (unsigned long long)blockIdx.x * kTile, st)) return;
    const unsigned long long f = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < A.frames) finalize_frame(A, f);
}

// The separate launches: prologue and / or symbols.  Under
// LPHY_F_DEBUG_RECHECK the mark goes between the two, on the same stream.
int launch_demod(const SfOps* o, const DemodArgs& A, hipStream_t st, bool pro, bool sym) {
    if (!(A.debug_recheck && sym)) return o->demod(A, st, pro, sym, 0);
    if (pro) {
        if (int rc = o->demod(A, st, true, false, 0)) return rc;
    }
    hipLaunchKernelGGL(k_mark_recheck, dim3((unsigned)((A.frames + kTile - 1) / kTile)), dim3(kTile), 0, st, A.meta,
                       A.frames);
    return o->demod(A, st, false, true, 0);
}

// Smallest batch the fused kernels take.  They give each frame one
// wavefront that walks its symbols in order, so a small batch leaves most
// of the GPU idle and the separate launches (symbol-parallel k_demod) finish
// first.  Crossovers measured per SF, mode 2 with decode, device time per
// call (tools/fused_crossover.py, profiles/r5/fused_crossover.json: with
// k_wave at SF 7-12 the fused kernel wins from 256 frames at SF 7-10, from
// 512 at SF 11-12, where 256 is a tie); the per-packet latency of the
// lora_phy:: API rides on the small end.  A context's own setting
// (lphy_hip_ctx_set_fused_min_frames) wins; the test build also reads a
// process default from LPHY_FUSED_MIN_FRAMES.
size_t fused_min_frames(const lphy_hip_ctx* c) {
    const long own = c->fused_min.load(std::memory_order_relaxed);
    if (own >= 0) return (size_t)own;
    const long test = lphy_test_fused_min_frames();
    if (test >= 0) return (size_t)test;
    static const size_t t[13] = {256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 384, 384};
    return t[c->sf <= 12 ? c->sf : 12];
}

int ensure_stage(lphy_hip_ctx* c, size_t bytes) {
    if (c->stage_bytes >= bytes) return 0;
    void* old = c->d_stage;
    c->d_stage = nullptr;
    c->stage_bytes = 0;
    if (old) HIP_OK(hipFree(old));
    HIP_OK(hipMalloc(&c->d_stage, bytes));
    c->stage_bytes = bytes;
    const size_t hb = std::min(bytes, kPinnedMax);
    if (hb > c->h_stage_bytes) {
        if (c->h_stage) HIP_OK(hipHostFree(c->h_stage));
        c->h_stage = nullptr;
        c->h_stage_bytes = 0;
        if (hipHostMalloc(&c->h_stage, hb, hipHostMallocDefault) == hipSuccess) c->h_stage_bytes = hb;
        else c->h_stage = nullptr;  // no pinned mirror: the calls take the pageable path
    }
    return 0;
}

// Per-call device scratch of the device-buffer entry points, one policy for
// all of them (demod_batch's SF 11-12 speculation records, the producer's
// phases, the compensation's shift buffer): allocated and released in the
// caller's stream order (hipMallocAsync / hipFreeAsync from the stream-
// ordered pool, the null stream included), so its lifetime is exactly the
// call's kernels and no caller synchronises.  (Round 2-3 kept a plain
// hipMalloc plus a stream sync for the producers on the null stream, over a
// transcript that read a recycled block once and was never reproduced;
// round 3 removed the scratch-lowered table that was its likely cause,
// DESIGN §8.)  The *_host entry points lend a slice of their reserved
// staging instead (they run on the context's own stream and synchronise it
// before returning).
struct StreamScratch {
    void* p = nullptr;
    hipStream_t st;
    bool owned = false, pooled = false, pool_null = false;
    explicit StreamScratch(hipStream_t s, void* lent = nullptr, bool pool_on_null = true)
        : p(lent), st(s), pool_null(pool_on_null) {}
    int get(size_t bytes) {
        if (p) return 0;  // lent by the caller
        pooled = st != nullptr || pool_null;
        const hipError_t e = pooled ? hipMallocAsync(&p, bytes, st) : hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            return -ENOMEM;
        }
        owned = true;
        return 0;
    }
    ~StreamScratch() {
        if (!owned) return;
        if (pooled) {
            (void)hipFreeAsync(p, st);
        } else {
            (void)hipStreamSynchronize(st);
            (void)hipFree(p);
        }
    }
};

// The fields of DemodArgs / DetectArgs that come from the context alone.
template <class ARGS>
void ctx_args(const lphy_hip_ctx* c, ARGS& A) {
    A.tw = c->d_tw;
    A.down = c->d_down;
    A.win = c->window == LPHY_WINDOW_HANN ? c->d_win : nullptr;
    A.power_scale = c->power_scale;
    A.counters = c->d_counters;
}

// Most workgroups the persistent grids of k_rg_demod, k_detect (both geometries) and
// k_tx_samples get on this context (0: no cap; test build only,
// lphy_hip_test_grid_cap).
unsigned test_grid_cap(const lphy_hip_ctx* c) {
#ifdef LPHY_TEST_PATHS
    return c->grid_cap.load(std::memory_order_relaxed);
#else
    (void)c;
    return 0;
#endif
}

// Counters [first, first + n) of the context after everything on the device
// is done, cleared with `reset`.
int read_counters(lphy_hip_ctx* c, int first, int n, unsigned long long* out, int reset) {
    if (!c || !out) return -EINVAL;
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, c->d_counters + first, n * sizeof(*out), hipMemcpyDeviceToHost));
    if (reset) HIP_OK(hipMemset(c->d_counters + first, 0, n * sizeof(*out)));
    return 0;
}

}  // namespace

extern "C" {

const char* lphy_hip_version(void) {
#if defined(LPHY_TEST_PATHS) && defined(LPHY_DEBUG_BOUNDS)
    return "lphy_hip 0.2 gfx950 test+bounds";
#elif defined(LPHY_TEST_PATHS)
    return "lphy_hip 0.2 gfx950 test";
#else
    return "lphy_hip 0.2 gfx950";
#endif
}

// Internal (not in include/lphy_hip.h): the context's HIP device, for the
// streaming ingestion in lphy_stream.hip.
int lphy_hip_ctx_device(const lphy_hip_ctx* c) { return c ? c->device : -1; }

// Internal: the streaming ingestion's state kept with the context (made by
// `make` on first use, released by `destroy` with the context).
void* lphy_hip_ctx_stream_ext(lphy_hip_ctx* c, void* (*make)(), void (*destroy)(void*)) {
    if (!c) return nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->stream_ext) {
        c->stream_ext = make();
        c->stream_ext_free = destroy;
    }
    return c->stream_ext;
}

namespace {
// A context's own state: the host entry points' stream and the counters
// (the tables are set by the caller).
int ctx_own_state(lphy_hip_ctx* c) {
    if (hipMalloc(&c->d_counters, kCounters * sizeof(unsigned long long)) != hipSuccess) return -ENOMEM;
    HIP_OK(hipMemset(c->d_counters, 0, kCounters * sizeof(unsigned long long)));
    HIP_OK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    return 0;
}
}  // namespace

int lphy_hip_ctx_create(lphy_hip_ctx** out, int device, unsigned sf, unsigned bw_hz,
                        unsigned osr, int window) {
    if (!out) return -EINVAL;
    *out = nullptr;
    if (sf < 1 || sf > 12) return -EINVAL;
    if (bw_hz != 125000 && bw_hz != 250000 && bw_hz != 500000) return -EINVAL;
    if (osr == 0) osr = 1;
    if (osr > 64) return -EINVAL;
    if (window != LPHY_WINDOW_NONE && window != LPHY_WINDOW_HANN) return -EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -ENODEV;
    HIP_OK(hipSetDevice(device));
    auto* c = new lphy_hip_ctx;
    c->device = device;
    c->sf = sf;
    c->N = 1u << sf;
    c->bw_hz = bw_hz;
    c->osr = osr;
    c->window = window;
    c->power_scale = (float)(20.0 * std::log10((double)c->N));  // LoRaDetector.hpp:29
    c->tab = std::make_shared<lphy_tables>();
    lphy_tables& t = *c->tab;
    t.device = device;
    std::vector<std::complex<float>> tw, down;
    make_twiddles(tw, (int)c->N);
    make_downchirp(down, (int)c->N, (float)bw_hz / 125000.0f);
    if (hipMalloc(&t.d_tw, c->N * sizeof(cf32)) != hipSuccess ||
        hipMalloc(&t.d_down, c->N * sizeof(cf32)) != hipSuccess ||
        (window == LPHY_WINDOW_HANN && hipMalloc(&t.d_win, c->N * sizeof(float)) != hipSuccess)) {
        lphy_hip_ctx_destroy(c);
        return -ENOMEM;
    }
    c->d_tw = t.d_tw;
    c->d_down = t.d_down;
    c->d_win = t.d_win;
    if (int rc = ctx_own_state(c)) {
        lphy_hip_ctx_destroy(c);
        return rc;
    }
    HIP_OK(hipMemcpy(t.d_tw, tw.data(), c->N * sizeof(cf32), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(t.d_down, down.data(), c->N * sizeof(cf32), hipMemcpyHostToDevice));
    if (window == LPHY_WINDOW_HANN) {
        std::vector<float> w;
        make_hann(w, (int)c->N);
        HIP_OK(hipMemcpy(t.d_win, w.data(), c->N * sizeof(float), hipMemcpyHostToDevice));
    }
    *out = c;
    return 0;
}

int lphy_hip_ctx_share(lphy_hip_ctx** out, const lphy_hip_ctx* base, unsigned osr) {
    if (!out || !base) return -EINVAL;
    *out = nullptr;
    if (osr == 0) osr = base->osr;
    if (osr > 64) return -EINVAL;
    HIP_OK(hipSetDevice(base->device));
    auto* c = new lphy_hip_ctx;
    c->device = base->device;
    c->sf = base->sf;
    c->N = base->N;
    c->bw_hz = base->bw_hz;
    c->osr = osr;  // the tables depend on N only
    c->window = base->window;
    c->power_scale = base->power_scale;
    c->tab = base->tab;
    c->d_tw = base->d_tw;
    c->d_down = base->d_down;
    c->d_win = base->d_win;
    if (int rc = ctx_own_state(c)) {
        lphy_hip_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return 0;
}

// Internal (not in include/lphy_hip.h): the oversampling ratio of a context
// the caller owns alone (the C++ shim's per-workspace contexts; the
// reference's lora_demodulate takes osr per call).  The tables depend on N
// only.
int lphy_hip_ctx_set_osr(lphy_hip_ctx* c, unsigned osr) {
    if (!c || osr == 0 || osr > 64) return -EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->osr = osr;
    return 0;
}

void lphy_hip_ctx_destroy(lphy_hip_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamDestroy(c->stream);
    }
    if (c->stream_ext && c->stream_ext_free) c->stream_ext_free(c->stream_ext);
    if (c->d_stage) (void)hipFree(c->d_stage);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->d_counters) (void)hipFree(c->d_counters);
    c->tab.reset();  // the tables go with the last context holding them
    delete c;
}

int lphy_hip_ctx_set_fused_min_frames(lphy_hip_ctx* c, long frames) {
    if (!c) return -EINVAL;
    c->fused_min.store(frames < 0 ? -1L : frames, std::memory_order_relaxed);
    return 0;
}

size_t lphy_hip_syms_per_frame(const lphy_hip_ctx* c, size_t frame_samples, int mode) {
    return c ? ragged_out_syms(frame_samples / ((size_t)c->N * c->osr), mode) : 0;
}

namespace {
// what the ragged entry points' argument checks read of a context (lphy_ragged_layout.h)
RaggedCtx ragged_ctx(const lphy_hip_ctx* c) { return c ? RaggedCtx{true, c->sf, c->osr} : RaggedCtx{}; }

int demod_batch_impl(lphy_hip_ctx* c, const float* d_iq, size_t frames, size_t frame_samples,
                     uint16_t* d_syms, uint8_t* d_bytes, lphy_frame_meta* d_meta, int mode,
                     unsigned flags, hipStream_t st, void* lent_spec);
}

int lphy_hip_demod_batch(lphy_hip_ctx* c, const float* d_iq, size_t frames,
                         size_t frame_samples, uint16_t* d_syms, uint8_t* d_bytes,
                         lphy_frame_meta* d_meta, int mode, unsigned flags, void* stream) {
    return demod_batch_impl(c, d_iq, frames, frame_samples, d_syms, d_bytes, d_meta, mode, flags,
                            (hipStream_t)stream, nullptr);
}

namespace {
// lent_spec: frames * 16 bytes of speculation records the caller owns
// (the *_host entry point's staging), else per-call pooled scratch.
int demod_batch_impl(lphy_hip_ctx* c, const float* d_iq, size_t frames, size_t frame_samples,
                     uint16_t* d_syms, uint8_t* d_bytes, lphy_frame_meta* d_meta, int mode,
                     unsigned flags, hipStream_t st, void* lent_spec) {
    if (!c || !d_iq || !d_meta || !d_syms) return -EINVAL;
    if (mode < 0 || mode > 2) return -EINVAL;
#ifndef LPHY_TEST_PATHS
    if (flags & kTestFlags) return -EINVAL;  // comparison paths: test build only
#endif
    if ((flags & LPHY_F_DECODE) && !d_bytes) return -EINVAL;
    if (frames == 0) return 0;
    const size_t step = (size_t)c->N * c->osr;
    const size_t total = frame_samples / step;
    if (mode == LPHY_MODE_DEMODULATE) {
        // phy.cpp:190-194
        if (frame_samples % step != 0) return -EINVAL;
        if (total < 2) return -ERANGE;
    }
    if (mode == LPHY_MODE_DECHIRP_LORA_DEMODULATE && (c->osr != 1 || frame_samples % c->N)) return -EINVAL;
    HIP_OK(hipSetDevice(c->device));
    DemodArgs A{};
    ctx_args(c, A);
    A.iq = reinterpret_cast<const cf32*>(d_iq);
    A.syms = d_syms;
    A.meta = d_meta;
    A.frames = frames;
    A.frame_samples = frame_samples;
    A.total_syms = total;
    A.out_per_frame = lphy_hip_syms_per_frame(c, frame_samples, mode);
    A.osr = (int)c->osr;
    A.mode = mode;
    A.no_scratch = (flags & LPHY_F_NO_SCRATCH) ? 1 : 0;
    A.exact_rotation = (flags & LPHY_F_EXACT_ROTATION) ? 1 : 0;
    A.spec = (mode != LPHY_MODE_DEMODULATE && !A.no_scratch && !(flags & LPHY_F_SCAN_FIRST)) ? 1 : 0;
    A.debug_recheck = (flags & LPHY_F_DEBUG_RECHECK) ? 1 : 0;
    A.est_units = (int)(ragged_est_syms(total, mode) * c->osr);
    // 32-bit symbol / sample bookkeeping in the kernels
    if (frames > 0x7fffffffULL || frames * (total ? total : 1) >= 0xffffffffULL ||
        frame_samples >= 0x7fffffffULL)
        return -ERANGE;
    const unsigned stages = flags & (LPHY_F_STAGE_PROLOGUE | LPHY_F_STAGE_SYMBOLS | LPHY_F_STAGE_FINAL);
    const bool all = stages == 0;
    // one fused launch for prologue + symbols when the call's shape allows it
    // (lphy_route.h); selecting exactly those two stages runs it alone
    const unsigned both = LPHY_F_STAGE_PROLOGUE | LPHY_F_STAGE_SYMBOLS;
    // (Measured alternative: the separate kernels pipelined over chunks on
    // two streams, prologue of chunk c+1 beside the symbol kernel of chunk
    // c: the co-running kernels slowed each other ~2x, 1.1x slower overall.)
    const Path path = route({c->sf, c->osr, mode, A.win != nullptr, total, A.est_units, frames, fused_min_frames(c),
                             A.spec != 0, A.exact_rotation != 0, flags});
    const bool fused = path != Path::Separate;
    A.wave = path == Path::Wave ? 1 : 0;
    const SfOps* ops = sf_ops(c->sf);
    if (!ops) return fused ? -ENOTSUP : -EINVAL;  // (an experiment build without this SF's object)
    // SF 11-12 separate launches, modes 1/2: the speculative normalisation
    // of k_frames across workgroups (k_maxabs scans the two estimate
    // symbols, k_demod folds the rest, k_post closes each frame); needs the
    // prologue, the symbols and the fix-up in this one call
    // (per call, in the caller's stream order: released after this call's
    // last kernel, k_post, which is launched below while `spec` is in scope)
    StreamScratch spec(st, lent_spec);
    if (!fused && A.spec && c->sf >= 11 && c->osr == 1 && !A.exact_rotation && total >= 2 &&
        (all || (stages & both) == both)) {
        if (int rc = spec.get(frames * sizeof(uint4))) return rc;
        A.spec_big = static_cast<uint4*>(spec.p);
    }
    int rc = path == Path::Wave     ? ops->wave(A, st)
             : path == Path::Frames ? ops->frames(A, st)
                                    : launch_demod(ops, A, st, all || (stages & LPHY_F_STAGE_PROLOGUE),
                                                   all || (stages & LPHY_F_STAGE_SYMBOLS));
    if (rc) return rc;
    // exact re-run of flagged frames (part of the symbols stage) and the
    // per-frame finalisation, in one launch
    const bool fix = all || (stages & LPHY_F_STAGE_SYMBOLS);
    const bool fin = all || (stages & LPHY_F_STAGE_FINAL);
    if (!fix && !fin) return 0;
    FinalArgs F{};
    F.syms = d_syms;
    F.bytes = d_bytes;
    F.meta = d_meta;
    F.frames = frames;
    F.nsyms = A.out_per_frame;
    F.sym_stride = A.out_per_frame;
    F.shift = c->sf > 4 ? (int)c->sf - 4 : 0;
    F.decode = (flags & LPHY_F_DECODE) ? 1 : 0;
    F.set_sync = 1;
    return ops->post(mode, A, F, fix, fin, st);
}
}  // namespace

// ---- ragged batches (lphy_ragged.h) ---------------------------------------
int lphy_hip_ragged_layout(const lphy_hip_ctx* c, const uint64_t* h_samples, size_t frames, int mode,
                           lphy_ragged_desc* h_desc) {
    if (!c) return -EINVAL;
    return ragged_layout((uint64_t)c->N * c->osr, h_samples, frames, mode, h_desc);
}

namespace {
// units_hint: the call's whole symbols when the caller's table is on the host
int demod_ragged_impl(lphy_hip_ctx* c, const float* d_iq, const lphy_ragged_desc* d_desc, size_t frames,
                      uint16_t* d_syms, uint8_t* d_bytes, lphy_frame_meta* d_meta, int mode, unsigned flags,
                      hipStream_t st, unsigned long long units_hint) {
    const SfOps* ops = sf_ops(c->sf);
    if (!ops || !ops->ragged) return -ENOTSUP;  // (an experiment build without this SF's object)
    HIP_OK(hipSetDevice(c->device));
    RaggedArgs R{};
    DemodArgs& A = R.A;
    ctx_args(c, A);
    A.iq = reinterpret_cast<const cf32*>(d_iq);
    A.syms = d_syms;
    A.meta = d_meta;
    A.frames = frames;
    A.osr = 1;
    A.mode = mode;
    A.no_scratch = (flags & LPHY_F_NO_SCRATCH) ? 1 : 0;
    A.exact_rotation = 1;
    R.desc = d_desc;
    R.bytes = (flags & LPHY_F_DECODE) ? d_bytes : nullptr;
    R.units_hint = units_hint;
    R.shift = (int)c->sf - 4;
    R.decode = (flags & LPHY_F_DECODE) ? 1 : 0;
    return ops->ragged(R, st, test_grid_cap(c));
}
}  // namespace

int lphy_hip_demod_ragged(lphy_hip_ctx* c, const float* d_iq, const lphy_ragged_desc* d_desc, size_t frames,
                          uint16_t* d_syms, uint8_t* d_bytes, lphy_frame_meta* d_meta, int mode,
                          unsigned flags, void* stream) {
    if (int rc = demod_ragged_args(ragged_ctx(c), d_iq && d_desc && d_meta && d_syms, mode, flags, d_bytes, frames))
        return rc > 0 ? 0 : rc;
    return demod_ragged_impl(c, d_iq, d_desc, frames, d_syms, d_bytes, d_meta, mode, flags, (hipStream_t)stream, 0);
}

// ---- the detector on a batch of windows (lphy_detect.h) --------------------
namespace {
// The argument checks of both forms, in the header's order; *last is the
// largest sample index the call reads (windows > 0).  rc > 0: nothing to do.
int detect_check(const lphy_hip_ctx* c, const void* iq, size_t total_samples, size_t first, size_t hop,
                 size_t step, size_t windows, const void* out, unsigned flags, size_t* last) {
    if (!c || !iq || !out || hop == 0 || step == 0) return -EINVAL;
    if (flags & ~(unsigned)LPHY_DET_DECHIRP) return -EINVAL;
    if (c->sf < 7) return -ENOTSUP;
    if (windows == 0) return 1;
    if ((unsigned long long)windows >= (1ull << 32)) return -ERANGE;
    // first + (windows - 1) * hop + (N - 1) * step < total_samples, without overflow
    if (total_samples == 0 || first > total_samples - 1) return -ERANGE;
    size_t room = total_samples - 1 - first;
    const size_t n1 = (size_t)c->N - 1;
    if (step > room / n1) return -ERANGE;
    room -= n1 * step;
    if (windows > 1 && hop > room / (windows - 1)) return -ERANGE;
    *last = first + (windows - 1) * hop + n1 * step;
    return 0;
}

int detect_impl(lphy_hip_ctx* c, const float* d_iq, size_t total_samples, size_t first, size_t hop, size_t step,
                size_t windows, lphy_detect_rec* d_out, unsigned flags, hipStream_t st) {
    const SfOps* ops = sf_ops(c->sf);
    if (!ops || !ops->detect) return -ENOTSUP;  // (an experiment build without this SF's object)
    HIP_OK(hipSetDevice(c->device));
    DetectArgs D{};
    ctx_args(c, D);
    D.iq = reinterpret_cast<const cf32*>(d_iq);
    D.out = d_out;
    D.dechirp = (flags & LPHY_DET_DECHIRP) ? 1 : 0;
    return ops->detect(D, DetLattice{first, hop, step, windows, total_samples}, st, test_grid_cap(c));
}
}  // namespace

int lphy_hip_detect_batch(lphy_hip_ctx* c, const float* d_iq, size_t total_samples, size_t first, size_t hop,
                          size_t step, size_t windows, lphy_detect_rec* d_out, unsigned flags, void* stream) {
    size_t last = 0;
    if (int rc = detect_check(c, d_iq, total_samples, first, hop, step, windows, d_out, flags, &last))
        return rc > 0 ? 0 : rc;
    return detect_impl(c, d_iq, total_samples, first, hop, step, windows, d_out, flags, (hipStream_t)stream);
}

// ---- the detector on a ragged table (k_detect over DetRagged, lphy_detect.h)
namespace {
// units_hint: the call's whole symbols when the caller's table is on the host
int detect_ragged_impl(lphy_hip_ctx* c, const float* d_iq, const lphy_ragged_desc* d_desc, size_t frames,
                       unsigned phase, lphy_detect_rec* d_out, unsigned flags, hipStream_t st,
                       unsigned long long units_hint) {
    const SfOps* ops = sf_ops(c->sf);
    if (!ops || !ops->detect_ragged) return -ENOTSUP;  // (an experiment build without this SF's object)
    HIP_OK(hipSetDevice(c->device));
    DetectArgs D{};
    ctx_args(c, D);
    D.iq = reinterpret_cast<const cf32*>(d_iq);
    D.out = d_out;
    D.dechirp = (flags & LPHY_DET_DECHIRP) ? 1 : 0;
    return ops->detect_ragged(D, DetRagged{d_desc, (unsigned)frames, (unsigned)c->osr, phase, units_hint}, st,
                              test_grid_cap(c));
}
}  // namespace

int lphy_hip_detect_ragged(lphy_hip_ctx* c, const float* d_iq, const lphy_ragged_desc* d_desc, size_t frames,
                           unsigned phase, lphy_detect_rec* d_out, unsigned flags, void* stream) {
    if (int rc = detect_ragged_args(ragged_ctx(c), frames, d_iq && d_desc && d_out, phase, flags))
        return rc > 0 ? 0 : rc;
    return detect_ragged_impl(c, d_iq, d_desc, frames, phase, d_out, flags, (hipStream_t)stream, 0);
}

// ---- the frame search (lphy_find.h) ------------------------------------------
size_t lphy_hip_find_frames_workspace(size_t windows) { return find_layout(windows).bytes; }

namespace {
int find_frames_check(const lphy_hip_ctx* c, const void* rec, size_t windows, const lphy_find_params* p, int mode,
                      size_t max_frames, const void* desc, const void* info, bool work) {
    return find_frames_args(ragged_ctx(c), p, desc && info, rec != nullptr, work, c ? (uint64_t)c->N * c->osr : 1,
                            windows, mode, max_frames);
}

// The six launches; the arguments have passed find_frames_check.
int find_frames_impl(lphy_hip_ctx* c, const lphy_detect_rec* d_rec, size_t windows, const lphy_find_params& p, int mode,
                     size_t max_frames, lphy_ragged_desc* d_desc, lphy_find_info* d_info, void* d_work,
                     hipStream_t st) {
    HIP_OK(hipSetDevice(c->device));
    const FindLayout l = find_layout(windows);
    char* w = static_cast<char*>(d_work);
    FindArgs A{};
    A.rec = reinterpret_cast<const uint4*>(d_rec);
    A.windows = windows;
    A.geo = FindGeo{p.first, p.hop, p.lead, p.total_samples, (uint64_t)c->N * c->osr, p.max_gap, p.min_symbols, mode};
    A.threshold = p.threshold_db;
    A.max_frames = (unsigned)max_frames;
    A.desc = d_desc;
    A.info = d_info;
    A.tiles = l.tiles;
    A.totals = reinterpret_cast<FindTotals*>(w + l.totals);
    A.bits = reinterpret_cast<unsigned long long*>(w + l.bits);
    A.sums = reinterpret_cast<FindSum*>(w + l.sums);
    A.carry = reinterpret_cast<uint2*>(w + l.carry);
    A.counts = reinterpret_cast<FindTileCount*>(w + l.counts);
    A.prefix = reinterpret_cast<FindTilePrefix*>(w + l.prefix);
    const unsigned cap = test_grid_cap(c);
    const unsigned g_flags = persistent_grid(resident_blocks<&k_find_flags>(c->device), l.tiles, cap);
    const unsigned g_count = persistent_grid(resident_blocks<&k_find_count>(c->device), l.tiles, cap);
    const unsigned g_write = persistent_grid(resident_blocks<&k_find_write>(c->device), l.tiles, cap);
    const unsigned g_pad =
        persistent_grid(resident_blocks<&k_find_pad>(c->device), ((unsigned long long)max_frames + kTile) / kTile, cap);
    hipLaunchKernelGGL(k_find_flags, dim3(g_flags), dim3(kTile), 0, st, A);
    hipLaunchKernelGGL(k_find_carry, dim3(1), dim3(kTile), 0, st, A);
    hipLaunchKernelGGL(k_find_count, dim3(g_count), dim3(kTile), 0, st, A);
    hipLaunchKernelGGL(k_find_offsets, dim3(1), dim3(kTile), 0, st, A);
    hipLaunchKernelGGL(k_find_write, dim3(g_write), dim3(kTile), 0, st, A);
    hipLaunchKernelGGL(k_find_pad, dim3(g_pad), dim3(kTile), 0, st, A);
    HIP_OK(hipGetLastError());
    return 0;
}
}  // namespace

int lphy_hip_find_frames(lphy_hip_ctx* c, const lphy_detect_rec* d_rec, size_t windows, const lphy_find_params* p,
                         int mode, size_t max_frames, lphy_ragged_desc* d_desc, lphy_find_info* d_info, void* d_work,
                         void* stream) {
    if (int rc = find_frames_check(c, d_rec, windows, p, mode, max_frames, d_desc, d_info,
                                   d_work && ((uintptr_t)d_work & 15) == 0))
        return rc;
    return find_frames_impl(c, d_rec, windows, *p, mode, max_frames, d_desc, d_info, d_work, (hipStream_t)stream);
}

// ---- the channeliser (lphy_chan.h) and the synthesiser (lphy_synth.h) ---------
uint64_t lphy_hip_channelize_outputs(uint64_t in_samples, uint64_t first, uint32_t taps, uint32_t decim) {
    return chan_outputs(in_samples, first, taps, decim);
}
uint64_t lphy_hip_synthesize_outputs(uint64_t in_samples, uint64_t first, uint32_t taps, uint32_t interp) {
    return synth_outputs(in_samples, first, taps, interp);
}

extern "C++" {
namespace {
// Both calls' argument check; a plan that passes with outputs == 0 is done
// (1, for the caller to return 0), as the *_host forms need to know too.
// `args`: chan_args or synth_args.
template <class Plan>
int resample_check(int (*args)(bool, const Plan*, bool, bool, bool, bool), const lphy_hip_ctx* c, const float* in,
                   const Plan* p, const float* taps, const float* rot, const float* out) {
    if (int rc = args(c != nullptr, p, taps && rot, in != nullptr, out != nullptr, res_aligned(in, taps, rot, out)))
        return rc;
    return p->outputs == 0;
}

// The one launch (resample_launch of lphy_chan.h or lphy_synth.h, by the plan's
// type); the plan has passed resample_check and has outputs > 0.
template <class Plan>
int resample_impl(lphy_hip_ctx* c, const float* d_in, const Plan& p, const float* d_taps, const float* d_rot,
                  float* d_out, hipStream_t st) {
    HIP_OK(hipSetDevice(c->device));
    resample_launch(p, d_in, d_taps, d_rot, d_out, st);
    HIP_OK(hipGetLastError());
    return 0;
}

template <class Plan>
int resample_entry(int (*args)(bool, const Plan*, bool, bool, bool, bool), lphy_hip_ctx* c, const float* d_in,
                   const Plan* p, const float* d_taps, const float* d_rot, float* d_out, void* stream) {
    if (int rc = resample_check(args, c, d_in, p, d_taps, d_rot, d_out)) return rc > 0 ? 0 : rc;
    return resample_impl(c, d_in, *p, d_taps, d_rot, d_out, (hipStream_t)stream);
}

// lphy_hip_channelize_raw's argument check and launch, as resample_check and
// resample_impl: chan_args with the format's row and its alignment row
// (chan_raw_aligned), and the kernel of the format.
int chan_raw_check(const lphy_hip_ctx* c, const void* in, int format, const lphy_chan_plan* p, const float* taps,
                   const float* rot, const float* out) {
    if (int rc = chan_args(c != nullptr, p, taps && rot, in != nullptr, out != nullptr,
                           chan_raw_aligned(in, format, taps, rot, out)))
        return rc;
    return p->outputs == 0;
}

int chan_raw_impl(lphy_hip_ctx* c, const void* d_in, int format, const lphy_chan_plan& p, const float* d_taps,
                  const float* d_rot, float* d_out, hipStream_t st) {
    HIP_OK(hipSetDevice(c->device));
    chan_launch(p, d_in, format, d_taps, d_rot, d_out, st);
    HIP_OK(hipGetLastError());
    return 0;
}
}  // namespace
}  // extern "C++"

size_t lphy_hip_sample_bytes(int format) { return chan_sample_bytes(format); }

int lphy_hip_channelize_raw(lphy_hip_ctx* c, const void* d_in, int format, const lphy_chan_plan* p,
                            const float* d_taps, const float* d_rot, float* d_out, void* stream) {
    if (int rc = chan_raw_check(c, d_in, format, p, d_taps, d_rot, d_out)) return rc > 0 ? 0 : rc;
    return chan_raw_impl(c, d_in, format, *p, d_taps, d_rot, d_out, (hipStream_t)stream);
}

int lphy_hip_channelize(lphy_hip_ctx* c, const float* d_in, const lphy_chan_plan* p, const float* d_taps,
                        const float* d_rot, float* d_out, void* stream) {
    return resample_entry(chan_args, c, d_in, p, d_taps, d_rot, d_out, stream);
}
int lphy_hip_synthesize(lphy_hip_ctx* c, const float* d_in, const lphy_synth_plan* p, const float* d_taps,
                        const float* d_rot, float* d_out, void* stream) {
    return resample_entry(synth_args, c, d_in, p, d_taps, d_rot, d_out, stream);
}

int lphy_hip_detect_serial_count(lphy_hip_ctx* c, unsigned long long* out, int reset) {
    return read_counters(c, kCtrDetectSerial, 1, out, reset);
}

#ifdef LPHY_PROFILE_PHASES
// experiments only: read and clear the kernels' per-phase clock sums (8)
int lphy_hip_phase_cycles(lphy_hip_ctx* c, unsigned long long* out8) {
    return read_counters(c, kCtrClocks, 8, out8, 1);
}
#endif

int lphy_hip_decode_batch(lphy_hip_ctx* c, const uint16_t* d_syms, size_t frames,
                          size_t syms_per_frame, uint8_t* d_bytes, lphy_frame_meta* d_meta,
                          void* stream) {
    if (!c || !d_syms || !d_bytes || !d_meta) return -EINVAL;
    if (syms_per_frame & 1) return -EINVAL;
    if (frames == 0) return 0;
    HIP_OK(hipSetDevice(c->device));
    FinalArgs F{};
    F.syms = d_syms;
    F.bytes = d_bytes;
    F.meta = d_meta;
    F.frames = frames;
    F.nsyms = syms_per_frame;
    F.sym_stride = syms_per_frame;
    F.shift = 0;
    F.decode = 1;
    F.set_sync = 0;
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, F);
    HIP_OK(hipGetLastError());
    return 0;
}

int lphy_hip_estimate_batch(lphy_hip_ctx* c, const float* d_iq, size_t frames,
                            size_t frame_samples, size_t est_samples,
                            lphy_frame_meta* d_meta, void* stream) {
    if (!c || !d_iq || !d_meta) return -EINVAL;
    const size_t step = (size_t)c->N * c->osr;
    const size_t syms = est_samples / step;
    if (frames == 0) return 0;
    // the estimate may not leave its frame (the last frame's would leave the buffer)
    if (est_samples > frame_samples) return -EINVAL;
    if (syms == 0) return 0;  // phy.cpp:87,91: nothing written
    if (syms * c->osr > (size_t)INT_MAX) return -ERANGE;  // A.est_units
    HIP_OK(hipSetDevice(c->device));
    DemodArgs A{};
    ctx_args(c, A);
    A.iq = reinterpret_cast<const cf32*>(d_iq);
    A.meta = d_meta;
    A.frames = frames;
    A.frame_samples = frame_samples;
    A.total_syms = frame_samples / step;
    A.osr = (int)c->osr;
    A.mode = LPHY_MODE_DEMODULATE;
    A.est_units = (int)(syms * c->osr);
    const SfOps* o = sf_ops(c->sf);
    return o ? o->estimate(A, (hipStream_t)stream) : -EINVAL;
}

namespace {
int estimate_ragged_impl(lphy_hip_ctx* c, const float* d_iq, const lphy_ragged_desc* d_desc, size_t frames,
                         size_t est_samples, lphy_frame_meta* d_meta, hipStream_t st) {
    const SfOps* ops = sf_ops(c->sf);
    if (!ops || !ops->estimate_ragged) return -ENOTSUP;  // (an experiment build without this SF's object)
    HIP_OK(hipSetDevice(c->device));
    RaggedArgs R{};
    DemodArgs& A = R.A;
    ctx_args(c, A);
    A.iq = reinterpret_cast<const cf32*>(d_iq);
    A.meta = d_meta;
    A.frames = frames;
    A.osr = (int)c->osr;
    A.mode = LPHY_MODE_DEMODULATE;
    R.desc = d_desc;
    return ops->estimate_ragged(R, (unsigned long long)est_samples, st);
}
}  // namespace

int lphy_hip_estimate_ragged(lphy_hip_ctx* c, const float* d_iq, const lphy_ragged_desc* d_desc, size_t frames,
                             size_t est_samples, lphy_frame_meta* d_meta, void* stream) {
    if (int rc = ragged_args(ragged_ctx(c), frames, d_iq && d_desc && d_meta)) return rc > 0 ? 0 : rc;
    return estimate_ragged_impl(c, d_iq, d_desc, frames, est_samples, d_meta, (hipStream_t)stream);
}

namespace {
// compensate_offsets (phy.cpp:150-180) on device samples.  The rotation is
// elementwise and runs in place; only a time shift needs scratch (`lent`,
// when given, is count complex values the caller owns).
int compensate_impl(lphy_hip_ctx* c, float* d_iq, size_t count, float cfo, float time_offset,
                    hipStream_t st, void* lent) {
    // phy.cpp:159-160
    const float rate = -2.0f * kPi * cfo / (static_cast<float>(c->N) * static_cast<float>(c->osr));
    const unsigned blocks = (unsigned)((count + 255) / 256);
    cf32* x = reinterpret_cast<cf32*>(d_iq);
    const float r = std::round(time_offset);  // phy.cpp:167, x86 cvttss2si
    const long long off = (r >= -2147483648.0f && r < 2147483648.0f) ? (long long)(int)r
                                                                     : (long long)(int)0x80000000u;
    if (off == 0 || (unsigned long long)(off > 0 ? off : -off) >= count) {
        hipLaunchKernelGGL(k_comp_rotate, dim3(blocks), dim3(256), 0, st, x, x,
                           (unsigned long long)count, rate);
        HIP_OK(hipGetLastError());
        return 0;
    }
    StreamScratch scratch(st, lent);
    if (int rc = scratch.get(count * sizeof(cf32))) return rc;
    cf32* tmp = static_cast<cf32*>(scratch.p);
    hipLaunchKernelGGL(k_comp_rotate, dim3(blocks), dim3(256), 0, st, tmp, x, (unsigned long long)count, rate);
    hipLaunchKernelGGL(k_comp_shift, dim3(blocks), dim3(256), 0, st, x, tmp, (unsigned long long)count, off);
    HIP_OK(hipGetLastError());
    return 0;
}

// compensate_offsets for every frame of a batch, offsets read on the device
// (k_comp_batch, lphy_mod.h): one launch, no scratch.  `slots` workgroups
// share a frame out of place; in place (d_out == d_in) one owns it and walks
// its tiles in memmove order.
constexpr unsigned long long kCompMaxGrid = 1ull << 22;  // (x 256 threads stays below 2^32)

extern "C++" {
template <class GEO>
int compensate_batch_launch(const lphy_hip_ctx* c, const float* d_in, float* d_out, GEO geo, size_t frames,
                            unsigned slots, const lphy_frame_meta* d_meta, hipStream_t st) {
    const cf32* in = reinterpret_cast<const cf32*>(d_in);
    cf32* out = reinterpret_cast<cf32*>(d_out);
    const bool in_place = d_in == d_out;
    if (in_place) slots = 1;
    const unsigned grid = (unsigned)std::min<unsigned long long>((unsigned long long)frames * slots, kCompMaxGrid);
    if (in_place)
        hipLaunchKernelGGL((k_comp_batch<GEO, true>), dim3(grid), dim3(kTile), 0, st, in, out, geo, d_meta,
                           (unsigned long long)frames, slots, (int)c->N, (int)c->osr);
    else
        hipLaunchKernelGGL((k_comp_batch<GEO, false>), dim3(grid), dim3(kTile), 0, st, in, out, geo, d_meta,
                           (unsigned long long)frames, slots, (int)c->N, (int)c->osr);
    HIP_OK(hipGetLastError());
    return 0;
}
}  // extern "C++"

// The uniform form's argument checks (before any device call): 0 to go on,
// 1 when there is nothing to do, or the error.
int compensate_batch_check(const lphy_hip_ctx* c, const float* in, const float* out, size_t frames,
                           size_t frame_samples, const lphy_frame_meta* meta) {
    if (!c) return -EINVAL;
    if (frames == 0) return 1;
    if (!in || !out || !meta) return -EINVAL;
    if (frames > kRaggedMaxFrames) return -ERANGE;
    if (frame_samples == 0) return 1;
    size_t bytes = 0;
    if (__builtin_mul_overflow(frames, frame_samples, &bytes) || __builtin_mul_overflow(bytes, sizeof(cf32), &bytes))
        return -ERANGE;
    // in place or disjoint; a partial overlap has no order that is right for every frame
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if (a != b && a < b + bytes && b < a + bytes) return -EINVAL;
    return 0;
}

int compensate_batch_impl(const lphy_hip_ctx* c, const float* d_in, float* d_out, size_t frames,
                          size_t frame_samples, const lphy_frame_meta* d_meta, hipStream_t st) {
    // one workgroup per tile (a frame's first output sample may sit half a 16-byte pair in)
    const size_t tiles = (frame_samples + 1 + kCompTile - 1) / kCompTile;
    const unsigned slots = (unsigned)std::min<size_t>(tiles, size_t(1) << 20);
    return compensate_batch_launch(c, d_in, d_out, CompUniform{(unsigned long long)frame_samples}, frames, slots,
                                   d_meta, st);
}

// lora_modulate (LoRaMod.cpp:8-43) for `frames` frames; `lent` (optional)
// holds mod_scratch_bytes(): the per-symbol start phases, and below
// mod_walk_all_below symbols every sample's phase too.
constexpr size_t mod_walk_all_below = 4096;

// k_mod_fast's dynamic LDS limit on the context's device, found once per
// device: the device's LDS per workgroup less the kernel's static LDS
// (ModFastShared), and the kernel's attribute raised to it once, outside the
// per-packet path (the limit was a gfx950 constant, set per call).
size_t mod_fast_lds(int device) {
    // (a device the runtime does not count: the limit no attribute has to be raised for)
    return (size_t)per_device(device, 64 << 10, [](int d) {
        int cur = 0, per_block = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(d);
        (void)hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, d);
        size_t stat = 0;
        hipFuncAttributes fa{};
        if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_mod_fast<false>)) == hipSuccess)
            stat = fa.sharedSizeBytes;
        size_t avail = per_block > 0 && (size_t)per_block > stat ? (size_t)per_block - stat : 0;
        if (avail > kModFastLds) avail = kModFastLds;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_mod_fast<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)avail) != hipSuccess)
            avail = std::min<size_t>(avail, size_t(64) << 10);  // the default limit stands
        (void)hipSetDevice(cur);
        return avail;
    });
}

// Which modulator form a call takes (modulate_impl): 0 the three-kernel or
// batch forms, 1 k_mod_fast with the f rows in LDS, 2 k_mod_fast's split
// form with the f rows in the phase buffer (GROWS: k_mod_fast<true, 1>,
// k_mod_cand, k_mod_fast<true, 3>).
int mod_form(const lphy_hip_ctx* c, size_t frames, size_t nsyms) {
    const size_t ns = nsyms + 2, nph = frames * ns;
    if (nph >=mod_walk_all_below || ns > (size_t)kModFastSyms) return 0;
    const size_t lds = ns * (((size_t)c->N * c->osr + 4) * sizeof(float) + kModFastWin);
    return lds <= mod_fast_lds(c->device) ? 1 : 2;
}

size_t mod_scratch_bytes(const lphy_hip_ctx* c, size_t frames, size_t nsyms) {
    const size_t nph = frames * (nsyms + 2);
    return align_up(nph * sizeof(float)) +
           (nph < mod_walk_all_below ? align_up(nph * (size_t)c->N * c->osr * sizeof(float)) : 0) +
           (mod_form(c, frames, nsyms) == 2
                ? align_up(frames * sizeof(ModFastG)) + align_up(frames * (size_t)kModFastSyms * kModFastWin)
                : 0);
}

int modulate_impl(lphy_hip_ctx* c, const uint16_t* d_syms, size_t frames, size_t nsyms,
                  float* d_iq, float amplitude, uint8_t sync, hipStream_t st, void* lent) {
    ModArgs A{};
    A.syms = d_syms;
    A.iq = reinterpret_cast<cf32*>(d_iq);
    A.frames = frames;
    A.nsyms = nsyms;
    A.N = (int)c->N;
    A.osr = (int)c->osr;
    A.bws = (float)c->bw_hz / 125000.0f;
    A.ampl = std::max(-1.0f, std::min(1.0f, amplitude));  // LoRaMod.cpp:18
    A.sync = sync;
    A.slow = c->d_counters + kCtrModSerial;  // lphy_hip_test_counter(kCtrModSerial)
#ifdef LPHY_TEST_PATHS
    A.force_serial = c->mod_force_serial.load(std::memory_order_relaxed);
#endif
    const size_t nph = frames * (nsyms + 2);
    const size_t samples = nph * (size_t)c->N * c->osr;
    // few symbols: every sample's phase from the walk, then sample-parallel
    // sincos (a per-symbol pass would run a handful of threads N steps each)
    const bool walk_all = nph < mod_walk_all_below;
    const int form = mod_form(c, frames, nsyms);
    StreamScratch scratch(st, lent);
    if (int rc = scratch.get(mod_scratch_bytes(c, frames, nsyms))) return rc;
    A.phase0 = static_cast<float*>(scratch.p);
    A.phases = walk_all ? reinterpret_cast<float*>(static_cast<char*>(scratch.p) + align_up(nph * sizeof(float)))
                        : nullptr;
    if (form == 2) {
        char* g = static_cast<char*>(scratch.p) + align_up(nph * sizeof(float)) + align_up(samples * sizeof(float));
        A.mfg = reinterpret_cast<ModFastG*>(g);
        A.mft = reinterpret_cast<unsigned char*>(g + align_up(frames * sizeof(ModFastG)));
        A.blk = (int)(nsyms + 2);  // (k_mod_fast<true>'s interleaved rows, read so by k_mod_sincos)
    }
    // ... then the walk by candidate windows and a chain of lookups
    // (k_mod_fast): with the f rows in LDS when they fit there beside the
    // kernel's static LDS (up to SF 9 at 66 symbols), else in A.phases
    // (k_mod_fast<true, 1> / k_mod_cand / k_mod_fast<true, 3>), then the sincos
    const int stride = (int)(c->N * c->osr) + 4;
    const size_t ns = nsyms + 2;
    const size_t lds = ns * ((size_t)stride * sizeof(float) + kModFastWin);
    if (form == 1 || form == 2) {
        if (form == 1) {
            hipLaunchKernelGGL((k_mod_fast<false>), dim3((unsigned)frames), dim3(kModFastThreads), lds, st, A, stride);
        } else {
            // (the candidate walks, 64 per symbol boundary, are 64x the work of
            // a row walk: across the GPU, between the two halves)
            const int step = (int)(c->N * c->osr);
            hipLaunchKernelGGL((k_mod_fast<true, 1>), dim3((unsigned)frames), dim3(kModFastThreads), 0, st, A, step);
            hipLaunchKernelGGL(k_mod_cand, dim3((unsigned)(frames * ((ns - 1 + 3) / 4))), dim3(256), 0, st, A);
            hipLaunchKernelGGL((k_mod_fast<true, 3>), dim3((unsigned)frames), dim3(kModFastThreads), 0, st, A, step);
        }
        hipLaunchKernelGGL(k_mod_sincos, dim3((unsigned)((samples + 255) / 256)), dim3(256), 0, st, A,
                           (unsigned long long)samples);
    } else if (walk_all) {
        hipLaunchKernelGGL(k_mod_freq, dim3((unsigned)((nph + 63) / 64)), dim3(64), 0, st, A);
        hipLaunchKernelGGL(k_mod_accumulate, dim3((unsigned)((frames + 63) / 64)), dim3(64), 0, st, A);
        hipLaunchKernelGGL(k_mod_sincos, dim3((unsigned)((samples + 255) / 256)), dim3(256), 0, st, A,
                           (unsigned long long)samples);
    } else {
        hipLaunchKernelGGL(k_mod_walk, dim3((unsigned)((frames + 63) / 64)), dim3(64), 0, st, A);
        hipLaunchKernelGGL(k_mod_samples, dim3((unsigned)((nph + 63) / 64)), dim3(64), 0, st, A);
    }
    HIP_OK(hipGetLastError());
    return 0;
}
}  // namespace

int lphy_hip_compensate(lphy_hip_ctx* c, float* d_iq, size_t count, float cfo,
                        float time_offset, void* stream) {
    if (!c || !d_iq) return -EINVAL;
    if (count == 0) return 0;
    HIP_OK(hipSetDevice(c->device));
    return compensate_impl(c, d_iq, count, cfo, time_offset, (hipStream_t)stream, nullptr);
}

int lphy_hip_compensate_batch(lphy_hip_ctx* c, const float* d_in, float* d_out, size_t frames,
                              size_t frame_samples, const lphy_frame_meta* d_meta, void* stream) {
    if (int rc = compensate_batch_check(c, d_in, d_out, frames, frame_samples, d_meta)) return rc > 0 ? 0 : rc;
    HIP_OK(hipSetDevice(c->device));
    return compensate_batch_impl(c, d_in, d_out, frames, frame_samples, d_meta, (hipStream_t)stream);
}

int lphy_hip_compensate_ragged(lphy_hip_ctx* c, const float* d_in, float* d_out, const lphy_ragged_desc* d_desc,
                               size_t frames, const lphy_frame_meta* d_meta, void* stream) {
    if (int rc = ragged_args(ragged_ctx(c), frames, d_in && d_out && d_desc && d_meta, 0)) return rc > 0 ? 0 : rc;
    HIP_OK(hipSetDevice(c->device));
    return compensate_batch_launch(c, d_in, d_out, CompRagged{d_desc}, frames, kCompRaggedSlots, d_meta,
                                   (hipStream_t)stream);
}

int lphy_hip_modulate_batch(lphy_hip_ctx* c, const uint16_t* d_syms, size_t frames,
                            size_t nsyms, float* d_iq, float amplitude, uint8_t sync,
                            void* stream) {
    if (!c || !d_iq || (nsyms && !d_syms)) return -EINVAL;
    if (frames == 0) return 0;
    HIP_OK(hipSetDevice(c->device));
    return modulate_impl(c, d_syms, frames, nsyms, d_iq, amplitude, sync, (hipStream_t)stream,
                         nullptr);
}

// ---- ragged transmit (lphy_tx.h) -------------------------------------------
int lphy_hip_tx_layout(const lphy_hip_ctx* c, const uint64_t* h_len_bytes, size_t frames,
                       lphy_ragged_desc* h_desc) {
    if (!c) return -EINVAL;
    return tx_layout((uint64_t)c->N * c->osr, h_len_bytes, frames, h_desc);
}

// lphy_hip_tx_layout on the lengths of the LoRaWAN frames of h_tx
// (lphy_lorawan_ragged.h); the calls that build and parse them are context-free
// (lphy_lorawan.hip) and take N * osr from lphy_hip_symbol_samples.
int lphy_hip_lorawan_tx_layout(const lphy_hip_ctx* c, const lphy_lorawan_tx* h_tx, size_t frames,
                               lphy_ragged_desc* h_desc) {
    if (!c) return -EINVAL;
    return lw_tx_layout((uint64_t)c->N * c->osr, h_tx, frames, h_desc);
}

size_t lphy_hip_symbol_samples(const lphy_hip_ctx* c) { return c ? (size_t)c->N * c->osr : 0; }

namespace {
extern "C++" {
// The two launches.  units_hint: the call's whole symbols when the caller's
// table is on the host (the sample pass's grid then stops at its tiles).
template <class SRC>
int tx_launch(const lphy_hip_ctx* c, SRC src, const lphy_ragged_desc* d_desc, size_t frames, float* d_iq,
              uint16_t* d_syms_out, float amplitude, uint8_t sync, hipStream_t st, unsigned long long units_hint) {
    TxArgs A{};
    A.desc = d_desc;
    A.iq = reinterpret_cast<cf32*>(d_iq);
    A.syms_out = d_syms_out;
    A.frames = (unsigned)frames;
    A.N = (int)c->N;
    A.osr = (int)c->osr;
    A.shift = (int)c->sf - 4;
    A.bws = (float)c->bw_hz / 125000.0f;
    A.ampl = std::max(-1.0f, std::min(1.0f, amplitude));  // LoRaMod.cpp:18
    A.sync = sync;
    // (the device form does not know the call's units: units_hint 0)
    const unsigned grid = persistent_grid(resident_blocks<&k_tx_samples<SRC>>(c->device),
                                          (units_hint + kTile - 1) / kTile, test_grid_cap(c));
    hipLaunchKernelGGL(k_tx_walk<SRC>, dim3((unsigned)((frames + 63) / 64)), dim3(64), 0, st, A, src);
    hipLaunchKernelGGL(k_tx_samples<SRC>, dim3(grid), dim3(kTile), 0, st, A, src);
    HIP_OK(hipGetLastError());
    return 0;
}
}  // extern "C++"
}  // namespace

int lphy_hip_modulate_ragged(lphy_hip_ctx* c, const uint16_t* d_syms, const lphy_ragged_desc* d_desc, size_t frames,
                             float* d_iq, float amplitude, uint8_t sync, void* stream) {
    if (int rc = ragged_args(ragged_ctx(c), frames, d_syms && d_desc && d_iq)) return rc > 0 ? 0 : rc;
    HIP_OK(hipSetDevice(c->device));
    return tx_launch(c, TxSymbols{d_syms}, d_desc, frames, d_iq, nullptr, amplitude, sync, (hipStream_t)stream, 0);
}

int lphy_hip_tx_ragged(lphy_hip_ctx* c, const uint8_t* d_bytes, const lphy_ragged_desc* d_desc, size_t frames,
                       float* d_iq, uint16_t* d_syms_out, float amplitude, uint8_t sync, void* stream) {
    if (int rc = ragged_args(ragged_ctx(c), frames, d_bytes && d_desc && d_iq)) return rc > 0 ? 0 : rc;
    HIP_OK(hipSetDevice(c->device));
    return tx_launch(c, TxBytes{d_bytes}, d_desc, frames, d_iq, d_syms_out, amplitude, sync, (hipStream_t)stream, 0);
}

int lphy_hip_sync(void* stream) {
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int lphy_hip_recheck_count(lphy_hip_ctx* c, unsigned long long* out, int reset) {
    return read_counters(c, kCtrRecheck, 1, out, reset);
}

#ifdef LPHY_TEST_PATHS
// Test build only (csrc/lphy_testing.h): the context's device counter `idx`
// (kCtrParseval: symbols the wave kernels certified by Parseval; kCtrModSerial:
// frames k_mod_fast walked serially).  Synchronises.
// Test build only: every k_mod_fast frame takes the serial walk (its
// fallback, otherwise reached only when a candidate chain leaves its windows).
int lphy_hip_test_mod_force_serial(lphy_hip_ctx* c, int on) {
    if (!c) return -EINVAL;
    c->mod_force_serial.store(on ? 1 : 0, std::memory_order_relaxed);
    return 0;
}

// Test build only: the largest call (its copied slices) that goes through the
// pinned mirror on this context; 0 sends every *_host call down the pageable
// path, which otherwise needs a call above kPinnedMax (lphy_host.h).
int lphy_hip_test_pinned_max(lphy_hip_ctx* c, size_t bytes) {
    if (!c) return -EINVAL;
    c->pinned_max.store(bytes, std::memory_order_relaxed);
    return 0;
}

// Test build only: at most `blocks` workgroups in the persistent grids of
// k_rg_demod, k_detect (both geometries), k_tx_samples and the frame search on this context, after the launchers'
// own caps (0: the default).  A small call then walks its grid-stride loops
// more than once, which otherwise needs more tiles than the device holds
// workgroups.
int lphy_hip_test_grid_cap(lphy_hip_ctx* c, unsigned blocks) {
    if (!c) return -EINVAL;
    c->grid_cap.store(blocks, std::memory_order_relaxed);
    return 0;
}

int lphy_hip_test_counter(lphy_hip_ctx* c, int idx, unsigned long long* out, int reset) {
    if (idx < 0 || idx >= kCounters) return -EINVAL;
    return read_counters(c, idx, 1, out, reset);
}

namespace {
extern "C++" {
// One element per input, grid-stride; each op calls what the kernels call,
// the way they call it (SPLIT: rotate_sample's choice; SQRTF: unit_result's
// sqrtf; DETECTOR_POWER: lphy_demod.h's function itself).
template <int OP>
__global__ __launch_bounds__(kTile) void k_test_libm(const float* a, const float* b, float* out0, float* out1,
                                                     unsigned long long n) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kTile;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kTile + threadIdx.x; i < n; i += stride) {
        const float x = a[i];
        if constexpr (OP == LPHY_LIBM_SINCOS_EXACT || OP == LPHY_LIBM_SINCOS_SPLIT || OP == LPHY_LIBM_SINCOS_LARGE) {
            float sn, cs;
            if constexpr (OP == LPHY_LIBM_SINCOS_EXACT) {
                lphy_libm::sincosf_exact(x, &sn, &cs);
            } else if constexpr (OP == LPHY_LIBM_SINCOS_SPLIT) {
                const bool large = lphy_libm::sincosf_needs_large(x);
                if (large) lphy_libm::sincosf_large(x, &sn, &cs);
                else lphy_libm::sincosf_fast(x, &sn, &cs);
            } else {
                lphy_libm::sincosf_large(x, &sn, &cs);
            }
            out0[i] = sn;
            out1[i] = cs;
        } else if constexpr (OP == LPHY_LIBM_ATAN2) {
            out0[i] = lphy_libm::atan2f_exact(x, b[i]);
        } else if constexpr (OP == LPHY_LIBM_CABS) {
            out0[i] = lphy_libm::cabsf_exact(x, b[i]);
        } else if constexpr (OP == LPHY_LIBM_LOGF) {
            out0[i] = lphy_libm::logf_exact(x);
        } else if constexpr (OP == LPHY_LIBM_LOG10F) {
            out0[i] = lphy_libm::log10f_exact(x);
        } else if constexpr (OP == LPHY_LIBM_SQRTF) {
            out0[i] = sqrtf(x);
        } else {
            out0[i] = detector_power(x, b[i]);
        }
    }
}
}  // extern "C++"
}  // namespace

// Test build only (csrc/lphy_testing.h): libm_exact.h, the device sqrtf and
// detector_power over the caller's inputs, as this translation unit's flags
// compile them for the device.
int lphy_hip_test_libm(lphy_hip_ctx* c, int op, const float* d_a, const float* d_b, float* d_out0, float* d_out1,
                       size_t n, void* stream) {
    if (!c || !d_a || !d_out0 || op < 0 || op >= LPHY_LIBM_OPS) return -EINVAL;
    const bool two_in = op == LPHY_LIBM_ATAN2 || op == LPHY_LIBM_CABS || op == LPHY_LIBM_DETECTOR_POWER;
    const bool two_out = op <= LPHY_LIBM_SINCOS_LARGE;
    if ((two_in && !d_b) || (two_out && !d_out1)) return -EINVAL;
    if (n == 0) return 0;
    if ((unsigned long long)n >= (1ull << 32)) return -ERANGE;
    HIP_OK(hipSetDevice(c->device));
    const unsigned long long blocks = ((unsigned long long)n + kTile - 1) / kTile;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048)), block(kTile);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned long long count = n;
    switch (op) {
#define LPHY_LIBM_CASE(OP) \
    case OP: hipLaunchKernelGGL(k_test_libm<OP>, grid, block, 0, st, d_a, d_b, d_out0, d_out1, count); break
        LPHY_LIBM_CASE(LPHY_LIBM_SINCOS_EXACT);
        LPHY_LIBM_CASE(LPHY_LIBM_SINCOS_SPLIT);
        LPHY_LIBM_CASE(LPHY_LIBM_SINCOS_LARGE);
        LPHY_LIBM_CASE(LPHY_LIBM_ATAN2);
        LPHY_LIBM_CASE(LPHY_LIBM_CABS);
        LPHY_LIBM_CASE(LPHY_LIBM_LOGF);
        LPHY_LIBM_CASE(LPHY_LIBM_LOG10F);
        LPHY_LIBM_CASE(LPHY_LIBM_SQRTF);
        LPHY_LIBM_CASE(LPHY_LIBM_DETECTOR_POWER);
#undef LPHY_LIBM_CASE
    }
    HIP_OK(hipGetLastError());
    return 0;
}
#endif

int lphy_hip_bounds_violations(lphy_hip_ctx* c, unsigned long long* out, int reset) {
    if (!c || !out) return -EINVAL;
#ifdef LPHY_DEBUG_BOUNDS
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipDeviceSynchronize());
    unsigned long long total = 0;
    for (unsigned sf = 1; sf <= 12; ++sf) {
        const SfOps* o = sf_ops(sf);
        unsigned long long n = 0;
        if (o && o->violations) {
            if (int rc = o->violations(&n, reset)) return rc;
        }
        total += n;
    }
    *out = total;
    return 0;
#else
    *out = 0;
    return -ENOTSUP;
#endif
}

}  // extern "C"

#include "lphy_host.h"
