/*
 * lphy_hip.h — C ABI of the MI355X (gfx950) LoRa PHY demodulation layer.
 *
 * This is the drop-in boundary below the lora_phy:: C++ API
 * (include/lora_phy/phy.hpp, implemented by liblora_phy_amd.so on top of
 * these entry points).  Plain pointers and sizes only; device pointers are
 * hipMalloc'd (or torch) memory, `stream` is a hipStream_t (NULL = default).
 * Every function returns 0 or a negative errno, like the reference.
 *
 * Reference interfaces replaced (file:line under the reference tree):
 *   lphy_hip_ctx_create    lora_phy::init            src/phy/phy.cpp:27-52
 *                          lora_phy::lora_demod_init src/phy/LoRaDemod.cpp:11-33
 *   lphy_hip_ctx_destroy   lora_phy::lora_demod_free src/phy/LoRaDemod.cpp:35-48
 *   lphy_hip_demod_batch   mode LPHY_MODE_DEMODULATE:
 *                            lora_phy::demodulate        src/phy/phy.cpp:182-243
 *                            (+ estimate_offsets          src/phy/phy.cpp:81-148)
 *                          mode LPHY_MODE_LORA_DEMODULATE:
 *                            lora_phy::lora_demodulate   src/phy/LoRaDemod.cpp:50-197
 *                          mode LPHY_MODE_DECHIRP_LORA_DEMODULATE:
 *                            test-side dechirp (tests/e2e_chain_test.cpp:80-93)
 *                            fused in front of lora_demodulate
 *                          flag LPHY_F_DECODE adds, per frame:
 *                            lora_phy::decode / lora_decode src/phy/phy.cpp:245-261,
 *                            src/phy/LoRaDecoder.cpp:7-21
 *   lphy_hip_demod_ragged  the same three modes for frames of different lengths
 *                          in one call (lphy_ragged_desc, below)
 *   lphy_hip_detect_batch  LoRaDetector<float>::detect include/lora_phy/LoRaDetector.hpp:39-74
 *                          over a batch of windows (lphy_detect_rec, below)
 *   lphy_hip_detect_ragged the same on every whole symbol of every frame of
 *                          a ragged table (lphy_ragged_desc, below)
 *   lphy_hip_find_frames   no reference function: the ragged table of the
 *                          frames found in a capture, from those records
 *   lphy_hip_channelize    no reference function: a wideband capture to the
 *                          per-channel streams the calls above take
 *   lphy_hip_channelize_raw  the same from a capture of int16 or 8-bit samples,
 *                            as the radio wrote it (lphy_sample_format, below)
 *   lphy_hip_synthesize    no reference function: per-channel streams (those
 *                          lphy_hip_tx_ragged makes) to one wideband stream
 *   lphy_hip_decode_batch  lora_phy::decode / lora_decode on device symbols
 *   lphy_hip_estimate_batch lora_phy::estimate_offsets src/phy/phy.cpp:81-148
 *   lphy_hip_estimate_ragged the same for frames of different lengths in one
 *                            call (lphy_ragged_desc, below)
 *   lphy_hip_modulate_batch lora_phy::lora_modulate  src/phy/LoRaMod.cpp:8-43
 *                            (producer; bit-exact, used for synthetic IQ)
 *   lphy_hip_modulate_ragged lora_phy::lora_modulate src/phy/LoRaMod.cpp:8-43
 *                            for frames of different lengths in one call
 *   lphy_hip_tx_ragged       lora_phy::lora_encode   src/phy/LoRaEncoder.cpp:6-18
 *                            fused in front of it: bytes in, IQ out
 *   lphy_hip_compensate   lora_phy::compensate_offsets src/phy/phy.cpp:150-180
 *   lphy_hip_compensate_batch  the same for every frame of a batch, each with its
 *   lphy_hip_compensate_ragged own offsets read on the device from its
 *                          lphy_frame_meta (frames of one length / of different
 *                          lengths, lphy_ragged_desc)
 *   lphy_hip_lorawan_build_ragged lorawan::build_frame src/lorawan/lorawan.cpp:100-136
 *   lphy_hip_lorawan_parse_ragged lorawan::parse_frame src/lorawan/lorawan.cpp:138-177
 *                          for frames of different lengths on that table, the
 *                          key found by DevAddr (lphy_lorawan_session)
 *   lphy_hip_lorawan_crypt_batch      no reference function: the FRMPayload
 *   lphy_hip_lorawan_crypt_tx_ragged  cipher of LoRaWAN 1.0.x 4.3.3 on byte
 *   lphy_hip_lorawan_crypt_rx_ragged  ranges, in front of build_ragged and
 *                          behind parse_ragged on that table
 *
 * Batch layout in HBM:
 *   IQ      interleaved float32 (I,Q) = std::complex<float>, frame f at
 *           d_iq + 2*f*frame_samples floats.
 *   symbols uint16, frame f at d_syms + f*lphy_hip_syms_per_frame(...)
 *           (data symbols only when the frame has >= 2 symbols — the two
 *           sync symbols go to lphy_frame_meta.sw0/sw1, as the reference
 *           routes them to ws->sync_word / *out_sync).
 *   bytes   uint8, frame f at d_bytes + f*(data_symbols/2) (LPHY_F_DECODE).
 *   meta    one lphy_frame_meta per frame (also the kernels' hand-off
 *           between the per-frame prologue and the per-symbol demodulator).
 */
#ifndef LPHY_HIP_H
#define LPHY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lphy_hip_ctx lphy_hip_ctx;

/* Per-frame results (32 bytes). */
typedef struct lphy_frame_meta {
    float cfo;          /* ws->metrics.cfo after the call                    */
    float time_offset;  /* ws->metrics.time_offset                           */
    float rate;         /* -2*pi*cfo/N: per-sample CFO rotation              */
    float scale;        /* 1/max(|I|,|Q|) when normalised (modes 1,2), else 1 */
    int32_t t_off;      /* (int)round(time_offset)                           */
    int32_t status;     /* 0 | -ERANGE (needs scratch) | -EINVAL (odd count) */
    uint16_t sw0, sw1;  /* argmax bins of the two sync symbols               */
    uint8_t sync_word;  /* ((sw0>>(sf-4))&15)<<4 | ((sw1>>(sf-4))&15)        */
    uint8_t crc_ok;     /* lora_phy::decode's metrics.crc_ok (LPHY_F_DECODE) */
    uint8_t normalised; /* 1 when max(|I|,|Q|) > 1 forced the rescale        */
    uint8_t have_sync;  /* frame had >= 2 symbols                            */
} lphy_frame_meta;

enum lphy_mode {
    LPHY_MODE_DEMODULATE = 0,              /* lora_phy::demodulate (raw IQ)  */
    LPHY_MODE_LORA_DEMODULATE = 1,         /* lora_demodulate (dechirped IQ) */
    LPHY_MODE_DECHIRP_LORA_DEMODULATE = 2  /* raw IQ, dechirp fused, then 1  */
};

enum lphy_flags {
    LPHY_F_DECODE = 1u,      /* also Hamming-decode + CRC each frame        */
    LPHY_F_NO_SCRATCH = 2u,  /* modes 1/2: behave as lora_demodulate with no
                                scratch buffer (-ERANGE when rescale needed) */
    /* Stage selection (profiling / overlap): when any of these bits is set
     * only the selected stages are launched; none set = all three.  With
     * PROLOGUE | SYMBOLS both set, the fused kernel (when it applies) runs
     * both in one launch. */
    LPHY_F_STAGE_PROLOGUE = 4u,  /* per-frame max-abs + offset estimate   */
    LPHY_F_STAGE_SYMBOLS = 8u,   /* per-symbol rotate + FFT + argmax      */
    LPHY_F_STAGE_FINAL = 16u,    /* per-frame sync word, decode, CRC      */
    LPHY_F_UNFUSED = 32u         /* separate prologue / symbol launches
                                    instead of the fused single launch
                                    (same results; the shapes the fused
                                    kernels do not take run them anyway) */
    /* Bits 64..1024 are comparison / test paths of the test-only build
     * (lib/test/, csrc/lphy_testing.h); this library rejects them with
     * -EINVAL. */
};

enum lphy_window { LPHY_WINDOW_NONE = 0, LPHY_WINDOW_HANN = 1 };

/* Create a context for one (sf, bandwidth, osr, window) configuration on
 * HIP device `device`.  Precomputes the KISS twiddles, the down-chirp and
 * the window on the host with the same libm calls as the reference, and
 * uploads them.  sf in [1,12]; bw_hz in {125000,250000,500000}.
 * Returns 0, -EINVAL (bad arguments) or -ENODEV / -ENOMEM. */
int lphy_hip_ctx_create(lphy_hip_ctx** out, int device, unsigned sf,
                        unsigned bw_hz, unsigned osr, int window);
void lphy_hip_ctx_destroy(lphy_hip_ctx* ctx);

/* A context of its own over `base`'s constant tables (shared, read-only;
 * they are freed with the last context holding them), with `osr` (0: the
 * base's).  Each context has its own stream and staging for the *_host
 * entry points, so contexts made this way - one per workspace or thread, as
 * the C++ shim does (lora_demod_init, init) - never wait for each other.
 * Returns 0, -EINVAL, -ENOMEM or -EIO. */
int lphy_hip_ctx_share(lphy_hip_ctx** out, const lphy_hip_ctx* base, unsigned osr);

/* Size the context's host-call staging for calls of up to `frames` frames
 * of `frame_samples` samples (the *_host entry points below), so that those
 * calls allocate nothing: the reference allocates nothing after init
 * (API_SPEC.md:9-14; lora_demod_init's max_samples, LoRaDemod.cpp:11-33).
 * The size covers every *_host form at that shape: frames of frame_samples
 * each, or one buffer of frames * frame_samples samples (the ragged receive
 * and transmit forms: `frames` frames of up to frame_samples each).
 * A larger call later grows the staging once.  Returns 0 or -ENOMEM/-EIO. */
int lphy_hip_ctx_reserve(lphy_hip_ctx* ctx, size_t frames, size_t frame_samples);

/* Smallest batch (frames per lphy_hip_demod_batch call) that takes the
 * fused single-launch kernels on this context; smaller batches take the
 * separate symbol-parallel launches, which finish a few frames sooner.
 * `frames` < 0 restores the measured per-SF crossover (the default); 0 sends
 * every batch whose shape fits to the fused kernels (throughput callers, the
 * test suite).  Results are identical either way.  Returns 0 or -EINVAL. */
int lphy_hip_ctx_set_fused_min_frames(lphy_hip_ctx* ctx, long frames);

/* Symbols written per frame for a frame of `frame_samples` samples. */
size_t lphy_hip_syms_per_frame(const lphy_hip_ctx* ctx, size_t frame_samples,
                               int mode);

/* Demodulate `frames` frames of device-resident IQ (asynchronous on
 * `stream`).  d_bytes may be NULL unless LPHY_F_DECODE.  d_meta is
 * required.  Returns 0 or -EINVAL/-ERANGE for shape errors (the per-frame
 * conditions the reference reports through its return value are in
 * lphy_frame_meta.status).
 * Limits: frames * (frame_samples / (N*osr)) < 2^32 symbols per call and
 * frame_samples < 2^31 (32-bit symbol bookkeeping in the kernels): larger
 * batches give -ERANGE; split them across calls.
 * Launch choice: the fused launches (k_wave at SF 7-12 for osr 1, no
 * window, modes 1/2 with the speculative normalisation or mode 0, and below
 * SF 9 at least 4096/N symbols per frame - SF 7-10 with units spanning
 * frames; k_frames otherwise up to SF 10, e.g. windowed or short frames)
 * for batches of at
 * least a per-SF crossover (256 frames at SF <= 7 ... 384 at SF 10-12,
 * DESIGN.md 4.7; lphy_hip_ctx_set_fused_min_frames overrides it per
 * context), the separate symbol-parallel launches below it (a packet at a
 * time).  The choice depends on the arguments and that setting only (no
 * environment variables).
 * Memory: the fused launches allocate nothing.  The SF 11-12 separate launches
 * (LPHY_F_UNFUSED, small batches, osr > 1, a window) take per-call speculation records
 * (16 B per frame) from the stream-ordered pool on `stream`, released in
 * stream order, so calls on different streams of one context never share
 * them; the *_host forms lend them from the reserved staging instead. */
int lphy_hip_demod_batch(lphy_hip_ctx* ctx, const float* d_iq, size_t frames,
                         size_t frame_samples, uint16_t* d_syms,
                         uint8_t* d_bytes, lphy_frame_meta* d_meta, int mode,
                         unsigned flags, void* stream);

/* ------------------------------------------------------------------------
 * Ragged batches: frames of different lengths in one call.
 *
 * Frame f is described by record f of `frames + 1` descriptors; record
 * [frames] holds the totals.  Frame f gets exactly what the uniform call
 * (and the reference) returns for that frame alone on `samples` samples:
 * its symbols at d_syms + sym_offset, its lphy_frame_meta at d_meta + f and,
 * with LPHY_F_DECODE, its bytes at d_bytes + sym_offset/2.
 *
 * lphy_hip_ragged_layout fills the descriptors for frames packed back to
 * back (outputs packed by lphy_hip_syms_per_frame, every sym_offset even).
 * Callers may write their own, with gaps between frames in the IQ or in the
 * outputs and frames in any address order, as long as
 *   - no two frames overlap in the outputs (slots between them are left
 *     untouched),
 *   - unit_offset is the exclusive prefix sum of samples / N in record
 *     order, starting at 0, with the total in record [frames], and
 *   - sym_offset is even when LPHY_F_DECODE is set.
 *
 * Per-frame status: what the uniform call reports through its return value
 * for a frame length becomes meta[f].status, and the frame writes nothing
 * else: mode 0 with samples % N != 0 gives -EINVAL, mode 0 with fewer than
 * two symbols -ERANGE, mode 2 with samples % N != 0 -EINVAL, and a frame of
 * samples >= 2^31 -ERANGE.  -ERANGE under LPHY_F_NO_SCRATCH and -EINVAL for
 * an odd decode count are reported as by lphy_hip_demod_batch.
 *
 * Scope: SF 7-12, osr 1, window none or Hann, modes 0-2, flags
 * LPHY_F_DECODE and LPHY_F_NO_SCRATCH.  Anything else - the stage flags,
 * LPHY_F_UNFUSED, the test build's flags, an osr > 1 context, SF < 7 -
 * returns -ENOTSUP.  Limits (-ERANGE from lphy_hip_ragged_layout and the
 * host form): any samples >= 2^31, or 2^32 or more whole symbols in the call.
 * Launches: three symbol-parallel kernels (per-frame prologue, per-symbol
 * rotate + FFT + argmax with the reference's per-sample rotation, per-frame
 * finalisation); the call allocates nothing on the device.
 * --------------------------------------------------------------------- */
typedef struct lphy_ragged_desc {   /* 32 bytes; frames + 1 records */
    uint64_t iq_offset;    /* first sample of frame f, in samples from d_iq   */
    uint64_t samples;      /* the frame's sample_count (any value, 0 allowed) */
    uint64_t sym_offset;   /* frame's first output symbol, from d_syms        */
    uint64_t unit_offset;  /* exclusive prefix of whole symbols per frame     */
} lphy_ragged_desc;        /* record [frames] holds the totals (samples = 0)  */

/* Host-only, no device work.  From h_samples[frames] fills h_desc[frames+1].
 * Returns 0, -EINVAL (null pointer, bad mode) or -ERANGE (the limits above). */
int lphy_hip_ragged_layout(const lphy_hip_ctx* ctx, const uint64_t* h_samples,
                           size_t frames, int mode, lphy_ragged_desc* h_desc);

/* Demodulate `frames` frames described by d_desc (device memory, frames + 1
 * records), asynchronously on `stream`.  d_bytes may be NULL unless
 * LPHY_F_DECODE.  frames == 0 returns 0. */
int lphy_hip_demod_ragged(lphy_hip_ctx* ctx, const float* d_iq,
                          const lphy_ragged_desc* d_desc, size_t frames,
                          uint16_t* d_syms, uint8_t* d_bytes,
                          lphy_frame_meta* d_meta, int mode, unsigned flags,
                          void* stream);

/* The same on host buffers, through the context's stream and staging like
 * lphy_hip_demod_host.  h_iq, h_syms and h_bytes span the descriptors' extent
 * (the largest iq_offset + samples, and sym_offset plus the frame's symbols);
 * output slots no frame owns keep the caller's values. */
int lphy_hip_demod_ragged_host(lphy_hip_ctx* ctx, const float* h_iq,
                               const lphy_ragged_desc* h_desc, size_t frames,
                               uint16_t* h_syms, uint8_t* h_bytes,
                               lphy_frame_meta* h_meta, int mode, unsigned flags);

/* ------------------------------------------------------------------------
 * The detector on a batch of windows: LoRaDetector<float>::detect
 * (include/lora_phy/LoRaDetector.hpp:39-74), all four outputs per window.
 *
 * Window w feeds the detector N = 2^sf samples, x_i = iq[first + w*hop +
 * i*step] for i = 0..N-1, prepared in this order:
 *   1. with LPHY_DET_DECHIRP, times the context's down-chirp, x_i * down[i]
 *      (the reference's complex product; the test-side dechirp of
 *      tests/e2e_chain_test.cpp:80-93 on the window),
 *   2. on a context created with LPHY_WINDOW_HANN, times win[i]
 *      (LoRaDemod.cpp:96-97).
 * No normalisation, no rotation.  hop < N makes the windows overlap (a
 * sliding detector); step is the decimation: hop = 1, step = osr, windows =
 * osr are the reference's osr phases of one symbol.  A frame's per-symbol SNR
 * is power - power_avg with first = the frame's start, hop = N, step = 1
 * (for many frames of different lengths: lphy_hip_detect_ragged, below).
 *
 * Every record holds what detect() returns for that input, bit for bit
 * (where the reference gives a NaN, a NaN): an all-zero window gives index
 * 0, power = power_avg = -inf, findex = 0; ties go to the lowest bin.
 *
 * Returns -EINVAL for a null ctx / iq / out, hop == 0, step == 0 or an
 * unknown flag bit; -ENOTSUP for SF < 7; then 0 for windows == 0; -ERANGE
 * for windows >= 2^32 or a last index first + (windows-1)*hop + (N-1)*step
 * >= total_samples.  The device form is asynchronous on `stream`, allocates
 * nothing and writes d_out[0 .. windows) only; the host form goes through the
 * context's stream and staging like lphy_hip_demod_host.
 *
 * power_avg needs the reference's double-precision sum in bin order.  The
 * kernel certifies its value from a parallel sum where it can and walks the
 * bins in order where it cannot (a clean tone: total - maxValue cancels);
 * lphy_hip_detect_serial_count reads (and with `reset` clears) the number of
 * windows that took the walk on this context.  It synchronises the device.
 * --------------------------------------------------------------------- */
typedef struct lphy_detect_rec {   /* 16 bytes, one per window */
    float    power;      /* detect()'s power                     */
    float    power_avg;  /* detect()'s powerAvg                  */
    float    findex;     /* detect()'s fIndex                    */
    uint16_t index;      /* detect()'s return value (peak bin)   */
    uint16_t reserved;   /* 0                                    */
} lphy_detect_rec;

enum lphy_detect_flags { LPHY_DET_DECHIRP = 1u };

int lphy_hip_detect_batch(lphy_hip_ctx* ctx, const float* d_iq, size_t total_samples,
                          size_t first, size_t hop, size_t step, size_t windows,
                          lphy_detect_rec* d_out, unsigned flags, void* stream);
int lphy_hip_detect_host(lphy_hip_ctx* ctx, const float* h_iq, size_t total_samples,
                         size_t first, size_t hop, size_t step, size_t windows,
                         lphy_detect_rec* h_out, unsigned flags);
int lphy_hip_detect_serial_count(lphy_hip_ctx* ctx, unsigned long long* out, int reset);

/* ------------------------------------------------------------------------
 * The detector on every whole symbol of every frame of a ragged table, in one
 * launch: the table of lphy_hip_demod_ragged, lphy_hip_estimate_ragged and
 * lphy_hip_compensate_ragged.  One lphy_detect_rec per symbol, so a frame's
 * per-symbol SNR (power - power_avg) comes with its demodulation, whatever
 * the frames' lengths.
 *
 * Frame f, with d = d_desc[f], step = N * osr and n = d.samples / step whole
 * symbols:
 *   - symbol s < n feeds the detector x_i = iq[d.iq_offset + s*step + phase +
 *     i*osr], i = 0..N-1: `phase` < osr picks the decimation phase (0 is what
 *     demodulate reads, phy.cpp:225).  The input is prepared as
 *     lphy_hip_detect_batch prepares a window: with LPHY_DET_DECHIRP times
 *     down[i], on a Hann context times win[i], no normalisation, no rotation.
 *   - its record goes to d_out[d.unit_offset + s], bit for bit what detect()
 *     returns for that input: what lphy_hip_detect_batch(first = d.iq_offset +
 *     phase, hop = step, step = osr, windows = n) gives for the frame alone.
 *     d_out holds d_desc[frames].unit_offset records (read on the device).
 *   - the partial symbol at the frame's end is not read, nor anything outside
 *     the frame, nor sym_offset.
 *   - n == 0: the frame writes nothing.  d.samples >= 2^31: the frame writes
 *     nothing and nothing of it is read (lphy_hip_demod_ragged's rule).
 *   - a table whose unit_offset prefix is wrong cannot lead outside a frame
 *     or past d_desc[frames].unit_offset records; which records it fills is
 *     then unspecified.  Frames may lie in any address order and may overlap
 *     each other in the IQ: the call only reads it.
 *
 * Scope: SF 7-12, every osr the context accepts, window none or Hann.
 * Returns -EINVAL for a null ctx, then 0 for frames == 0; -EINVAL for a null
 * d_iq, d_desc or d_out, an unknown flag bit or phase >= osr; -ERANGE for
 * frames >= 2^31; -ENOTSUP for SF < 7.  All of it before any device call.
 *
 * The device form is asynchronous on `stream`: one launch, no device
 * allocation, no host read of the table.  Windows that take the in-order
 * power_avg walk count in lphy_hip_detect_serial_count, as for
 * lphy_hip_detect_batch.
 *
 * The host form goes through the context's stream and staging like
 * lphy_hip_demod_host.  It checks the table before any device call: -ERANGE
 * for any samples >= 2^31, an iq_offset above 2^48 or 2^32 or more whole
 * symbols, -EINVAL for a unit_offset that is not the exclusive prefix of
 * samples / step (record [frames] included), as lphy_hip_demod_ragged_host.
 * It uploads h_iq over the descriptors' extent (the largest iq_offset +
 * samples) and the frames + 1 records, and downloads h_desc[frames]
 * .unit_offset records into h_out: every one has exactly one owner.
 * --------------------------------------------------------------------- */
int lphy_hip_detect_ragged(lphy_hip_ctx* ctx, const float* d_iq,
                           const lphy_ragged_desc* d_desc, size_t frames,
                           unsigned phase, lphy_detect_rec* d_out,
                           unsigned flags, void* stream);
int lphy_hip_detect_ragged_host(lphy_hip_ctx* ctx, const float* h_iq,
                                const lphy_ragged_desc* h_desc, size_t frames,
                                unsigned phase, lphy_detect_rec* h_out,
                                unsigned flags);

/* ------------------------------------------------------------------------
 * Frame search: the ragged table of the frames found in a capture, from the
 * detector records of its windows.  No reference function: the reference's
 * waveform has no preamble (two sync symbols, then data, LoRaMod.cpp:8-43) and
 * it has no search.  The result is a pure function of the records, which
 * lphy_hip_detect_batch pins to the reference's detector bit for bit, so the
 * receive chain starts at the capture with no host read between the calls:
 *   lphy_hip_channelize -> lphy_hip_detect_batch (hop <= N) -> lphy_hip_find_frames ->
 *   lphy_hip_estimate_ragged -> lphy_hip_compensate_ragged ->
 *   lphy_hip_demod_ragged -> lphy_hip_lorawan_parse_ragged -> ..._crypt_rx_ragged
 *
 * With S = lphy_hip_symbol_samples(ctx) and p = *params:
 *   1. Window w is active iff (rec[w].power - rec[w].power_avg) >=
 *      p.threshold_db, the subtraction and the compare in float32.  A NaN
 *      difference is inactive: the all-zero window (both fields -inf) is.
 *   2. Two consecutive active windows a < a' belong to one burst iff a' - a - 1
 *      <= p.max_gap.  A burst is (a, b), its first and last active window;
 *      inactive windows before the first and after the last active one are
 *      never bridged.
 *   3. start = p.first + p.lead + a * p.hop.  extent = 0 when start >=
 *      p.total_samples, else min((b - a + 1) * p.hop, p.total_samples - start).
 *      total = extent / S.  The frame is total * S samples at start: whole
 *      symbols, never overlapping another frame, never leaving the capture.
 *   4. Drops, in this order: total < p.min_symbols counts in dropped_short;
 *      total * S >= 2^31 counts in dropped_long.
 *   5. The kept bursts, in order of a, are frames 0, 1, ...  Those past
 *      max_frames count in overflow and are not written.
 *   6. Record k of a frame is {iq_offset = start, samples = total * S,
 *      sym_offset, unit_offset}: sym_offset the exclusive prefix of
 *      (lphy_hip_syms_per_frame(total * S, mode) + 1) & ~1, unit_offset the
 *      exclusive prefix of total, exactly as lphy_hip_ragged_layout packs them.
 *   7. Records frames .. max_frames, the last included, hold the totals of the
 *      frames written: {end of the last frame (0 with none), 0, the symbol
 *      total, the unit total}.  The table is therefore valid for every ragged
 *      call with frames = max_frames: the padding frames have 0 samples, which
 *      all of those calls define, record [max_frames] is the totals record, and
 *      no host read of d_info is needed to go on.
 *   8. The call writes all max_frames + 1 records and d_info, and nothing else
 *      outside d_work.  The result does not depend on what d_work held and is
 *      the same on every run (no atomic decides an order).
 *
 * d_work: lphy_hip_find_frames_workspace(windows) bytes of device memory,
 * 16-byte aligned (never 0 bytes).  The device form is asynchronous on
 * `stream`: six launches whatever the arguments, no device allocation, no host
 * read of anything on the device, and no workgroup waits on another (the
 * order between the passes is the order of the launches).  Every SF is in
 * scope: there is no transform.  The host form goes through the context's
 * stream and staging like lphy_hip_detect_host and takes its workspace from
 * that staging.
 *
 * Returns, all before any device call and in this order: -EINVAL for a null
 * ctx, params, d_desc or d_info; d_rec null with windows > 0; d_work null or
 * not 16-byte aligned; hop == 0, min_symbols == 0 or max_frames == 0; a NaN
 * threshold; reserved != 0; a mode outside 0..2.  -ERANGE for windows >= 2^32;
 * max_frames > 2^31 - 1; first + lead + windows * hop > 2^48; windows * hop / S
 * >= 2^32 (each computed without overflow).  windows == 0 is not an early
 * return: it writes the all-padding table and a zero d_info.
 * --------------------------------------------------------------------- */
typedef struct lphy_find_params {      /* host memory, read on the host */
    uint64_t first;          /* first sample of window 0 (lphy_hip_detect_batch's first)  */
    uint64_t hop;            /* samples between window starts (its hop), >= 1             */
    uint64_t lead;           /* samples added to every frame's start (the caller's        */
                             /* calibration for overlapping windows; 0 when hop = symbol) */
    uint64_t total_samples;  /* the capture's length: no frame reaches past it            */
    float    threshold_db;   /* window active iff power - power_avg >= threshold_db       */
    uint32_t max_gap;        /* up to this many inactive windows inside a burst are bridged */
    uint32_t min_symbols;    /* bursts of fewer whole symbols are dropped, >= 1           */
    uint32_t reserved;       /* 0 */
} lphy_find_params;

typedef struct lphy_find_info {        /* 32 bytes, device memory, written by the call */
    uint32_t frames;         /* records 0 .. frames-1 of the table are real frames */
    uint32_t bursts;         /* bursts found before any was dropped                */
    uint32_t dropped_short, dropped_long, overflow;
    uint32_t active;         /* active windows */
    uint32_t reserved[2];    /* 0 */
} lphy_find_info;

size_t lphy_hip_find_frames_workspace(size_t windows);   /* bytes, host-only */
int lphy_hip_find_frames(lphy_hip_ctx* ctx, const lphy_detect_rec* d_rec, size_t windows,
                         const lphy_find_params* params, int mode, size_t max_frames,
                         lphy_ragged_desc* d_desc /* max_frames + 1 records */,
                         lphy_find_info* d_info, void* d_work, void* stream);
int lphy_hip_find_frames_host(lphy_hip_ctx* ctx, const lphy_detect_rec* h_rec, size_t windows,
                              const lphy_find_params* params, int mode, size_t max_frames,
                              lphy_ragged_desc* h_desc, lphy_find_info* h_info);

/* ------------------------------------------------------------------------
 * Channeliser: `channels` narrow-band streams from one wideband capture, a
 * mixer, a low-pass FIR and a decimator per channel.  No reference function:
 * the reference, like every call above, starts from a capture that is one LoRa
 * channel at the context's sample rate.  It stands in front of the chain,
 *   lphy_hip_channelize -> lphy_hip_detect_batch -> lphy_hip_find_frames -> ...
 * on the device and in stream order.  Samples are interleaved float32 I/Q.
 *
 * With T = taps, D = decim, R = rot_period of *plan, for channel c < channels
 * and output m < outputs:
 *     ar = ai = +0.0f
 *     for k = 0 .. T-1, in this order:
 *         x = in[first + m*D + k]          g = taps[c*T + k]
 *         pr = x.re*g.re - x.im*g.im       pi = x.re*g.im + x.im*g.re
 *         ar = ar + pr                     ai = ai + pi
 *     r = rot[c*R + (rot_first + m) % R]
 *     out[c*out_stride + m] = (ar*r.re - ai*r.im,  ar*r.im + ai*r.re)
 * Every product, sum and difference is one IEEE float32 operation rounded on
 * its own: no FMA, no reassociation, subnormals kept.  The device computes no
 * trigonometry: taps (channels x T) and rot (channels x R) are the caller's
 * complex float32 tables in device memory, so the result is a pure function of
 * its inputs, the same bits on every run.  In signal terms taps[c] is a
 * low-pass prototype times channel c's mixer over one filter length and rot[c]
 * the mixer's phase at the decimated rate, periodic whenever the centre is a
 * rational number of cycles per sample.  `first` lets the blocks of a long
 * capture overlap by T - D samples and `rot_first` carries the rotation's
 * phase from one block to the next.
 *
 * Limits: channels 1..64, taps 1..4096, decim 1..65536 (decim > taps is
 * legal: samples are skipped), rot_period 1..65536, outputs < 2^32,
 * out_stride >= outputs, in_samples <= 2^48, first + (outputs-1)*decim + taps
 * <= in_samples (asked with outputs > 0), channels * out_stride <= 2^48.
 *
 * Returns, all before any device call and in this order: -EINVAL for a null
 * ctx, plan, d_taps or d_rot; d_in or d_out null with outputs > 0; d_in,
 * d_taps, d_rot or d_out not 8-byte aligned; reserved != 0; channels, taps,
 * decim or rot_period == 0.  -ERANGE, in this order, for channels > 64; taps >
 * 4096; decim > 65536; rot_period > 65536; outputs >= 2^32; out_stride <
 * outputs; in_samples > 2^48; a tap outside the capture; channels * out_stride
 * > 2^48 (each computed without overflow).  outputs == 0 then returns 0 and
 * launches nothing.
 *
 * The device form is asynchronous on `stream`: one launch, no device
 * allocation, nothing read back, no workgroup waits on another and no atomic.
 * It writes out[c*out_stride + m] for m < outputs alone: slots outputs ..
 * out_stride-1 of every channel keep the caller's values.  d_in and d_out must
 * not overlap; the call does not check it.  Any SF: ctx supplies the device
 * and, for the host form, the stream and the staging (the host form moves the
 * samples first .. first + (outputs-1)*decim + taps alone, and all of h_out
 * both ways).
 * lphy_hip_channelize_outputs: the largest `outputs` for which every tap lies
 * inside the capture, 0 when there is none (or taps or decim is 0).
 * --------------------------------------------------------------------- */
typedef struct lphy_chan_plan {   /* host memory, read on the host */
    uint64_t first;          /* input sample of output 0's first tap                    */
    uint64_t in_samples;     /* the capture's length in samples                         */
    uint64_t outputs;        /* outputs per channel                                     */
    uint64_t out_stride;     /* samples between the channels' streams in out            */
    uint64_t rot_first;      /* rotation phase of output 0: rot[c*R + rot_first % R]    */
    uint32_t channels, taps, decim, rot_period;
    uint32_t reserved[2];    /* 0 */
} lphy_chan_plan;

uint64_t lphy_hip_channelize_outputs(uint64_t in_samples, uint64_t first,
                                     uint32_t taps, uint32_t decim);   /* host-only */
int lphy_hip_channelize(lphy_hip_ctx* ctx, const float* d_in, const lphy_chan_plan* plan,
                        const float* d_taps, const float* d_rot, float* d_out, void* stream);
int lphy_hip_channelize_host(lphy_hip_ctx* ctx, const float* h_in, const lphy_chan_plan* plan,
                             const float* h_taps, const float* h_rot, float* h_out);

/* ------------------------------------------------------------------------
 * The channeliser on a capture as the radio wrote it: interleaved I/Q in one
 * of the formats below, so that the largest object of the chain crosses the
 * host link and lies in device memory at 4 or 2 bytes a sample instead of 8.
 *
 * lphy_hip_channelize_raw gives, byte for byte, what lphy_hip_channelize gives
 * with the same plan and tables on the float32 capture x' of the same length:
 *     LPHY_FMT_SC16, LPHY_FMT_SC8:  x'.re = (float)I           x'.im = (float)Q
 *     LPHY_FMT_CU8:                 x'.re = (float)I - 127.5f  x'.im = (float)Q - 127.5f
 *     LPHY_FMT_CF32:                x' = the capture: the call is lphy_hip_channelize
 *                                   itself, same alignment rule, same bytes
 * Every one of these conversions is exact in float32, -32768, -128 and the
 * half-integers of CU8 included, so the result stays a pure function of the
 * inputs.  There is no scale argument: the caller folds 1/32768 (or 1/128,
 * 1/127.5) into the taps.  The call is a plain converter too: with channels =
 * taps = decim = rot_period = 1, taps = (g, 0) and rot = (1, 0), output m is
 * exactly (g * x'.re, g * x'.im) of sample first + m, each one float32
 * product (every other operation of the definition adds or subtracts a zero or
 * multiplies by one; a power-of-two g does not round at all), so a
 * single-channel capture at the channel's own rate enters the chain through
 * this call as well.
 *
 * *plan is used as it is, all its counts in samples, and the limits are those
 * of lphy_hip_channelize.  Returns, all before any device call, in
 * lphy_hip_channelize's order with two changes: directly after the
 * null-pointer rows (ctx, plan, d_taps, d_rot; d_in or d_out null with outputs
 * > 0) a format that is none of the four gives -EINVAL; and the alignment row
 * asks d_in for lphy_hip_sample_bytes(format) bytes (8, 4, 2, 2) and the other
 * three pointers for 8.  Everything after that row is unchanged: reserved, the
 * zero counts, the -ERANGE rows in their order; outputs == 0 then returns 0
 * and launches nothing.
 *
 * The device form is asynchronous on `stream`: one launch, no device
 * allocation, nothing read back, no workgroup waits on another and no atomic.
 * It writes out[c*out_stride + m] for m < outputs alone and reads no byte
 * outside the samples its outputs name.  The host form goes through the
 * context's stream and staging like lphy_hip_channelize_host: it moves the
 * samples first .. first + (outputs-1)*decim + taps alone, at
 * lphy_hip_sample_bytes(format) each (1/2 or 1/4 of the float32 form's
 * upload), and all of h_out both ways.
 *
 * Not provided: the transmit mirror (lphy_hip_synthesize to integer samples
 * needs a rounding and saturation rule of its own), lphy_hip_demod_stream on
 * integer files, big-endian or non-interleaved captures, 12-bit packed formats.
 * --------------------------------------------------------------------- */
enum lphy_sample_format {
    LPHY_FMT_CF32 = 0,  /* float32 I, float32 Q: what lphy_hip_channelize takes      */
    LPHY_FMT_SC16 = 1,  /* int16 I, int16 Q, little endian                           */
    LPHY_FMT_SC8  = 2,  /* int8 I, int8 Q                                            */
    LPHY_FMT_CU8  = 3   /* uint8 I, uint8 Q, offset binary: value = byte - 127.5     */
};
size_t lphy_hip_sample_bytes(int format);   /* 8, 4, 2, 2; 0 for anything else; host-only */

int lphy_hip_channelize_raw(lphy_hip_ctx* ctx, const void* d_in, int format,
                            const lphy_chan_plan* plan, const float* d_taps,
                            const float* d_rot, float* d_out, void* stream);
int lphy_hip_channelize_raw_host(lphy_hip_ctx* ctx, const void* h_in, int format,
                                 const lphy_chan_plan* plan, const float* h_taps,
                                 const float* h_rot, float* h_out);

/* ------------------------------------------------------------------------
 * Synthesiser: one wideband stream from `channels` narrow-band streams, the
 * channeliser's mirror: per channel a rotation, a polyphase interpolating FIR
 * and a mixer, then the sum over the channels.  No reference function.  It
 * stands behind the transmit chain,
 *   lphy_hip_lorawan_crypt_tx_ragged -> lphy_hip_lorawan_build_ragged ->
 *   lphy_hip_tx_ragged (one stream per channel) -> lphy_hip_synthesize
 * on the device and in stream order.  Samples are interleaved float32 I/Q.
 *
 * With T = taps, U = interp, R = rot_period of *plan, for output n < outputs
 * let w = first + n, q = w / U and p = w % U (64-bit integer division and
 * remainder):
 *     yr = yi = +0.0f
 *     for c = 0 .. channels-1, in this order:
 *         ar = ai = +0.0f
 *         for i = 0, 1, 2, ... while k = i*U + p < T, in this order:
 *             j = q - i                                  (signed)
 *             if 0 <= j < in_samples:
 *                 x = in[c*in_stride + j]    r = rot[c*R + (rot_first + j) % R]
 *                 xr = x.re*r.re - x.im*r.im             xi = x.re*r.im + x.im*r.re
 *             else:
 *                 xr = xi = +0.0f            (the operand is +0; the products below are still formed)
 *             g  = taps[c*T + k]
 *             pr = xr*g.re - xi*g.im                     pi = xr*g.im + xi*g.re
 *             ar = ar + pr                               ai = ai + pi
 *         yr = yr + ar                                   yi = yi + ai
 *     out[n] = (yr, yi)
 * Every product, sum and difference is one IEEE float32 operation rounded on
 * its own: no FMA, no reassociation, subnormals kept (the channeliser's rule).
 * A phase p >= T has no taps: its output is (+0, +0).  The device computes no
 * trigonometry: taps (channels x T) and rot (channels x R) are the caller's
 * complex float32 tables in device memory.  In signal terms taps[c] is U times
 * a low-pass prototype times channel c's mixer exp(+2 pi i f_c k) over one
 * filter length and rot[c][j] = exp(+2 pi i f_c U j) the mixer's phase at the
 * narrow rate: the conjugates of the channeliser's tables for decim = U, the
 * taps scaled by U.  `first` and `rot_first` let a long transmission go out in
 * blocks: advance d_in by J0 narrow samples, pass first = w0 - J0*U and
 * rot_first = J0, and the block's bytes are those one call over the whole
 * transmission gives.
 *
 * Limits: channels 1..64, taps 1..4096, interp 1..65536, rot_period 1..65536,
 * outputs < 2^32, in_stride >= in_samples, in_samples <= 2^48, channels *
 * in_stride <= 2^48, first + outputs <= 2^48.
 *
 * Returns, all before any device call and in this order: -EINVAL for a null
 * ctx, plan, d_taps or d_rot; d_out null with outputs > 0; d_in null with
 * outputs > 0 and in_samples > 0; d_in, d_taps, d_rot or d_out (those given)
 * not 8-byte aligned; reserved != 0; channels, taps, interp or rot_period ==
 * 0.  -ERANGE, in this order, for channels > 64; taps > 4096; interp > 65536;
 * rot_period > 65536; outputs >= 2^32; in_stride < in_samples; in_samples >
 * 2^48; channels * in_stride > 2^48; first + outputs > 2^48 (each computed
 * without overflow).  outputs == 0 then returns 0 and launches nothing.
 *
 * The device form is asynchronous on `stream`: one launch, no device
 * allocation, nothing read back, no workgroup waits on another and no atomic.
 * It writes out[0 .. outputs) alone.  d_in and d_out must not overlap; the
 * call does not check it.  Any SF: ctx supplies the device and, for the host
 * form, the stream and the staging (the host form moves h_in from channel 0's
 * first sample to the last channel's sample in_samples - 1, strides included,
 * and `outputs` samples back).
 * lphy_hip_synthesize_outputs: the outputs up to the last one an input sample
 * reaches, (in_samples - 1) * interp + taps - first when in_samples >= 1 and
 * that is positive, else 0 (also when taps or interp is 0); past the limits
 * above the product saturates at 2^64 - 1.  A larger `outputs` is legal: the
 * tail is (+0, +0).
 * --------------------------------------------------------------------- */
typedef struct lphy_synth_plan {  /* host memory, read on the host */
    uint64_t first;          /* wideband sample index of output 0                       */
    uint64_t in_samples;     /* narrow samples per channel                              */
    uint64_t in_stride;      /* samples between the channels' streams in in             */
    uint64_t outputs;        /* wideband samples to write                               */
    uint64_t rot_first;      /* rotation phase of narrow sample 0: rot[c*R + rot_first % R] */
    uint32_t channels, taps, interp, rot_period;
    uint32_t reserved[2];    /* 0 */
} lphy_synth_plan;

uint64_t lphy_hip_synthesize_outputs(uint64_t in_samples, uint64_t first,
                                     uint32_t taps, uint32_t interp);   /* host-only */
int lphy_hip_synthesize(lphy_hip_ctx* ctx, const float* d_in, const lphy_synth_plan* plan,
                        const float* d_taps, const float* d_rot, float* d_out, void* stream);
int lphy_hip_synthesize_host(lphy_hip_ctx* ctx, const float* h_in, const lphy_synth_plan* plan,
                             const float* h_taps, const float* h_rot, float* h_out);

/* Hamming(8,4)sx decode + sx1272 CRC of device symbols: frame f holds
 * syms_per_frame symbols at d_syms + f*syms_per_frame and yields
 * syms_per_frame/2 bytes; meta[f].crc_ok / .status updated.  An odd
 * syms_per_frame gives -EINVAL (LoRaDecoder.cpp:10). */
int lphy_hip_decode_batch(lphy_hip_ctx* ctx, const uint16_t* d_syms,
                          size_t frames, size_t syms_per_frame,
                          uint8_t* d_bytes, lphy_frame_meta* d_meta,
                          void* stream);

/* estimate_offsets (phy.cpp:81-148) over the first `est_samples` samples of
 * each frame (its est_samples / (N*osr) whole symbols; nothing after them is
 * read): writes meta[f].cfo / .time_offset / .t_off / .rate, with
 * t_off = (int)round(time_offset) and rate = -2*pi*cfo / N.  The call
 * rewrites the whole record, not only those four fields: status = 0,
 * scale = 1, have_sync = (frame_samples / (N*osr) >= 2), and sw0, sw1,
 * sync_word, crc_ok and normalised = 0, whatever the record held before.
 * With frames == 0, or est_samples shorter than one symbol, it returns 0 and
 * writes nothing (phy.cpp:87,91).  est_samples > frame_samples (frames >= 1)
 * gives -EINVAL and launches nothing: the estimate would read the next
 * frame, and the last frame's past the end of d_iq. */
int lphy_hip_estimate_batch(lphy_hip_ctx* ctx, const float* d_iq,
                            size_t frames, size_t frame_samples,
                            size_t est_samples, lphy_frame_meta* d_meta,
                            void* stream);

/* ------------------------------------------------------------------------
 * estimate_offsets (phy.cpp:81-148) for every frame of a ragged table in one
 * launch: the table of lphy_hip_demod_ragged, lphy_hip_compensate_ragged and
 * the ragged transmit.  What it leaves in d_meta[f].cfo / .time_offset feeds
 * lphy_hip_compensate_ragged on the same stream, so estimate -> compensate ->
 * demodulate runs device-resident for frames of different lengths.
 *
 * Frame f, with d = d_desc[f] and step = N * osr:
 *   - its estimate extent is e = min(d.samples, est_samples) samples;
 *     est_samples == 0 means the whole frame, e = d.samples.  It has n = e /
 *     step whole symbols.  Nothing of the frame past n * step samples is read
 *     (neither the partial symbol at the end of the extent nor the rest of
 *     the frame), and nothing outside the frame.
 *   - n >= 1: d_meta[f] is rewritten as a whole, as lphy_hip_estimate_batch
 *     rewrites it: cfo and time_offset bit for bit what estimate_offsets gives
 *     for those n * step samples alone (a Hann context applies the window,
 *     phy.cpp:110-111), t_off = (int)round(time_offset), rate = -2*pi*cfo / N,
 *     status = 0, scale = 1, have_sync = (d.samples / step >= 2), and sw0, sw1,
 *     sync_word, crc_ok and normalised = 0.
 *   - n == 0: d_meta[f] is left untouched (phy.cpp:87,91).
 *   - d.samples >= 2^31: d_meta[f] is all zero but status = -ERANGE, and
 *     nothing of the frame is read (lphy_hip_demod_ragged's rule).
 *   - sym_offset and unit_offset are not read, nor is record [frames]
 *     (unit_offset counts the whole symbols of the whole frame, not the
 *     estimate's).  Frames may lie in any address order and may overlap each
 *     other in the IQ: the call only reads it.
 *
 * Scope: SF 7-12, every osr the context accepts, window none or Hann.
 * Returns -EINVAL for a null ctx, then 0 for frames == 0; -EINVAL for a null
 * d_iq, d_desc or d_meta; -ERANGE for frames >= 2^31; -ENOTSUP for SF < 7.
 * All of it before any device call.
 *
 * The device form is asynchronous on `stream`: one launch, no device
 * allocation, no host read of the table.  A workgroup takes a group of
 * consecutive frames (16 at SF 7 ... 1 at SF 11-12) and transforms their
 * estimate symbols T at a time (T = 32 at SF 7 ... 1 at SF 12), so the
 * parallelism within one frame is T symbols per workgroup, as in
 * lphy_hip_estimate_batch: the call is for many frames with short estimate
 * extents; a single very long buffer is lphy_hip_estimate_host's case.
 *
 * The host form goes through the context's stream and staging like
 * lphy_hip_demod_host.  It checks the table before any device call (-ERANGE
 * for any samples >= 2^31 or an iq_offset above 2^48; the prefix is not
 * required), uploads h_iq over the descriptors' extent (the largest iq_offset
 * + samples), the frames' records and h_meta, and downloads h_meta: the
 * records of n == 0 frames keep the caller's values.
 * --------------------------------------------------------------------- */
int lphy_hip_estimate_ragged(lphy_hip_ctx* ctx, const float* d_iq,
                             const lphy_ragged_desc* d_desc, size_t frames,
                             size_t est_samples, lphy_frame_meta* d_meta,
                             void* stream);
int lphy_hip_estimate_ragged_host(lphy_hip_ctx* ctx, const float* h_iq,
                                  const lphy_ragged_desc* h_desc, size_t frames,
                                  size_t est_samples, lphy_frame_meta* h_meta);

/* compensate_offsets (phy.cpp:150-180), in place on one device buffer. */
int lphy_hip_compensate(lphy_hip_ctx* ctx, float* d_iq, size_t count,
                        float cfo, float time_offset, void* stream);

/* ------------------------------------------------------------------------
 * compensate_offsets (phy.cpp:150-180) for every frame of a batch, each with
 * its own offsets read on the device from d_meta[f].cfo / .time_offset: what
 * lphy_hip_estimate_batch (or, for the ragged form, lphy_hip_estimate_ragged)
 * left there feeds it on the same stream, with no host copy between the two
 * calls.  Only those two fields are read (not
 * .rate, which is -2*pi*cfo/N without osr, nor .t_off: a caller may have
 * filled cfo and time_offset alone); d_meta is not written.
 *
 * Frame f of `count` samples gets, bit for bit, what the reference gives for
 * that frame alone, n = 0..count-1 within the frame:
 *   rate = -2.0f * PI * cfo / ((float)N * (float)osr), in float, on the device;
 *   off  = (int)std::round(time_offset) as x86-64 evaluates it (INT_MIN for a
 *          NaN or a value out of int's range);
 *   a shift applies iff off != INT_MIN and 0 < |off| < count; then, with
 *   src = n - off, out[n] = (0 <= src < count) ? in[src] * cis(rate * (float)src) : 0;
 *   without a shift out[n] = in[n] * cis(rate * (float)n).
 * cis is the reference's sincosf pair and the product its std::complex
 * product (with the Annex G recovery).  Frame indices are 64-bit.  Nothing
 * outside a frame's own samples is read or written.
 *
 * Aliasing: d_out == d_in is in place, disjoint buffers are out of place;
 * the uniform form returns -EINVAL for any other overlap of the two extents
 * (frames * frame_samples samples each).  The ragged form cannot know its
 * extent on the host: a partial overlap there is the caller's error, and
 * ragged frames must not overlap each other.
 *
 * One fused rotate-and-shift launch, asynchronous on `stream`: 16 bytes of
 * traffic per sample, no device allocation, no host read of d_meta.  Out of
 * place every 1024-sample tile of every frame is a workgroup of its own (the
 * ragged form: eight workgroups per frame).  In place a frame's tiles depend
 * on each other when off != 0, so one workgroup owns the frame and walks its
 * tiles in memmove order: in-place parallelism is per frame.  A batch of many
 * frames fills the GPU either way; a single very long buffer is what
 * lphy_hip_compensate is for.
 *
 * Returns -EINVAL for a null ctx, then 0 for frames == 0; -EINVAL for a null
 * d_in, d_out, d_meta or d_desc; -ERANGE for frames >= 2^31 (uniform form:
 * also when frames * frame_samples * 8 bytes overflows size_t); 0 for
 * frame_samples == 0; -EINVAL for the partial overlap above.  All of it
 * before any device call.
 * --------------------------------------------------------------------- */
int lphy_hip_compensate_batch(lphy_hip_ctx* ctx, const float* d_in, float* d_out,
                              size_t frames, size_t frame_samples,
                              const lphy_frame_meta* d_meta, void* stream);

/* The same for frames of different lengths: frame f is d_desc[f].samples
 * samples at d_desc[f].iq_offset (in samples), in d_in and in d_out alike.
 * sym_offset and unit_offset are not read, nor is record [frames].  Gaps
 * between frames in d_out keep their contents; a frame of 0 samples writes
 * nothing. */
int lphy_hip_compensate_ragged(lphy_hip_ctx* ctx, const float* d_in, float* d_out,
                               const lphy_ragged_desc* d_desc, size_t frames,
                               const lphy_frame_meta* d_meta, void* stream);

/* lora_modulate (LoRaMod.cpp:8-43) for `frames` frames of `nsyms` symbols
 * each (d_syms + f*nsyms) into d_iq + 2*f*(nsyms+2)*N*osr floats; bit-exact
 * with the reference.  Producer for synthetic input, not on the timed path
 * (the transmit path built for throughput is lphy_hip_modulate_ragged /
 * lphy_hip_tx_ragged, below, which also take frames of one length). */
int lphy_hip_modulate_batch(lphy_hip_ctx* ctx, const uint16_t* d_syms,
                            size_t frames, size_t nsyms, float* d_iq,
                            float amplitude, uint8_t sync, void* stream);

/* ------------------------------------------------------------------------
 * Ragged transmit: encode and modulate frames of different lengths in one
 * call, on the same lphy_ragged_desc table as the receive side.  A table made
 * by lphy_hip_tx_layout (or lphy_hip_ragged_layout in mode
 * LPHY_MODE_LORA_DEMODULATE on samples = (2*len + 2) * N * osr) serves both
 * directions: lphy_hip_tx_ragged turns bytes into IQ, and
 * lphy_hip_demod_ragged(..., LPHY_MODE_DECHIRP_LORA_DEMODULATE, LPHY_F_DECODE)
 * on the same table turns that IQ back into bytes at the same offsets.
 *
 * Frame f, with step = N * osr and total = samples / step:
 *   - total < 2: the frame writes nothing.  Otherwise nsyms = total - 2.
 *   - lphy_hip_modulate_ragged reads nsyms symbols at d_syms + sym_offset.
 *     lphy_hip_tx_ragged reads nsyms / 2 bytes at d_bytes + sym_offset / 2;
 *     byte j gives symbols 2j and 2j + 1, encodeHamming84sx of its high, then
 *     its low nibble (LoRaCodes.hpp:229-242); it modulates 2 * (nsyms / 2)
 *     data symbols and, when d_syms_out is not NULL, also stores them at
 *     d_syms_out + sym_offset.
 *   - The IQ goes to d_iq + 2 * iq_offset floats: sync symbol 0, sync symbol
 *     1, the data symbols; bit for bit what lora_modulate gives for that frame
 *     alone with the context's sf, bandwidth and osr.  The phase starts at 0
 *     in every frame; the amplitude is clamped to [-1, 1] (LoRaMod.cpp:18).
 *   - The frame's samples past its last modulated symbol, the gaps between
 *     frames and d_syms_out outside the frames' slots are left untouched.
 *   - unit_offset is read: the exclusive prefix sum of total in record order,
 *     the sum in record [frames], as for lphy_hip_demod_ragged.  Frames may
 *     lie in any address order and must not overlap.
 *
 * Returns -EINVAL for a null ctx, then 0 for frames == 0; -EINVAL for a null
 * d_syms / d_bytes, d_desc or d_iq (the device forms cannot see whether any
 * data symbol exists, so the source is always required there); -ERANGE for
 * frames >= 2^31; -ENOTSUP for SF < 7.  Every osr the context accepts is in
 * scope.
 *
 * The device forms are asynchronous on `stream`, allocate nothing on the
 * device and read no descriptor on the host.  Two launches: one thread per
 * frame walks the frame's phase recurrence and parks the phase at each symbol
 * start in that symbol's own first output sample; a persistent grid over the
 * symbols then writes every sample with 16-byte stores ("Ragged
 * transmit").  This path is for throughput: many frames per call.  A single
 * packet stays lphy_hip_modulate_host's case, whose walk is parallel within
 * the frame.
 *
 * The host form goes through the context's stream and staging like
 * lphy_hip_demod_host, and checks the table before any device call: the
 * limits and the prefix as lphy_hip_demod_ragged_host, and -EINVAL for a frame
 * with samples % step != 0, with total < 2 or with an odd nsyms.  h_bytes may
 * be NULL only when no frame has data symbols; h_syms_out may be NULL.  h_iq
 * and h_syms_out span the descriptors' extent; what no frame owns keeps the
 * caller's values (those buffers are uploaded only when the frames leave gaps
 * in them).
 * --------------------------------------------------------------------- */
int lphy_hip_modulate_ragged(lphy_hip_ctx* ctx, const uint16_t* d_syms,
                             const lphy_ragged_desc* d_desc, size_t frames,
                             float* d_iq, float amplitude, uint8_t sync,
                             void* stream);
int lphy_hip_tx_ragged(lphy_hip_ctx* ctx, const uint8_t* d_bytes,
                       const lphy_ragged_desc* d_desc, size_t frames,
                       float* d_iq, uint16_t* d_syms_out /* may be NULL */,
                       float amplitude, uint8_t sync, void* stream);
int lphy_hip_tx_ragged_host(lphy_hip_ctx* ctx, const uint8_t* h_bytes,
                            const lphy_ragged_desc* h_desc, size_t frames,
                            float* h_iq, uint16_t* h_syms_out, float amplitude,
                            uint8_t sync);

/* Host-only, no device work: h_desc[frames + 1] for frames of h_len_bytes[f]
 * payload bytes, packed back to back: lphy_hip_ragged_layout in mode
 * LPHY_MODE_LORA_DEMODULATE on samples = (2*len + 2) * N * osr, so sym_offset
 * / 2 is the exclusive prefix of len.  Returns 0, -EINVAL (null pointer),
 * -ERANGE (a frame of 2^31 samples or more, or the limits of
 * lphy_hip_ragged_layout) or -ENOMEM. */
int lphy_hip_tx_layout(const lphy_hip_ctx* ctx, const uint64_t* h_len_bytes,
                       size_t frames, lphy_ragged_desc* h_desc);

/* Host-buffer convenience used by the C++ shim: uploads, runs
 * lphy_hip_demod_batch, downloads, on the context's own stream and staging
 * (lphy_hip_ctx_reserve); returns when that stream is done, without waiting
 * for other work on the device.  Calls on one context are serialised; use
 * one context per thread (lphy_hip_ctx_share) for concurrent calls. */
int lphy_hip_demod_host(lphy_hip_ctx* ctx, const float* h_iq, size_t frames,
                        size_t frame_samples, uint16_t* h_syms,
                        uint8_t* h_bytes, lphy_frame_meta* h_meta, int mode,
                        unsigned flags);
int lphy_hip_decode_host(lphy_hip_ctx* ctx, const uint16_t* h_syms,
                         size_t count, uint8_t* h_bytes, lphy_frame_meta* h_meta);
int lphy_hip_estimate_host(lphy_hip_ctx* ctx, const float* h_iq,
                           size_t count, lphy_frame_meta* h_meta);
int lphy_hip_compensate_host(lphy_hip_ctx* ctx, float* h_iq, size_t count,
                             float cfo, float time_offset);
/* lphy_hip_compensate_batch on host buffers, in place (h_iq: frames *
 * frame_samples samples, h_meta: frames records, read only). */
int lphy_hip_compensate_batch_host(lphy_hip_ctx* ctx, float* h_iq, size_t frames,
                                   size_t frame_samples, const lphy_frame_meta* h_meta);
int lphy_hip_modulate_host(lphy_hip_ctx* ctx, const uint16_t* h_syms,
                           size_t nsyms, float* h_iq, float amplitude,
                           uint8_t sync);

/* Streaming ingestion.  Reads the reference receive
 * runner's input format - float32 (I, Q) pairs back to back, from a file or
 * stdin (runners/rx_runner.cpp:61-79) - from file descriptor `fd` until EOF
 * or `max_frames` frames, whichever comes first, as consecutive frames of
 * `frame_samples` samples, and demodulates them (lphy_hip_demod_batch,
 * `mode`, `flags`) in chunks of `chunk_frames` (0: whole frames of about
 * 64 MiB): the read of one chunk into
 * pinned host memory and its H2D copy (copy stream) overlap the
 * demodulation of the previous one (compute stream).  Results land in the
 * caller's host arrays in stream order (frame f at h_syms +
 * f*lphy_hip_syms_per_frame, h_bytes + f*(syms/2) with LPHY_F_DECODE,
 * h_meta + f).  A seekable fd is read by a pool of reader threads
 * (LPHY_STREAM_READERS, default one per usable CPU but one); a regular file
 * is mapped read-only and the readers copy out of the mapping with
 * non-temporal stores (LPHY_STREAM_COPY=pread: pread instead; the file
 * size is re-read before each chunk, but as with any mapping, a truncation
 * racing a chunk's copy can raise SIGBUS); the pinned
 * slots and streams stay with the context for its next call, and calls on
 * one context are serialised (a second thread's call waits for the first);
 * use one context per thread (lphy_hip_ctx_share) for concurrent streams.
 * `max_frames` is their capacity in frames and is required
 * (0 gives -EINVAL): reading stops there and the rest of the stream is left
 * unread on `fd` for a later call.  Synchronous.
 * *frames_out = whole frames demodulated; *tail_bytes (optional) = bytes of
 * a trailing partial frame, which is not demodulated (the runner rejects a
 * partial symbol count, rx_runner.cpp:87-91).  Returns 0, -EINVAL, -EIO
 * (read or HIP error) or a lphy_hip_demod_batch shape error. */
int lphy_hip_demod_stream(lphy_hip_ctx* ctx, int fd, size_t frame_samples,
                          size_t chunk_frames, int mode, unsigned flags,
                          size_t max_frames, uint16_t* h_syms, uint8_t* h_bytes,
                          lphy_frame_meta* h_meta, size_t* frames_out,
                          size_t* tail_bytes);

/* Wait for all work queued on `stream`. */
int lphy_hip_sync(void* stream);

/* Version / build string (for tests that check the library loaded). */
const char* lphy_hip_version(void);

/* Symbols the fused kernel recomputed with the exact per-sample rotation
 * because the certified fast path could not prove its argmax (near-ties,
 * NaN, shifted windows; every symbol under LPHY_F_EXACT_ROTATION; every
 * symbol, sync symbols included, of a frame re-run whole), summed
 * over launches on `ctx`'s device since the last reset.  Diagnostic only:
 * synchronises the device.  Returns 0 or -EIO. */
int lphy_hip_recheck_count(lphy_hip_ctx* ctx, unsigned long long* out, int reset);

/* Device index checks that failed (an LDS or global index outside its
 * array) since the last reset, summed over the kernels of every SF.  Only
 * the test build (lib/test/, -DLPHY_DEBUG_BOUNDS) counts them; this library
 * returns -ENOTSUP.  Synchronises the device. */
int lphy_hip_bounds_violations(lphy_hip_ctx* ctx, unsigned long long* out, int reset);

/* ------------------------------------------------------------------------
 * Batch forms of the codec helpers of the reference's LoRaCodes.hpp (SURVEY
 * §8f rank 3) on device buffers; `stream` is a hipStream_t (NULL = default).
 * Rows are `frames` records `stride` elements apart.  Results equal the
 * reference helper applied to each row (tests/test_gpu_codes.py); elements
 * past a row's length, or past its last whole interleaver block, are left
 * alone.  Each call returns 0, -EINVAL or -ERANGE as stated with it, or -EIO
 * when the launch failed.  With frames (or count) zero an otherwise valid
 * call returns 0, null buffers included, and nothing is launched.
 * --------------------------------------------------------------------- */
enum lphy_whiten_kind {
    LPHY_WHITEN_SX1232 = 0,      /* SX1232RadioComputeWhitening (LoRaCodes.hpp:111-137) */
    LPHY_WHITEN_SX1272 = 1,      /* Sx1272ComputeWhitening (LoRaCodes.hpp:147-167)      */
    LPHY_WHITEN_SX1272_LFSR = 2  /* Sx1272ComputeWhiteningLfsr (LoRaCodes.hpp:176-189)  */
};
enum lphy_code_op {
    LPHY_CODE_ENC84 = 0,   /* encodeHamming84sx (LoRaCodes.hpp:229-242)             */
    LPHY_CODE_DEC84 = 1,   /* decodeHamming84sx (:250-281); flags bit0 error, bit1 bad */
    LPHY_CODE_ENC74 = 2,   /* encodeHamming74sx (:287-297)                          */
    LPHY_CODE_DEC74 = 3,   /* decodeHamming74sx (:306-334); flags bit0 error         */
    LPHY_CODE_ENCP54 = 4,  /* encodeParity54 (:347-350)                             */
    LPHY_CODE_CHKP54 = 5,  /* checkParity54 (:340-345); flags bit0 error             */
    LPHY_CODE_ENCP64 = 6,  /* encodeParity64 (:367-371)                             */
    LPHY_CODE_CHKP64 = 7   /* checkParity64 (:357-365); flags bit0 error             */
};
enum lphy_sum_kind {
    LPHY_SUM_SX1272_CRC = 0, /* sx1272DataChecksum over `len` bytes (LoRaCodes.hpp:92-105) */
    LPHY_SUM_HEADER = 1,     /* headerChecksum of the row's first 2 bytes (:43-67)        */
    LPHY_SUM_CHECKSUM8 = 2   /* checksum8 over `len` bytes (:32-41)                       */
};

/* binaryToGray16 (to_binary = 0) / grayToBinary16 (1), in place
 * (LoRaCodes.hpp:201-222).  -EINVAL for a null buffer with count > 0. */
int lphy_hip_gray_batch(uint16_t* d_syms, size_t count, int to_binary, void* stream);

/* diagonalInterleaveSx (LoRaCodes.hpp:376-393) per row: cw_per_frame / ppm
 * blocks of ppm codewords -> (4 + rdd) symbols each; codeword bits at and
 * above 4 + rdd are ignored, as are the codewords after the last whole block.
 * 1 <= ppm <= 16, rdd <= 4: -EINVAL otherwise, and for a null buffer with
 * frames > 0.  -ERANGE when a row's symbols exceed sym_stride or
 * cw_per_frame exceeds cw_stride. */
int lphy_hip_interleave_batch(const uint8_t* d_cw, size_t frames, size_t cw_stride, size_t cw_per_frame,
                              uint16_t* d_syms, size_t sym_stride, unsigned ppm, unsigned rdd,
                              void* stream);

/* diagonalDeterleaveSx (LoRaCodes.hpp:396-412) per row: syms_per_frame /
 * (4 + rdd) blocks -> ppm codewords each, written as the reference leaves a
 * zero-initialised codeword buffer; symbol bits at and above ppm are ignored.
 * -EINVAL as for the interleaver; -ERANGE when a row's codewords exceed
 * cw_stride or syms_per_frame exceeds sym_stride. */
int lphy_hip_deinterleave_batch(const uint16_t* d_syms, size_t frames, size_t sym_stride,
                                size_t syms_per_frame, uint8_t* d_cw, size_t cw_stride, unsigned ppm,
                                unsigned rdd, void* stream);

/* Whitening / de-whitening of the first `len` bytes of every row in place
 * (the generators are involutions).  bit_ofs and rdd as the reference's
 * bitOfs / RDD (ignored by LPHY_WHITEN_SX1232).  Any bit_ofs in
 * [0, INT_MAX] is accepted and the cost does not depend on it: the
 * generators are periodic and the offset is reduced by the period
 * (csrc/lphy_codes_plan.h).  -EINVAL for an unknown kind, rdd > 4 (the
 * SX1272 kinds), bit_ofs < 0, len > 65535, len > stride or a null buffer
 * with work to do. */
int lphy_hip_whiten_batch(uint8_t* d_bytes, size_t frames, size_t stride, size_t len, int kind,
                          int bit_ofs, unsigned rdd, void* stream);

/* Hamming / parity code `op` on `count` bytes in place; the decoders' error
 * flags go to d_flags[i] when it is not NULL.  -EINVAL for an op that is
 * no lphy_code_op or a null d_bytes with count > 0. */
int lphy_hip_hamming_batch(uint8_t* d_bytes, size_t count, int op, uint8_t* d_flags, void* stream);

/* Checksum `kind` of every row -> d_out[frame] (uint16).  LPHY_SUM_HEADER
 * ignores `len` and reads 2 bytes a row.  -EINVAL for an unknown kind, more
 * bytes a row than stride (len, or 2 for the header), or a null buffer with
 * frames > 0. */
int lphy_hip_checksum_batch(const uint8_t* d_bytes, size_t frames, size_t stride, size_t len, int kind,
                            uint16_t* d_out, void* stream);

/* lora_encode (LoRaEncoder.cpp:6-18) per row: byte j of the first `len`
 * bytes -> symbols 2j, 2j+1 (encodeHamming84sx of the high, low nibble),
 * the symbols modulate_batch takes.  -EINVAL when len > stride or a buffer
 * is null with frames and len > 0; -ERANGE when 2*len > sym_stride. */
int lphy_hip_lora_encode_batch(const uint8_t* d_bytes, size_t frames, size_t stride, size_t len,
                               uint16_t* d_syms, size_t sym_stride, void* stream);

/* ------------------------------------------------------------------------
 * LoRaWAN MAC helpers batched: lorawan::compute_mic
 * (lorawan.cpp:35-98, AES-128 CMAC over B0 || data) and parse_frame's
 * checks (lorawan.cpp:150-176) on the decoded bytes of many frames at once.
 * Keys are 16-byte records in device memory (d_keys, 16-byte aligned;
 * -EINVAL otherwise).
 * --------------------------------------------------------------------- */
typedef struct lphy_lorawan_desc { /* one MIC job */
    uint64_t offset;   /* byte offset of the frame's MHDR..FRMPayload in d_bytes */
    uint32_t len;      /* bytes the MIC covers (compute_mic's len)            */
    uint32_t devaddr;
    uint32_t fcnt;     /* 32-bit frame counter as compute_mic takes it        */
    uint32_t key;      /* index into d_keys                                   */
    uint32_t uplink;   /* nonzero: uplink (B0 byte 5 = 0)                     */
    uint32_t reserved;
} lphy_lorawan_desc;

typedef struct lphy_lorawan_frame { /* parse_frame's outcome for one row */
    int32_t  status;          /* parse_frame's return: FRMPayload length, or
                                 -EINVAL (MIC mismatch) / -ERANGE (short frame,
                                 FOpts past the MIC); -ENOKEY: key index
                                 >= nkeys (not a reference outcome)          */
    uint32_t devaddr;
    uint32_t mic;             /* MIC the frame carries (last 4 bytes)         */
    uint32_t calc_mic;        /* MIC computed over the rest                   */
    uint32_t payload_offset;  /* FRMPayload's offset in the row (status >= 0) */
    uint32_t payload_len;
    uint16_t fcnt;
    uint8_t  mhdr;            /* MType = mhdr >> 5, Major = mhdr & 3          */
    uint8_t  fctrl;           /* FOpts (at offset 8) length = fctrl & 0x0F    */
    uint8_t  fopts_len;
    uint8_t  reserved[3];
} lphy_lorawan_frame;         /* 32 bytes; all-zero but status when len < 12 */

#define LPHY_LW_APPEND 1u  /* mic_batch: also store the 4 MIC bytes (little
                              endian) right after each frame's data, as
                              build_frame does (lorawan.cpp:131-134) */

/* compute_mic for every descriptor -> d_mic[i] (NULL allowed with
 * LPHY_LW_APPEND).  d_bytes is written only with LPHY_LW_APPEND.  A
 * descriptor naming a key >= nkeys gets MIC 0 and nothing appended. */
int lphy_hip_lorawan_mic_batch(uint8_t* d_bytes, const lphy_lorawan_desc* d_desc, size_t frames,
                               const uint8_t* d_keys, size_t nkeys, uint32_t* d_mic, unsigned flags,
                               void* stream);

/* parse_frame's checks on `frames` rows of decoded bytes `stride` apart
 * (e.g. demod_batch's d_bytes): row i holds d_lens[i] bytes (d_lens NULL:
 * `len` each) and uses key d_key_index[i] (NULL: key 0).  Results in
 * d_out[i].  Lengths up to 65535 bytes and at most `stride`: a row whose
 * d_lens[i] exceeds either gets status -ERANGE and nothing of it is read
 * (a fixed `len` beyond them is -EINVAL for the whole call). */
int lphy_hip_lorawan_parse_batch(const uint8_t* d_bytes, size_t frames, size_t stride,
                                 const uint32_t* d_lens, size_t len, const uint8_t* d_keys, size_t nkeys,
                                 const uint32_t* d_key_index, lphy_lorawan_frame* d_out, void* stream);

/* One compute_mic through the batch kernel, host buffers (device `device`);
 * serialised process-wide.  Returns 0, -EINVAL, -ENODEV or -EIO. */
int lphy_hip_lorawan_mic_host(int device, const uint8_t key[16], int uplink, uint32_t devaddr, uint32_t fcnt,
                              const uint8_t* data, size_t len, uint32_t* mic);

/* ------------------------------------------------------------------------
 * LoRaWAN on the ragged table: lorawan::build_frame (lorawan.cpp:100-136) and
 * parse_frame's checks (lorawan.cpp:138-177) for frames of different lengths,
 * on the lphy_ragged_desc table of the ragged PHY calls.  Both directions are
 * then a chain of launches on one stream with no host read of the table:
 *   receive   lphy_hip_estimate_ragged -> lphy_hip_compensate_ragged ->
 *             lphy_hip_demod_ragged(LPHY_F_DECODE) -> lphy_hip_lorawan_parse_ragged
 *             -> lphy_hip_lorawan_crypt_rx_ragged
 *   transmit  lphy_hip_lorawan_crypt_tx_ragged -> lphy_hip_lorawan_build_ragged
 *             -> lphy_hip_tx_ragged
 * (the two crypt calls, the FRMPayload cipher, are described further down).
 * Neither call takes a context: symbol_samples is N * osr of the context whose
 * calls share the table (lphy_hip_symbol_samples).  Keys as above: 16-byte
 * records at d_keys, 16-byte aligned.  Both calls are one launch, asynchronous
 * on `stream`, allocate nothing on the device and read nothing of the table on
 * the host; one thread takes one frame.  Of a descriptor only samples and
 * sym_offset are read (not iq_offset, not unit_offset, not record [frames]).
 * --------------------------------------------------------------------- */

/* N * osr of the context: the samples of one symbol.  0 for a null ctx. */
size_t lphy_hip_symbol_samples(const lphy_hip_ctx* ctx);

typedef struct lphy_lorawan_tx {   /* 32 bytes, one frame to build */
    uint64_t src_offset;   /* FOpts, then FRMPayload, at d_src + src_offset   */
    uint32_t devaddr;
    uint32_t key;          /* index into d_keys                               */
    uint32_t payload_len;  /* FRMPayload bytes                                */
    uint16_t fcnt;
    uint8_t  mtype;        /* MHDR = mtype << 5 | (major & 3)                 */
    uint8_t  major;
    uint8_t  fctrl;        /* FCtrl = (fctrl & 0xF0) | fopts_len              */
    uint8_t  fopts_len;    /* 0..15                                           */
    uint8_t  reserved[6];
} lphy_lorawan_tx;

/* build_frame for every frame of a table.  Frame f, with t = d_tx[f] and d =
 * d_desc[f], has L = 12 + t.fopts_len + t.payload_len bytes and a slot of cap
 * = (d.samples / symbol_samples - 2) / 2 bytes (0 when the frame has fewer
 * than two symbols): what lphy_hip_tx_ragged sends for it and the receiver
 * parses.
 *   - Success: the bytes MHDR | DevAddr (LE) | FCtrl | FCnt (LE) | FOpts |
 *     FRMPayload | MIC (LE) go to d_bytes + d.sym_offset / 2, bit for bit what
 *     build_frame leaves in tmp_bytes: uplink = (t.mtype & 1) == 0, fcnt
 *     widened to 32 bits for B0, the key d_keys[t.key].  With d_syms_out, the
 *     2L symbols lora_encode gives for them (build_frame's output) go to
 *     d_syms_out + d.sym_offset.  d_status[f] = 2L, build_frame's return.
 *   - A failure writes d_status[f] and nothing else.  In this order: -EINVAL
 *     for t.fopts_len > 15 or t.mtype > 7; -ENOKEY for t.key >= nkeys; -ERANGE
 *     for d.samples >= 2^31; -ERANGE for L != cap.  The reference refuses
 *     needed > tmp_cap; a frame shorter than its slot is refused too, because
 *     the whole slot goes on air and the receiver parses the whole slot, so it
 *     could never verify.
 *   - Frames sit back to back at byte granularity (any alignment), and their
 *     neighbours are written at the same time: every byte of d_bytes is stored
 *     as a byte, so no dword a frame does not wholly own is read and written
 *     back.  A symbol pair is one 32-bit store when d.sym_offset is even, two
 *     16-bit stores otherwise.  Bytes of d_bytes and symbols of d_syms_out that
 *     no frame owns keep their contents; frames must not overlap.
 *   - d_src is read in aligned dwords that hold at least one byte of the
 *     frame's FOpts / FRMPayload, never another (so no read leaves the pages
 *     the source bytes are on).  A frame with neither reads nothing of d_src.
 * Returns 0 for frames == 0; -EINVAL for a null d_src, d_tx, d_desc, d_keys,
 * d_bytes or d_status (a null d_syms_out is allowed), symbol_samples == 0,
 * nkeys == 0, or d_keys / d_tx not 16-byte aligned; -ERANGE for frames >=
 * 2^31.  All of it before the launch. */
int lphy_hip_lorawan_build_ragged(const uint8_t* d_src, const lphy_lorawan_tx* d_tx,
                                  const lphy_ragged_desc* d_desc, size_t frames, size_t symbol_samples,
                                  const uint8_t* d_keys, size_t nkeys, uint8_t* d_bytes,
                                  uint16_t* d_syms_out /* may be NULL */, int32_t* d_status, void* stream);

/* Host-only, no device work: h_desc[frames + 1] for the frames of h_tx, packed
 * back to back: lphy_hip_tx_layout on the lengths L = 12 + fopts_len +
 * payload_len, so every frame's slot is exactly L bytes.  Returns what
 * lphy_hip_tx_layout returns, and -EINVAL for a null ctx or a fopts_len > 15. */
int lphy_hip_lorawan_tx_layout(const lphy_hip_ctx* ctx, const lphy_lorawan_tx* h_tx, size_t frames,
                               lphy_ragged_desc* h_desc);

typedef struct lphy_lorawan_session { /* one session of the DevAddr lookup */
    uint32_t devaddr;
    uint32_t key;                     /* index into d_keys */
} lphy_lorawan_session;

/* parse_frame's checks on what lphy_hip_demod_ragged(..., mode, LPHY_F_DECODE)
 * left in d_bytes.  Row f, with d = d_desc[f], is len = out / 2 bytes at
 * d_bytes + d.sym_offset / 2, where out is lphy_hip_syms_per_frame of d.samples
 * in `mode`: exactly the bytes that call wrote for the frame.  d_out[f] is the
 * lphy_lorawan_frame lphy_hip_lorawan_parse_batch gives for that row, and
 * before anything of the row is read:
 *   - d.samples >= 2^31: status -ERANGE, the rest of the record zero;
 *   - with d_meta, d_meta[f].status != 0: that status, the rest zero
 *     (parse_frame returns decode's error, lorawan.cpp:149; the per-frame
 *     length statuses of lphy_hip_demod_ragged flow through the same way).
 *     crc_ok is not consulted, as the reference does not consult it;
 *   - len < 12 or len > 65535: status -ERANGE, the rest zero.
 * Which key a frame gets:
 *   - d_key_index[f], as in lphy_hip_lorawan_parse_batch (an index >= nkeys:
 *     status -ENOKEY, the rest zero);
 *   - neither d_key_index nor d_sessions: key 0;
 *   - d_sessions: found by the row's DevAddr.  The table holds nsessions
 *     records sorted by devaddr ascending (lphy_hip_lorawan_sessions_check);
 *     equal DevAddrs are allowed, LoRaWAN does not make them unique.  A
 *     lower-bound search finds the first record with the row's DevAddr; the
 *     records with that DevAddr are then tried in table order, the first 8 of
 *     them at most (a fixed bound, so no table makes a thread spin: records
 *     past the eighth are not tried).  Of those, records whose key >= nkeys
 *     are skipped; the first one whose MIC matches wins.  No record, or none
 *     with a usable key: status -ENOKEY, the header fields and the carried mic
 *     filled, calc_mic = 0.  Candidates but no match: status -EINVAL, calc_mic
 *     the first candidate's.  An unsorted table cannot lead outside it; which
 *     records are then tried is unspecified.
 * d_key_used[f] (optional) receives the index of the key calc_mic was computed
 * with (on a session mismatch: the first candidate's), 0xFFFFFFFF when no MIC
 * was computed.
 * Returns 0 for frames == 0; -EINVAL for a null d_bytes, d_desc, d_keys or
 * d_out, nkeys == 0, a mode outside 0..2, symbol_samples == 0, d_keys / d_out
 * not 16-byte aligned, both d_key_index and d_sessions, or d_sessions with
 * nsessions == 0; -ERANGE for frames >= 2^31.  All of it before the launch. */
int lphy_hip_lorawan_parse_ragged(const uint8_t* d_bytes, const lphy_ragged_desc* d_desc, size_t frames,
                                  size_t symbol_samples, int mode,
                                  const lphy_frame_meta* d_meta /* may be NULL */, const uint8_t* d_keys,
                                  size_t nkeys, const uint32_t* d_key_index /* may be NULL */,
                                  const lphy_lorawan_session* d_sessions /* may be NULL */, size_t nsessions,
                                  lphy_lorawan_frame* d_out, uint32_t* d_key_used /* may be NULL */,
                                  void* stream);

/* Host-only: 0 when the table is sorted by devaddr ascending (equal DevAddrs
 * allowed, n == 0 included), -EINVAL when it is not or is null with n > 0. */
int lphy_hip_lorawan_sessions_check(const lphy_lorawan_session* h_sessions, size_t n);

/* ------------------------------------------------------------------------
 * The FRMPayload cipher (LoRaWAN 1.0.x 4.3.3), an extension beside
 * compute_mic: the reference sends Frame::payload as given.  For a range of
 * len bytes, block A_i (i = 1 .. ceil(len / 16)) is B0 of compute_mic
 * (lorawan.cpp:46-58) with byte 0 = 0x01 and byte 15 = i:
 *   01 | 00 00 00 00 | dir (0 up, 1 down) | DevAddr LE | FCnt LE (32 bit) | 00 | i
 * S_i = AES128(K, A_i), and byte j of the range becomes byte ^ S_(j/16+1)[j%16].
 * The operation is its own inverse.  i is one byte: a range of more than 4080
 * bytes is refused.
 *
 * d_keys is the table of the keys that cipher payloads (AppSKey in practice),
 * 16-byte records, 16-byte aligned, indexed like the NwkSKey table given to
 * build and parse, so one session index serves both.  The three device forms
 * are one launch each, asynchronous on `stream`, allocate nothing on the device
 * and read no table on the host.  A group of lanes shares a range and takes its
 * 16-byte blocks in turn.  Ranges sit at any byte and their neighbours are
 * written at the same time: bytes in front of a block's first aligned dword and
 * behind its last whole one are stored as bytes, the dwords a block fills as
 * dwords, and nothing is read and written back.  Reads are aligned dwords that
 * hold at least one byte of the range.  Ranges must not overlap.  d_status
 * (optional) receives one int32 per record.
 * All three return 0 for a zero count; -EINVAL for a null required pointer,
 * nkeys == 0, d_keys or the 32-byte records (d_desc of the batch form, d_tx,
 * d_parsed) not 16-byte aligned, skip > 1, symbol_samples == 0 or a mode outside
 * 0..2; -ERANGE for a count >= 2^31.  All of it before the launch.
 * --------------------------------------------------------------------- */

/* Job i ciphers d_bytes[offset .. offset + len) in place with devaddr, fcnt (all
 * 32 bits), key and uplink of d_desc[i].  d_status[i]: 0; -ENOKEY for key >=
 * nkeys; -ERANGE for len > 4080.  A refused job writes nothing else; len == 0
 * writes nothing and gives 0. */
int lphy_hip_lorawan_crypt_batch(uint8_t* d_bytes, const lphy_lorawan_desc* d_desc, size_t jobs,
                                 const uint8_t* d_keys, size_t nkeys, int32_t* d_status /* may be NULL */,
                                 void* stream);

/* Before lphy_hip_lorawan_build_ragged, on the same stream, d_src and d_tx:
 * ciphers the FRMPayload of every frame where build will read it.  Frame f,
 * with t = d_tx[f]: the range is the t.payload_len - skip bytes at d_src +
 * t.src_offset + t.fopts_len + skip (nothing when payload_len <= skip), with
 * t.devaddr, t.fcnt widened with zeros as build widens it for B0, uplink =
 * (t.mtype & 1) == 0 and the key d_keys[t.key].  skip is 0 or 1: with 1 the
 * first FRMPayload byte stays clear (the reference's frame has no FPort field;
 * a caller who sends one puts it there).  d_status[f], in build's order:
 * -EINVAL for t.fopts_len > 15 or t.mtype > 7; -ENOKEY for t.key >= nkeys;
 * -ERANGE for a range over 4080 bytes; else 0.  FOpts, the skipped byte and
 * everything else in d_src keep their contents. */
int lphy_hip_lorawan_crypt_tx_ragged(uint8_t* d_src, const lphy_lorawan_tx* d_tx, size_t frames,
                                     const uint8_t* d_keys, size_t nkeys, unsigned skip,
                                     int32_t* d_status /* may be NULL */, void* stream);

/* After lphy_hip_lorawan_parse_ragged, on its outputs: deciphers the FRMPayload
 * of every accepted frame in place.  Frame f, with r = d_parsed[f] and d =
 * d_desc[f]; its row is the len bytes at d_bytes + d.sym_offset / 2 that the
 * parse call defines from d.samples, symbol_samples and mode.  d_status[f], in
 * this order, with nothing of the row read or written for any of them:
 *   - d.samples >= 2^31: -ERANGE;
 *   - r.status < 0: that status;
 *   - r.payload_offset + r.payload_len + 4 > len, or r.payload_offset < 8:
 *     -EINVAL (a record that did not come from the parse call cannot lead
 *     outside the frame's slot);
 *   - the key index d_key_used[f] (NULL: key 0) is 0xFFFFFFFF or >= nkeys:
 *     -ENOKEY;
 *   - a range over 4080 bytes: -ERANGE.
 * Otherwise the bytes payload_offset + skip .. payload_offset + payload_len of
 * the row are deciphered with r.devaddr, r.fcnt widened with zeros and uplink =
 * ((r.mhdr >> 5) & 1) == 0, and the status is 0.  The header, FOpts, the
 * skipped byte, the MIC and other frames' bytes are untouched.  After this call
 * the MIC a row carries no longer covers the bytes in the buffer: it was
 * computed over the ciphertext, so parse the rows before, not after. */
int lphy_hip_lorawan_crypt_rx_ragged(uint8_t* d_bytes, const lphy_ragged_desc* d_desc,
                                     const lphy_lorawan_frame* d_parsed,
                                     const uint32_t* d_key_used /* may be NULL: key 0 */, size_t frames,
                                     size_t symbol_samples, int mode, const uint8_t* d_keys, size_t nkeys,
                                     unsigned skip, int32_t* d_status /* may be NULL */, void* stream);

/* One range through the batch kernel, host buffer in place (device `device`);
 * serialised process-wide with lphy_hip_lorawan_mic_host.  Returns 0, -EINVAL,
 * -ERANGE (len > 4080), -ENODEV or -EIO. */
int lphy_hip_lorawan_crypt_host(int device, const uint8_t key[16], int uplink, uint32_t devaddr, uint32_t fcnt,
                                uint8_t* data, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* LPHY_HIP_H */
