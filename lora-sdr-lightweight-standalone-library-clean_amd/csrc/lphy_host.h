// lphy_host.h — the host-buffer convenience entry points (*_host,
// synchronous), included by lphy_hip.hip alone, after the device-buffer forms
// they call.  Each call runs on the context's own stream and waits for that
// stream only: host copies in (async, ordered on the stream), the kernels,
// host copies out, hipStreamSynchronize.  Staging comes from
// lphy_hip_ctx_reserve; a call larger than the reservation grows it (the
// only allocation after it).  Where the buffers lie: lphy_stage_plan.h.
#pragma once
#include "lphy_stage_plan.h"

#include <initializer_list>

namespace {

int ensure_host_stage(lphy_hip_ctx* c, size_t bytes) {
    if (c->stage_bytes >= bytes) return 0;
    // the old staging may still be read by this context's stream
    if (c->d_stage) HIP_OK(hipStreamSynchronize(c->stream));
    return ensure_stage(c, bytes);
}

// One *_host call: the context's lock and device for its lifetime, the
// call's slices in the staging (begin), their device pointers (dev), the
// copies back and the wait (finish).  Leaving the call any other way after
// begin() - an *_impl that refuses it, a HIP call that fails - waits for the
// stream in the destructor, so no call returns while a copy from or into the
// caller's buffers, or a kernel on the staging, can still run.
//
// kMirror: demod, decode and modulate (the per-packet calls of the lora_phy::
// API) go through the pinned mirror when their copied slices fit
// it, one DMA copy each way; the other eight copy slice by slice from and to
// the caller's memory.  Which call does which is a measured choice, not an
// accident of this code.
enum HostCopy { kPageable, kMirror };

class HostCall {
public:
    HostCall(lphy_hip_ctx* c, HostCopy copy) : c_(c), lk_(c->mu), copy_(copy), set_device_(hipSetDevice(c->device)) {}
    ~HostCall() {
        if (busy_) (void)hipStreamSynchronize(c_->stream);
    }

    // `host`: the caller's pointer of each copied slice, in the plan's order;
    // null: that slice is not copied
    int begin(const StagePlan& plan, std::initializer_list<const void*> host) {
        HIP_OK(set_device_);
        plan_ = plan;
        std::copy(host.begin(), host.end(), host_);
        if (int rc = ensure_host_stage(c_, plan_.end)) return rc;
        base_ = static_cast<char*>(c_->d_stage);
        size_t mirror = c_->h_stage_bytes;
#ifdef LPHY_TEST_PATHS
        mirror = std::min(mirror, c_->pinned_max.load(std::memory_order_relaxed));
#endif
        h_ = copy_ == kMirror && plan_.copied_end <= mirror ? static_cast<char*>(c_->h_stage) : nullptr;
        busy_ = true;
        for (int i = 0; i < plan_.n; ++i) {
            const StageSlice& s = plan_.s[i];
            if (!s.size) continue;
            if (s.role & kStageZero) {
                if (h_) std::memset(h_ + s.off, 0, s.size);
                else HIP_OK(hipMemsetAsync(base_ + s.off, 0, s.size, stream()));
            } else if ((s.role & kStageIn) && host_[i]) {
                if (h_) std::memcpy(h_ + s.off, host_[i], s.size);
                else HIP_OK(hipMemcpyAsync(base_ + s.off, host_[i], s.size, hipMemcpyHostToDevice, stream()));
            }
        }
        if (h_ && plan_.up.end > plan_.up.begin)
            HIP_OK(hipMemcpyAsync(base_ + plan_.up.begin, h_ + plan_.up.begin, plan_.up.end - plan_.up.begin,
                                  hipMemcpyHostToDevice, stream()));
        return 0;
    }

    template <class T>
    T* dev(int slice) const {
        return reinterpret_cast<T*>(base_ + plan_.s[slice].off);
    }
    hipStream_t stream() const { return c_->stream; }

    // rc: the *_impl's.  (Inlined: the copies into the caller's buffers then
    // belong to the entry point's own frame in a sanitizer's report.)
    __attribute__((always_inline)) int finish(int rc) {
        if (rc) return rc;
        const StageSpan& d = plan_.down;
        if (h_ && d.end > d.begin)
            HIP_OK(hipMemcpyAsync(h_ + d.begin, base_ + d.begin, d.end - d.begin, hipMemcpyDeviceToHost, stream()));
        for (int i = 0; i < plan_.n; ++i) {
            const StageSlice& s = plan_.s[i];
            if (!h_ && out(i)) HIP_OK(hipMemcpyAsync(out(i), base_ + s.off, s.size, hipMemcpyDeviceToHost, stream()));
        }
        HIP_OK(hipStreamSynchronize(stream()));
        busy_ = false;
        for (int i = 0; i < plan_.n; ++i)
            if (h_ && out(i)) std::memcpy(out(i), h_ + plan_.s[i].off, plan_.s[i].size);
        return 0;
    }

private:
    // where slice i goes back to, if anywhere
    void* out(int i) const {
        return (plan_.s[i].role & kStageOut) && plan_.s[i].size ? const_cast<void*>(host_[i]) : nullptr;
    }

    lphy_hip_ctx* c_;
    std::lock_guard<std::mutex> lk_;
    HostCopy copy_;
    hipError_t set_device_;
    StagePlan plan_;
    const void* host_[StagePlan::kMaxSlices] = {};
    char* base_ = nullptr;  // the staging
    char* h_ = nullptr;     // its pinned mirror, when this call goes through it
    bool busy_ = false;     // enqueued on the stream and not yet waited for
};

}  // namespace

extern "C" {

int lphy_hip_ctx_reserve(lphy_hip_ctx* c, size_t frames, size_t frame_samples) {
    if (!c) return -EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_OK(hipSetDevice(c->device));
    const size_t total = frame_samples / ((size_t)c->N * c->osr);
    return ensure_host_stage(c, host_stage_bytes(c->N, c->osr, std::max<size_t>(frames, 1), frame_samples,
                                                 mod_scratch_bytes(c, 1, total)));
}

int lphy_hip_demod_host(lphy_hip_ctx* c, const float* h_iq, size_t frames,
                        size_t frame_samples, uint16_t* h_syms, uint8_t* h_bytes,
                        lphy_frame_meta* h_meta, int mode, unsigned flags) {
    if (!c || !h_iq || !h_meta) return -EINVAL;
    HostCall hc(c, kMirror);
    const bool decode = (flags & LPHY_F_DECODE) != 0;
    if (int rc = hc.begin(demod_plan(frames, frame_samples, lphy_hip_syms_per_frame(c, frame_samples, mode)),
                          {h_iq, h_syms, decode ? h_bytes : nullptr, h_meta}))
        return rc;
    return hc.finish(demod_batch_impl(c, hc.dev<float>(0), frames, frame_samples, hc.dev<uint16_t>(1),
                                      decode ? hc.dev<uint8_t>(2) : nullptr, hc.dev<lphy_frame_meta>(3), mode, flags,
                                      hc.stream(), hc.dev<void>(4)));
}

// The ragged call on host buffers: IQ, descriptors and the caller's output
// slots in, the three launches, symbols / bytes / records out.
int lphy_hip_demod_ragged_host(lphy_hip_ctx* c, const float* h_iq, const lphy_ragged_desc* h_desc, size_t frames,
                               uint16_t* h_syms, uint8_t* h_bytes, lphy_frame_meta* h_meta, int mode,
                               unsigned flags) {
    if (int rc = demod_ragged_args(ragged_ctx(c), h_desc && h_meta, mode, flags, h_bytes, frames))
        return rc > 0 ? 0 : rc;
    const bool decode = (flags & LPHY_F_DECODE) != 0;
    uint64_t iq_samples = 0, out_syms = 0;
    if (int rc = ragged_extent(c->N, h_desc, frames, mode, &iq_samples, &out_syms)) return rc;
    if ((iq_samples && !h_iq) || (out_syms && !h_syms)) return -EINVAL;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(ragged_plan(iq_samples, frames, out_syms),
                          {h_iq, h_desc, h_syms, decode ? h_bytes : nullptr, h_meta}))
        return rc;
    return hc.finish(demod_ragged_impl(c, hc.dev<float>(0), hc.dev<lphy_ragged_desc>(1), frames, hc.dev<uint16_t>(2),
                                       decode ? hc.dev<uint8_t>(3) : nullptr, hc.dev<lphy_frame_meta>(4), mode, flags,
                                       hc.stream(), h_desc[frames].unit_offset));
}

// The detector on host buffers: the samples the windows span in (h_iq[first
// .. last]), one launch, the records out.
int lphy_hip_detect_host(lphy_hip_ctx* c, const float* h_iq, size_t total_samples, size_t first, size_t hop,
                         size_t step, size_t windows, lphy_detect_rec* h_out, unsigned flags) {
    size_t last = 0;
    if (int rc = detect_check(c, h_iq, total_samples, first, hop, step, windows, h_out, flags, &last))
        return rc > 0 ? 0 : rc;
    const size_t span = last - first + 1;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(detect_plan(span, windows), {h_iq + 2 * first, h_out})) return rc;
    return hc.finish(detect_impl(c, hc.dev<float>(0), span, 0, hop, step, windows, hc.dev<lphy_detect_rec>(1), flags,
                                 hc.stream()));
}

// The ragged detector on host buffers: the table is checked first, then the
// descriptors' IQ extent and the frames + 1 records in, one launch sized by
// the table's whole symbols, that many records out.
int lphy_hip_detect_ragged_host(lphy_hip_ctx* c, const float* h_iq, const lphy_ragged_desc* h_desc, size_t frames,
                                unsigned phase, lphy_detect_rec* h_out, unsigned flags) {
    if (int rc = detect_ragged_args(ragged_ctx(c), frames, h_iq && h_desc && h_out, phase, flags))
        return rc > 0 ? 0 : rc;
    uint64_t iq_samples = 0, units = 0;
    if (int rc = detect_ragged_extent((uint64_t)c->N * c->osr, h_desc, frames, &iq_samples, &units)) return rc;
    if (units == 0) return 0;  // no frame holds a whole symbol: nothing is written
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(detect_ragged_plan(iq_samples, frames, units), {h_iq, h_desc, h_out})) return rc;
    return hc.finish(detect_ragged_impl(c, hc.dev<float>(0), hc.dev<lphy_ragged_desc>(1), frames, phase,
                                        hc.dev<lphy_detect_rec>(2), flags, hc.stream(), units));
}

// The frame search on host buffers: the records in, the six launches with the
// workspace lent from the staging, the table and the info out.
int lphy_hip_find_frames_host(lphy_hip_ctx* c, const lphy_detect_rec* h_rec, size_t windows, const lphy_find_params* p,
                              int mode, size_t max_frames, lphy_ragged_desc* h_desc, lphy_find_info* h_info) {
    if (int rc = find_frames_check(c, h_rec, windows, p, mode, max_frames, h_desc, h_info, true)) return rc;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(find_plan(windows, max_frames, find_layout(windows).bytes), {h_rec, h_desc, h_info}))
        return rc;
    return hc.finish(find_frames_impl(c, hc.dev<lphy_detect_rec>(0), windows, *p, mode, max_frames,
                                      hc.dev<lphy_ragged_desc>(1), hc.dev<lphy_find_info>(2), hc.dev<void>(3),
                                      hc.stream()));
}

// The channeliser on host buffers: the samples its outputs read (from `first`
// on, so the staged plan starts at 0), the two tables and the caller's output
// in, the one launch, the output back - all of it, so that the slots no output
// owns come back as they went.
int lphy_hip_channelize_host(lphy_hip_ctx* c, const float* h_in, const lphy_chan_plan* p, const float* h_taps,
                             const float* h_rot, float* h_out) {
    if (int rc = resample_check(chan_args, c, h_in, p, h_taps, h_rot, h_out)) return rc > 0 ? 0 : rc;
    lphy_chan_plan q = *p;
    q.in_samples = (p->outputs - 1) * p->decim + p->taps;
    q.first = 0;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(chan_plan(q.in_samples, p->channels, p->taps, p->rot_period, p->out_stride),
                          {h_in + 2 * p->first, h_taps, h_rot, h_out}))
        return rc;
    return hc.finish(
        resample_impl(c, hc.dev<float>(0), q, hc.dev<float>(1), hc.dev<float>(2), hc.dev<float>(3), hc.stream()));
}

// The same from a capture in `format`: the samples go up at the format's bytes each.
int lphy_hip_channelize_raw_host(lphy_hip_ctx* c, const void* h_in, int format, const lphy_chan_plan* p,
                                 const float* h_taps, const float* h_rot, float* h_out) {
    if (int rc = chan_raw_check(c, h_in, format, p, h_taps, h_rot, h_out)) return rc > 0 ? 0 : rc;
    const size_t bytes = chan_sample_bytes(format);
    lphy_chan_plan q = *p;
    q.in_samples = (p->outputs - 1) * p->decim + p->taps;
    q.first = 0;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(chan_raw_plan(q.in_samples * bytes, p->channels, p->taps, p->rot_period, p->out_stride),
                          {static_cast<const char*>(h_in) + p->first * bytes, h_taps, h_rot, h_out}))
        return rc;
    return hc.finish(chan_raw_impl(c, hc.dev<void>(0), format, q, hc.dev<float>(1), hc.dev<float>(2),
                                   hc.dev<float>(3), hc.stream()));
}

// The synthesiser on host buffers: the channels' streams (from the first
// channel's first sample to the last channel's last, strides included), the
// two tables in, the one launch, `outputs` samples back.
int lphy_hip_synthesize_host(lphy_hip_ctx* c, const float* h_in, const lphy_synth_plan* p, const float* h_taps,
                             const float* h_rot, float* h_out) {
    if (int rc = resample_check(synth_args, c, h_in, p, h_taps, h_rot, h_out)) return rc > 0 ? 0 : rc;
    const size_t in = p->in_samples ? (size_t)((p->channels - 1) * p->in_stride + p->in_samples) : 0;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(synth_plan(in, p->channels, p->taps, p->rot_period, p->outputs),
                          {h_in, h_taps, h_rot, h_out}))
        return rc;
    return hc.finish(
        resample_impl(c, hc.dev<float>(0), *p, hc.dev<float>(1), hc.dev<float>(2), hc.dev<float>(3), hc.stream()));
}

int lphy_hip_decode_host(lphy_hip_ctx* c, const uint16_t* h_syms, size_t count,
                         uint8_t* h_bytes, lphy_frame_meta* h_meta) {
    if (!c || !h_syms || !h_bytes || !h_meta) return -EINVAL;
    if (count & 1) return -EINVAL;
    HostCall hc(c, kMirror);
    if (int rc = hc.begin(decode_plan(count), {h_syms, h_bytes, h_meta})) return rc;
    return hc.finish(lphy_hip_decode_batch(c, hc.dev<uint16_t>(0), 1, count, hc.dev<uint8_t>(1),
                                           hc.dev<lphy_frame_meta>(2), hc.stream()));
}

int lphy_hip_estimate_host(lphy_hip_ctx* c, const float* h_iq, size_t count,
                           lphy_frame_meta* h_meta) {
    if (!c || !h_iq || !h_meta) return -EINVAL;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(estimate_plan(count), {h_iq, h_meta})) return rc;
    return hc.finish(lphy_hip_estimate_batch(c, hc.dev<float>(0), 1, count, count, hc.dev<lphy_frame_meta>(1),
                                             hc.stream()));
}

// The ragged estimate on host buffers: the descriptors' IQ extent, the
// frames' records and the caller's h_meta in, one launch, h_meta out (the
// record of a frame without a whole symbol comes back as it went).
int lphy_hip_estimate_ragged_host(lphy_hip_ctx* c, const float* h_iq, const lphy_ragged_desc* h_desc, size_t frames,
                                  size_t est_samples, lphy_frame_meta* h_meta) {
    if (int rc = ragged_args(ragged_ctx(c), frames, h_iq && h_desc && h_meta)) return rc > 0 ? 0 : rc;
    uint64_t iq_samples = 0;
    if (int rc = estimate_ragged_extent(h_desc, frames, &iq_samples)) return rc;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(estimate_ragged_plan(iq_samples, frames), {h_iq, h_desc, h_meta})) return rc;
    return hc.finish(estimate_ragged_impl(c, hc.dev<float>(0), hc.dev<lphy_ragged_desc>(1), frames, est_samples,
                                          hc.dev<lphy_frame_meta>(2), hc.stream()));
}

int lphy_hip_compensate_host(lphy_hip_ctx* c, float* h_iq, size_t count, float cfo,
                             float time_offset) {
    if (!c || !h_iq) return -EINVAL;
    if (count == 0) return 0;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(compensate_plan(count), {h_iq})) return rc;
    return hc.finish(compensate_impl(c, hc.dev<float>(0), count, cfo, time_offset, hc.stream(), hc.dev<void>(1)));
}

// The batch compensation on host buffers, in place: samples and records in,
// one launch, samples out.
int lphy_hip_compensate_batch_host(lphy_hip_ctx* c, float* h_iq, size_t frames, size_t frame_samples,
                                   const lphy_frame_meta* h_meta) {
    if (int rc = compensate_batch_check(c, h_iq, h_iq, frames, frame_samples, h_meta)) return rc > 0 ? 0 : rc;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(compensate_batch_plan(frames, frame_samples), {h_iq, h_meta})) return rc;
    return hc.finish(compensate_batch_impl(c, hc.dev<float>(0), hc.dev<float>(0), frames, frame_samples,
                                           hc.dev<lphy_frame_meta>(1), hc.stream()));
}

int lphy_hip_modulate_host(lphy_hip_ctx* c, const uint16_t* h_syms, size_t nsyms,
                           float* h_iq, float amplitude, uint8_t sync) {
    if (!c || !h_iq || (nsyms && !h_syms)) return -EINVAL;
    HostCall hc(c, kMirror);
    if (int rc = hc.begin(modulate_plan((size_t)c->N * c->osr, nsyms, mod_scratch_bytes(c, 1, nsyms)), {h_syms, h_iq}))
        return rc;
    return hc.finish(modulate_impl(c, hc.dev<uint16_t>(0), 1, nsyms, hc.dev<float>(1), amplitude, sync, hc.stream(),
                                   hc.dev<void>(2)));
}

// The ragged transmit call on host buffers: bytes and descriptors in (and the
// caller's IQ / symbols where the frames leave gaps in them), the two
// launches, IQ and symbols out.  The table is checked before any device call.
int lphy_hip_tx_ragged_host(lphy_hip_ctx* c, const uint8_t* h_bytes, const lphy_ragged_desc* h_desc, size_t frames,
                            float* h_iq, uint16_t* h_syms_out, float amplitude, uint8_t sync) {
    // (whether the bytes are needed is the table's to say)
    if (int rc = ragged_args(ragged_ctx(c), frames, h_desc && h_iq)) return rc > 0 ? 0 : rc;
    TxExtent x;
    if (int rc = tx_extent((uint64_t)c->N * c->osr, h_desc, frames, &x)) return rc;
    if (x.in_bytes && !h_bytes) return -EINVAL;
    const size_t out_syms = h_syms_out ? (size_t)x.out_syms : 0;
    HostCall hc(c, kPageable);
    if (int rc = hc.begin(tx_plan(x.in_bytes, frames, x.iq_samples, out_syms, x.iq_gaps, x.sym_gaps),
                          {h_bytes, h_desc, h_iq, h_syms_out}))
        return rc;
    return hc.finish(tx_launch(c, TxBytes{hc.dev<uint8_t>(0)}, hc.dev<lphy_ragged_desc>(1), frames, hc.dev<float>(2),
                               h_syms_out ? hc.dev<uint16_t>(3) : nullptr, amplitude, sync, hc.stream(),
                               h_desc[frames].unit_offset));
}

}  // extern "C"
