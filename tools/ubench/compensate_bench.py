#!/usr/bin/env python3
"""lphy_hip_compensate_batch against the single-buffer call, same box, same session.

Shape: the C1 IQ buffer, SF 7 x 65,536 frames x 66 symbols (553.6 M samples,
4.4 GB).  Per-frame offsets, fixed seed:
  (a) every off = 0, |cfo| <= 0.1 (rate * n stays below 120: sincosf's straight path)
  (b) off uniform in [-N, N] \\ {0}, the same cfo
  (c) off = 0, |cfo| = 0.45: rate * n passes 120 from sample ~5,400 of 8,448 on, so
      about a third of the samples take sincosf's large-argument reduction
New code: compensate_batch out of place and in place for (a) and (b), out of
place for (c).  Baseline: lphy_hip_compensate on the same buffer as one frame
with one non-zero shift (its two launches through a scratch buffer of the
input's size, 32 B of traffic per sample) and cfo = 1e-6, so that its angles
stay on the straight path too (one frame's n runs to 5.5e8).

HIP events around each call, warm-up runs, then timed repetitions with the
variants alternating; medians and min-max.  The in-place runs start from a
fresh copy of the input each time (copied outside the timed window).  GB/s
and the share of the 8 TB/s roofline are against the algorithmic 16 B per
sample.  Before timing, the batch output for the first frames is compared bit
for bit with lphy_hip_compensate on each of those frames alone, and the
in-place output with the out-of-place one.

    python tools/ubench/compensate_bench.py --out profiles/compensate/compensate_bench.json
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "lora-sdr-lightweight-standalone-library-clean_amd"))
import lphy  # noqa: E402

HBM = 8.0e12


def meta_tensor(cfo, toff, dev):
    m = np.zeros(cfo.size, lphy.META_DTYPE)
    m["cfo"], m["time_offset"] = cfo, toff
    return torch.from_numpy(m.view(np.uint8).copy()).to(dev)


def bits(t):
    return t.view(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sf", type=int, default=7)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--symbols", type=int, default=66)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("compensate_bench: no HIP device")
    dev = torch.device("cuda:0")
    sf, frames = a.sf, a.frames
    N = 1 << sf
    fs = a.symbols * N
    total = frames * fs
    d = lphy.Demodulator(sf)
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2026)
    gen = torch.Generator(device=dev).manual_seed(7)
    src = torch.randn(total * 2, dtype=torch.float32, device=dev, generator=gen)
    work = torch.empty_like(src)
    dst = torch.empty_like(src)
    cfo = rng.uniform(-0.1, 0.1, frames).astype(np.float32)
    off = rng.integers(1, N + 1, frames) * rng.choice([-1, 1], frames)
    metas = {"a": meta_tensor(cfo, np.zeros(frames, np.float32), dev),
             "b": meta_tensor(cfo, off.astype(np.float32), dev),
             "c": meta_tensor(np.where(cfo < 0, -0.45, 0.45).astype(np.float32), np.zeros(frames, np.float32), dev)}

    # the results first: batch == the single-buffer call per frame, in place == out of place
    for k in ("a", "b", "c"):
        d.compensate_batch(src, dst, frames, fs, metas[k], stream=st)
        work.copy_(src)
        d.compensate_batch(work, work, frames, fs, metas[k], stream=st)
        torch.cuda.synchronize()
        assert torch.equal(bits(work), bits(dst)), f"({k}) in place differs from out of place"
        m = metas[k].cpu().numpy().view(lphy.META_DTYPE)
        for f in range(8):
            one = src[2 * f * fs: 2 * (f + 1) * fs].clone()
            rc = d.lib.lphy_hip_compensate(d.ctx, one.data_ptr(), fs, float(m["cfo"][f]), float(m["time_offset"][f]), st)
            assert rc == 0
            torch.cuda.synchronize()
            assert torch.equal(bits(one), bits(dst[2 * f * fs: 2 * (f + 1) * fs])), f"({k}) frame {f} differs"

    def out_of_place(k):
        return lambda: d.compensate_batch(src, dst, frames, fs, metas[k], stream=st)

    def in_place(k):
        return lambda: d.compensate_batch(work, work, frames, fs, metas[k], stream=st)

    def baseline():
        rc = d.lib.lphy_hip_compensate(d.ctx, work.data_ptr(), total, 1e-6, 37.0, st)
        assert rc == 0

    variants = [("batch_out_a", out_of_place("a"), False), ("batch_in_a", in_place("a"), True),
                ("batch_out_b", out_of_place("b"), False), ("batch_in_b", in_place("b"), True),
                ("batch_out_c", out_of_place("c"), False), ("single_buffer_shift", baseline, True)]

    def timed(fn, fresh):
        if fresh:
            work.copy_(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        for _, fn, fresh in variants:
            timed(fn, fresh)
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.reps):
        for name, fn, fresh in variants:
            times[name].append(timed(fn, fresh))

    res = {"device": torch.cuda.get_device_name(0), "sf": sf, "frames": frames, "frame_samples": fs,
           "samples": total, "algorithmic_bytes": total * 16, "reps": a.reps, "warmup": a.warmup,
           "outputs_equal": True, "variants": {}}
    for name, t in times.items():
        med = float(np.median(t))
        res["variants"][name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t),
                                 "ns_per_sample": med * 1e6 / total,
                                 "algorithmic_GBps": total * 16 / (med * 1e-3) / 1e9,
                                 "roofline_fraction": total * 16 / (med * 1e-3) / HBM}
    res["variants"]["single_buffer_shift"]["traffic_bytes"] = total * 32
    base = res["variants"]["single_buffer_shift"]["median_ms"]
    for name in times:
        res["variants"][name]["time_over_single_buffer"] = res["variants"][name]["median_ms"] / base
    for name, v in res["variants"].items():
        print(json.dumps({name: v}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    d.close()


if __name__ == "__main__":
    main()
