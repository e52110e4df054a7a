#!/usr/bin/env python3
"""lphy_hip_tx_ragged against lphy_hip_lora_encode_batch + lphy_hip_modulate_batch,
same box, same session, same payloads.

Shapes (fixed seed):
  sf7_uniform   SF 7  x 65,536 frames x 32 bytes
  sf7_mixed     SF 7  x 65,536 frames, lengths uniform in 12..64 bytes
  sf12_uniform  SF 12 x  4,096 frames x 32 bytes
New code: one lphy_hip_tx_ragged call (bytes in, IQ out, no symbols out).
Baseline: encode_batch + modulate_batch, once for a uniform shape and once per
length bucket for the mixed one (53 buckets, 106 calls, each modulate_batch
taking its scratch from the stream pool).

Both paths write the same layout, so the whole outputs are compared bit for
bit before timing: the frames of one length lie together (bucket after
bucket, where the baseline's calls put them), while the ragged table lists
them in their drawn order - records against address order - so the waves of
the new path's walk pass see the mixed lengths.

HIP events around each variant, warm-up runs, then timed repetitions with the
variants alternating; medians and min-max.  GB/s and the share of the 8 TB/s
roofline are against the 8 output bytes per sample.  The acceptance condition
is recorded, not tuned: on the uniform shapes the new path may be slower than
the baseline by at most the baseline's own max - min; on the mixed shape it
must be faster.

    python tools/ubench/tx_bench.py --out profiles/tx/tx_bench.json
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


def bucket_table(lens, step):
    """Frames grouped by length in memory, listed in their drawn order."""
    lens = np.asarray(lens, np.int64)
    frames = lens.size
    values = np.unique(lens)
    desc = np.zeros(frames + 1, lphy.RAGGED_DESC_DTYPE)
    buckets = []
    iq_at = byte_at = 0
    for n in values:
        idx = np.flatnonzero(lens == n)
        samples = (2 * n + 2) * step
        desc["iq_offset"][idx] = iq_at + np.arange(idx.size) * samples
        desc["samples"][idx] = samples
        desc["sym_offset"][idx] = 2 * (byte_at + np.arange(idx.size) * n)
        buckets.append((int(n), idx.size, iq_at, byte_at))
        iq_at += idx.size * samples
        byte_at += idx.size * n
    total = 2 * lens + 2
    desc["unit_offset"][:frames] = np.cumsum(total) - total
    desc[frames] = (iq_at, 0, 2 * byte_at, total.sum())
    return desc, buckets, int(iq_at), int(byte_at)


def run_shape(name, sf, lens, reps, warmup, dev):
    d = lphy.Demodulator(sf)
    st = torch.cuda.current_stream().cuda_stream
    step = 1 << sf
    desc, buckets, n_iq, n_bytes = bucket_table(lens, step)
    frames = len(lens)
    rng = np.random.default_rng(2026)
    t_data = torch.from_numpy(rng.integers(0, 256, n_bytes + 1, dtype=np.uint8)).to(dev)
    t_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    new = torch.zeros(2 * n_iq, dtype=torch.float32, device=dev)
    old = torch.zeros(2 * n_iq, dtype=torch.float32, device=dev)
    t_sy = torch.zeros(2 * n_bytes + 2, dtype=torch.int16, device=dev)

    def tx():
        d.tx_ragged(t_data, t_desc, frames, new, None, 1.0, 0x12, stream=st, iq_samples=n_iq, out_syms=2 * n_bytes)

    def baseline():
        for n, count, iq_at, byte_at in buckets:
            sy = t_sy[2 * byte_at: 2 * byte_at + max(2 * n * count, 1)]
            lphy.lora_encode_batch(t_data[byte_at:], count, n, n, sy, 2 * n, stream=st)
            d.modulate_batch(sy, count, 2 * n, old[2 * iq_at:], 1.0, 0x12, stream=st)

    tx()
    baseline()
    torch.cuda.synchronize()
    equal = bool(torch.equal(new.view(torch.int32), old.view(torch.int32)))

    variants = [("tx_ragged", tx), ("encode_modulate_batch", baseline)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        for _, fn in variants:
            timed(fn)
    times = {k: [] for k, _ in variants}
    for _ in range(reps):
        for k, fn in variants:
            times[k].append(timed(fn))
    res = {"sf": sf, "frames": frames, "bytes_min": int(min(lens)), "bytes_max": int(max(lens)),
           "length_buckets": len(buckets), "samples": n_iq, "output_bytes": n_iq * 8, "outputs_equal": equal,
           "variants": {}}
    for k, t in times.items():
        med = float(np.median(t))
        res["variants"][k] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t),
                              "output_GBps": n_iq * 8 / (med * 1e-3) / 1e9,
                              "roofline_fraction": n_iq * 8 / (med * 1e-3) / HBM}
    v = res["variants"]
    base = v["encode_modulate_batch"]
    res["baseline_spread_ms"] = base["max_ms"] - base["min_ms"]
    res["tx_over_baseline"] = v["tx_ragged"]["median_ms"] / base["median_ms"]
    if len(buckets) == 1:
        res["condition"] = "tx median <= baseline median + baseline (max - min)"
        res["condition_met"] = v["tx_ragged"]["median_ms"] <= base["median_ms"] + res["baseline_spread_ms"]
    else:
        res["condition"] = "tx median < baseline median"
        res["condition_met"] = v["tx_ragged"]["median_ms"] < base["median_ms"]
    print(json.dumps({name: res}))
    d.close()
    del new, old, t_sy, t_data
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1, help="divide the frame counts (a quick look)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tx_bench: no HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    shapes = [("sf7_uniform", 7, np.full(65536 // a.scale, 32)),
              ("sf7_mixed", 7, rng.integers(12, 65, 65536 // a.scale)),
              ("sf12_uniform", 12, np.full(4096 // a.scale, 32))]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "shapes": {}}
    for name, sf, lens in shapes:
        res["shapes"][name] = run_shape(name, sf, lens, a.reps, a.warmup, dev)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
