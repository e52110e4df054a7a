#!/usr/bin/env python3
"""lphy_hip_detect_batch timing: hop = N, device-resident IQ, SF 7-12.

Workload per SF (fixed seed): 2^24 samples of modulated frames (64 symbols
each, the device modulator), every symbol one window (hop = N, step = 1,
LPHY_DET_DECHIRP), as they are (clean-tone set: total - maxValue cancels in
every window, so every window takes the in-order walk) and with noise at
-8 dB (noise set).  5 warm-up runs, 20 timed repetitions between two HIP
events, median and the min-max spread.  Reports windows/s, the fraction of
the 8 TB/s roofline at 8 B per sample (the IQ read once; the 16-byte records
are 1/64 of that or less) and the serial count of one call.

    python tools/ubench/detect_bench.py --out profiles/detect/detect_bench.json
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
SAMPLES = 1 << 24


def run(sf, noisy, reps, warm):
    dev = torch.device("cuda:0")
    N = 1 << sf
    nsyms = 62
    frames = SAMPLES // ((nsyms + 2) * N)
    windows = SAMPLES // N
    rng = np.random.default_rng(2026 + sf)
    d = lphy.Demodulator(sf)
    syms = torch.from_numpy(rng.integers(0, N, (frames, nsyms), dtype=np.int64).astype(np.int16)).to(dev)
    iq = torch.empty(SAMPLES, dtype=torch.complex64, device=dev)
    d.modulate_batch(syms, frames, nsyms, torch.view_as_real(iq))
    if noisy:
        g = torch.Generator(device=dev).manual_seed(7 + sf)
        s = float(np.sqrt(10 ** 0.8 / 2))
        iq += s * torch.view_as_complex(torch.randn((SAMPLES, 2), generator=g, device=dev))
    out = torch.zeros(windows * 16, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    t_iq = torch.view_as_real(iq)

    def call():
        d.detect_batch(t_iq, SAMPLES, 0, N, 1, windows, out, lphy.DET_DECHIRP, stream=st)

    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    d.detect_serial_count(reset=True)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    serial = d.detect_serial_count() // reps
    rec = out.cpu().numpy().view(lphy.DETECT_DTYPE)
    snr = (rec["power"] - rec["power_avg"]).astype(np.float64)
    med = float(np.median(ms))
    r = {"sf": sf, "set": "noise" if noisy else "clean", "windows": windows, "reps": reps, "warmup": warm,
         "ms": {"median": med, "min": min(ms), "max": max(ms)},
         "windows_per_s": windows / (med * 1e-3), "roofline": SAMPLES * 8 / (med * 1e-3) / HBM,
         "serial_windows": int(serial), "median_power_minus_power_avg_db": float(np.median(snr))}
    d.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    res = []
    for sf in range(7, 13):
        for noisy in (True, False):
            res.append(run(sf, noisy, a.reps, a.warmup))
            print(json.dumps(res[-1]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": res}, indent=1) + "\n")


if __name__ == "__main__":
    main()
