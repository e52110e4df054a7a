#!/usr/bin/env python3
"""Times lphy_hip_find_frames beside its producer, lphy_hip_detect_batch, on
the same windows: SF 7, hop = N, 2^22 windows by default (4 GiB of IQ).  The
capture is noise with bursts of a tone every 64 windows, so the search finds
2^16 frames.  Device events around each call, the two alternating in one loop;
writes profiles/find_frames/bench.json.  Needs a HIP device.

  python tools/find_frames_bench.py [--log2-windows 22] [--reps 20] [--warmup 3] [--out PATH]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "lora-sdr-lightweight-standalone-library-clean_amd"))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-windows", type=int, default=22)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "find_frames" / "bench.json"))
    a = ap.parse_args()
    import torch

    import find_frames_model as model
    import lphy
    assert torch.cuda.is_available(), "needs a HIP device"
    sf, N = 7, 128
    W = 1 << a.log2_windows
    dev = torch.device("cuda:0")
    d = lphy.Demodulator(sf)
    # noise everywhere; windows 8 .. 27 of every 64 carry a tone at bin 5
    g = torch.Generator(device=dev).manual_seed(7)
    iq = torch.randn((W, N, 2), generator=g, device=dev, dtype=torch.float32) * 0.1
    burst = ((torch.arange(W, device=dev) % 64 >= 8) & (torch.arange(W, device=dev) % 64 < 28)).float()
    ph = 2 * np.pi * 5 * torch.arange(N, device=dev, dtype=torch.float32) / N
    iq[:, :, 0] += burst[:, None] * torch.cos(ph)[None, :]
    iq[:, :, 1] += burst[:, None] * torch.sin(ph)[None, :]
    iq = iq.reshape(-1)
    max_frames = W // 64 + 16
    rec = torch.zeros(W * 16, dtype=torch.uint8, device=dev)
    desc = torch.zeros((max_frames + 1) * 32, dtype=torch.uint8, device=dev)
    info = torch.zeros(32, dtype=torch.uint8, device=dev)
    work = torch.zeros(d.find_frames_workspace(W), dtype=torch.uint8, device=dev)
    prm = lphy.find_params(hop=N, total_samples=W * N, threshold_db=0.0, max_gap=1, min_symbols=4)
    st = torch.cuda.current_stream().cuda_stream

    def detect():
        d.detect_batch(iq, W * N, 0, N, 1, W, rec, 0, stream=st)

    def find():
        d.find_frames(rec, W, prm, 2, max_frames, desc, info, work, stream=st)

    times = {"detect_batch": [], "find_frames": []}
    for i in range(a.warmup + a.reps):
        for name, fn in (("detect_batch", detect), ("find_frames", find)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    got_info = info.cpu().numpy().view(lphy.FIND_INFO)[0]
    # the result at this size against the definition
    want_desc, want_info = model.find_frames(rec.cpu().numpy().view(lphy.DETECT_DTYPE), model.params(
        hop=N, total_samples=W * N, threshold_db=0.0, max_gap=1, min_symbols=4), N, 2, max_frames)
    equal = (bytes(desc.cpu().numpy()) == want_desc.astype(lphy.RAGGED_DESC_DTYPE).tobytes()
             and {k: int(got_info[k]) for k in model.INFO_FIELDS} == want_info)
    tiles = W // lphy.FIND_TILE + 1
    out = {
        "device": torch.cuda.get_device_name(0), "sf": sf, "hop": N, "windows": W, "reps": a.reps, "warmup": a.warmup,
        "frames_found": int(got_info["frames"]), "active_windows": int(got_info["active"]),
        "table_equals_model": bool(equal),
        "bytes_per_pass": {
            "k_find_flags": {"read": W * 16, "written": tiles * 16 * 8 + tiles * 12},
            "k_find_carry": {"read": tiles * 12, "written": tiles * 8},
            "k_find_count": {"read": tiles * (16 * 8 + 8), "written": tiles * 48},
            "k_find_offsets": {"read": tiles * 48, "written": tiles * 32 + 32 + 64},
            "k_find_write": {"read": tiles * (16 * 8 + 8 + 32 + 48), "written": int(got_info["frames"]) * 32},
            "k_find_pad": {"read": 64, "written": (max_frames + 1 - int(got_info["frames"])) * 32},
            "detect_batch": {"read": W * N * 8, "written": W * 16},
        },
        "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
    }
    out["find_over_detect"] = out["ms"]["find_frames"]["median"] / out["ms"]["detect_batch"]["median"]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["ms"]), "find/detect", out["find_over_detect"], "equal", equal)
    d.close()
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
