#!/usr/bin/env python3
"""Times lphy_hip_channelize on a wideband capture of 2^26 samples by default
(512 MiB of IQ): 8 channels at decimation 16 with 65 and 129 taps, one channel
at decimation 8 with 65 taps, and beside them the consumer, lphy_hip_detect_batch
(SF 7, hop = N, dechirp) over the eight streams the 65-tap call produced.
Device events around each call, warm, the calls alternating in one loop.  Next
to every median: the time to read the input once and write the outputs at
8 TB/s, and the VALU bound of the complex multiply-accumulates (8 float32
operations each, none fused, 256 CUs x 4 SIMDs x 32 lanes a clock at 2.4 GHz).
Every timed shape's first and last tile are compared with the numpy model.
Writes profiles/channelize/bench.json.  Needs a HIP device.

  python tools/channelize_bench.py [--log2-samples 26] [--reps 20] [--warmup 3] [--out PATH]

With --format (all, or one of sc16, sc8, cu8) it times the sample formats of
lphy_hip_channelize_raw instead and writes profiles/channelize/bench_formats.json:
the same three shapes, lphy_hip_channelize on a float32 capture and
lphy_hip_channelize_raw on integer captures of the same length alternating in
one loop, so that the float32 number is taken in the same session; and the
host forms on the first shape, cut to 2^--host-log2-samples samples: wall time
of channelize_host and channelize_raw_host, whose uploads are 1, 1/2 and 1/4.
Every timed (shape, format) is first compared, first and last tile, with the
numpy model on the converted capture.

  python tools/channelize_bench.py --format all [--host-log2-samples 22] [--reps 20] [--warmup 3]
"""
import argparse
import json
import statistics
import sys
from fractions import Fraction as F
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "lora-sdr-lightweight-standalone-library-clean_amd"))
sys.path.insert(0, str(ROOT / "tests"))

HBM_BYTES_PER_S = 8.0e12
VALU_OPS_PER_S = 256 * 4 * 32 * 2.4e9   # one non-fused float32 operation per lane and clock
SHAPES = [("c8_d16_t65", 8, 16, 65), ("c8_d16_t129", 8, 16, 129), ("c1_d8_t65", 1, 8, 65)]


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def formats_main(a):
    """--format: lphy_hip_channelize against lphy_hip_channelize_raw, device and host forms."""
    import time

    import torch

    import channelize_model as model
    import lphy
    import sample_formats as sf
    assert torch.cuda.is_available(), "needs a HIP device"
    ids = {"sc16": sf.FMT_SC16, "sc8": sf.FMT_SC8, "cu8": sf.FMT_CU8}
    fmts = list(ids.values()) if a.format == "all" else [ids[a.format]]
    tdt = {sf.FMT_SC16: torch.int16, sf.FMT_SC8: torch.int8, sf.FMT_CU8: torch.uint8}
    n_in = 1 << a.log2_samples
    dev = torch.device("cuda:0")
    d = lphy.Demodulator(7)
    g = torch.Generator(device=dev).manual_seed(11)
    st = torch.cuda.current_stream().cuda_stream
    K = lphy.CHAN_TILE
    # the captures: float32 as the plain bench makes it, the integers over their whole range
    caps = {sf.FMT_CF32: torch.randn(2 * n_in, generator=g, device=dev, dtype=torch.float32)}
    for f in fmts:
        info = np.iinfo(sf.DTYPES[f])
        caps[f] = torch.randint(int(info.min), int(info.max) + 1, (2 * n_in,), generator=g, device=dev, dtype=tdt[f])

    def tiles_equal(x, f, taps, rot, D, T, n_out, t_out):
        ch = taps.shape[0]
        got = t_out.cpu().numpy().view(np.complex64).reshape(ch, n_out)
        m0 = (n_out - 1) // K * K
        head = sf.to_float(x[: 2 * ((K - 1) * D + T)].cpu().numpy(), f)
        tail = sf.to_float(x[2 * m0 * D: 2 * ((n_out - 1) * D + T)].cpu().numpy(), f)
        first = model.channelize(head, taps, rot, D, 0, K, 0)
        last = model.channelize(tail, taps, rot, D, 0, n_out - m0, m0)
        return bool(np.array_equal(got[:, :K].view(np.uint8), first.view(np.uint8))
                    and np.array_equal(got[:, m0:].view(np.uint8), last.view(np.uint8)))

    def device_call(f, plan, t_taps, t_rot, t_out):
        if f == sf.FMT_CF32:   # the float32 entry point itself
            return lambda: d.channelize(caps[f], plan, t_taps, t_rot, t_out, stream=st)
        return lambda: d.channelize_raw(caps[f], f, plan, t_taps, t_rot, t_out, stream=st)

    def host_call(f, x, taps, rot, D, n_out, out):
        if f == sf.FMT_CF32:
            return lambda: d.channelize_host(x.view(np.complex64), taps, rot, D, outputs=n_out, out=out)
        return lambda: d.channelize_raw_host(x, f, taps, rot, D, outputs=n_out, out=out)

    calls, shapes, equal = [], {}, True
    for name, ch, D, T in SHAPES:
        centres = [F(2 * c - ch + 1, 2 * ch * 5) for c in range(ch)]
        taps, rot, R, _ = lphy.chan_design(centres, D, T, 0.4 / D, 8.0)
        n_out = lphy.channelize_outputs(n_in, 0, T, D)
        t_taps = torch.from_numpy(taps.view(np.float32).copy()).to(dev)
        t_rot = torch.from_numpy(rot.view(np.float32).copy()).to(dev)
        t_out = torch.zeros(2 * ch * n_out, dtype=torch.float32, device=dev)
        plan = lphy.chan_plan(0, n_in, n_out, n_out, 0, ch, T, D, R)
        shapes[name] = {"channels": ch, "decim": D, "taps": T, "rot_period": R, "in_samples": n_in, "outputs": n_out,
                        "formats": {}}
        for f in [sf.FMT_CF32] + fmts:
            fn = device_call(f, plan, t_taps, t_rot, t_out)
            fn()
            torch.cuda.synchronize()
            ok = tiles_equal(caps[f], f, taps, rot, D, T, n_out, t_out)
            equal = equal and ok
            shapes[name]["formats"][sf.NAMES[f]] = {"sample_bytes": sf.BYTES[f], "tiles_equal_model": ok,
                                                    "bytes_moved": sf.BYTES[f] * n_in + 8 * ch * n_out}
            calls.append((name, sf.NAMES[f], fn))
    times = {(s, f): [] for s, f, _ in calls}
    for i in range(a.warmup + a.reps):
        for s, f, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[(s, f)].append(e0.elapsed_time(e1))
    for (s, f), v in times.items():
        shapes[s]["formats"][f]["ms"] = summary(v)
    for s in shapes.values():
        base = s["formats"]["cf32"]["ms"]
        s["cf32_spread_ms"] = base["max"] - base["min"]
        for f, r in s["formats"].items():
            r["median_over_cf32"] = r["ms"]["median"] / base["median"]
            r["slower_than_cf32_by_more_than_its_spread"] = bool(r["ms"]["median"] - base["median"]
                                                                 > s["cf32_spread_ms"])

    # the host forms: wall time of one call, the first shape on a shorter capture
    name, ch, D, T = SHAPES[0]
    n_host = 1 << a.host_log2_samples
    centres = [F(2 * c - ch + 1, 2 * ch * 5) for c in range(ch)]
    taps, rot, R, _ = lphy.chan_design(centres, D, T, 0.4 / D, 8.0)
    n_out = lphy.channelize_outputs(n_host, 0, T, D)
    out = np.zeros((ch, n_out), np.complex64)
    h_caps = {f: caps[f][: 2 * n_host].cpu().numpy() for f in caps}
    h_calls = [(f, host_call(f, h_caps[f], taps, rot, D, n_out, out)) for f in [sf.FMT_CF32] + fmts]
    h_times = {f: [] for f, _ in h_calls}
    h_equal = {}
    for i in range(a.warmup + a.reps):
        for f, fn in h_calls:
            t0 = time.perf_counter()
            got = fn()
            t1 = time.perf_counter()
            if i >= a.warmup:
                h_times[f].append(1e3 * (t1 - t0))
            if i == 0:
                want = model.channelize(sf.to_float(h_caps[f][: 2 * ((K - 1) * D + T)], f), taps, rot, D, 0, K, 0)
                h_equal[f] = bool(np.array_equal(got[:, :K].view(np.uint8), want.view(np.uint8)))
                equal = equal and h_equal[f]
    span = (n_out - 1) * D + T
    host = {"shape": name, "in_samples": n_host, "outputs": n_out, "out_bytes_each_way": 8 * ch * n_out, "formats": {}}
    base = statistics.median(h_times[sf.FMT_CF32])
    for f, v in h_times.items():
        up = sf.BYTES[f] * span
        host["formats"][sf.NAMES[f]] = {
            "sample_bytes": sf.BYTES[f], "first_tile_equals_model": h_equal[f], "ms": summary(v),
            "upload_bytes": up, "upload_over_cf32": sf.BYTES[f] / 8, "median_over_cf32": statistics.median(v) / base,
            "bytes_both_ways": up + 2 * 8 * ch * n_out + 8 * ch * (T + R),
            "capture_bytes_per_s_of_wall_time": up / (statistics.median(v) * 1e-3)}
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "method": "device: events around each call, warm, all calls alternating in one loop; "
                     "host: perf_counter around each synchronous call, pageable arrays, alternating",
           "shapes": shapes, "host_form": host}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({s: {f: r["ms"]["median"] for f, r in v["formats"].items()} for s, v in shapes.items()}),
          "host", json.dumps({f: r["ms"]["median"] for f, r in host["formats"].items()}), "equal", equal)
    d.close()
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=26)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--format", choices=["all", "sc16", "sc8", "cu8"], default=None)
    ap.add_argument("--host-log2-samples", type=int, default=22)
    a = ap.parse_args()
    if a.format:
        a.out = a.out or str(ROOT / "profiles" / "channelize" / "bench_formats.json")
        return formats_main(a)
    a.out = a.out or str(ROOT / "profiles" / "channelize" / "bench.json")
    import torch

    import channelize_model as model
    import lphy
    assert torch.cuda.is_available(), "needs a HIP device"
    sf, N = 7, 128
    n_in = 1 << a.log2_samples
    dev = torch.device("cuda:0")
    d = lphy.Demodulator(sf)
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn(2 * n_in, generator=g, device=dev, dtype=torch.float32)
    st = torch.cuda.current_stream().cuda_stream
    K = lphy.CHAN_TILE

    calls, shapes, checks = [], {}, {}
    for name, ch, D, T in SHAPES:
        centres = [F(2 * c - ch + 1, 2 * ch * 5) for c in range(ch)]    # centres 1/40 of a cycle apart: R = 5 at D = 16
        taps, rot, R, _ = lphy.chan_design(centres, D, T, 0.4 / D, 8.0)
        n_out = lphy.channelize_outputs(n_in, 0, T, D)
        t_taps = torch.from_numpy(taps.view(np.float32).copy()).to(dev)
        t_rot = torch.from_numpy(rot.view(np.float32).copy()).to(dev)
        t_out = torch.zeros(2 * ch * n_out, dtype=torch.float32, device=dev)
        plan = lphy.chan_plan(0, n_in, n_out, n_out, 0, ch, T, D, R)
        calls.append((name, lambda p=plan, tt=t_taps, tr=t_rot, to=t_out: d.channelize(x, p, tt, tr, to, stream=st)))
        macs = n_out * ch * T
        nbytes = 8 * (n_in + ch * n_out)
        shapes[name] = {"channels": ch, "decim": D, "taps": T, "rot_period": R, "in_samples": n_in, "outputs": n_out,
                        "complex_macs": macs, "bytes_moved": nbytes,
                        "hbm_bound_ms": 1e3 * nbytes / HBM_BYTES_PER_S,
                        "valu_bound_ms": 1e3 * 8 * macs / VALU_OPS_PER_S}
        checks[name] = (taps, rot, D, T, n_out, t_out)
    # the consumer: the detector over the eight streams of the first shape
    ch0, n_out0, streams = SHAPES[0][1], shapes[SHAPES[0][0]]["outputs"], checks[SHAPES[0][0]][5]
    windows = n_out0 // N
    rec = torch.zeros(ch0 * windows * 16, dtype=torch.uint8, device=dev)

    def detect():
        for c in range(ch0):
            d.detect_batch(streams[2 * c * n_out0: 2 * (c + 1) * n_out0], n_out0, 0, N, 1, windows,
                           rec[c * windows * 16: (c + 1) * windows * 16], lphy.DET_DECHIRP, stream=st)

    calls.append(("detect_batch_8_streams", detect))
    times = {name: [] for name, _ in calls}
    for i in range(a.warmup + a.reps):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    # the first and the last tile of every shape against the definition
    equal = True
    for name, (taps, rot, D, T, n_out, t_out) in checks.items():
        ch = taps.shape[0]
        got = t_out.cpu().numpy().view(np.complex64).reshape(ch, n_out)
        head = x[: 2 * ((K - 1) * D + T)].cpu().numpy().view(np.complex64)
        m0 = (n_out - 1) // K * K
        tail = x[2 * m0 * D: 2 * ((n_out - 1) * D + T)].cpu().numpy().view(np.complex64)
        ok = (np.array_equal(got[:, :K].view(np.uint8), model.channelize(head, taps, rot, D, 0, K, 0).view(np.uint8))
              and np.array_equal(got[:, m0:].view(np.uint8),
                                 model.channelize(tail, taps, rot, D, 0, n_out - m0, m0).view(np.uint8)))
        shapes[name]["tiles_equal_model"] = bool(ok)
        equal = equal and ok
    ms = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
    for name in shapes:
        s, med = shapes[name], ms[name]["median"]
        s["ms"] = ms[name]
        s["median_over_hbm_bound"] = med / s["hbm_bound_ms"]
        s["median_over_valu_bound"] = med / s["valu_bound_ms"]
        s["input_samples_per_s"] = n_in / (med * 1e-3)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "assumed": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "valu_f32_ops_per_s": VALU_OPS_PER_S,
                       "ops_per_complex_mac": 8},
           "shapes": shapes,
           "detect_batch_8_streams": {"sf": sf, "windows_per_stream": windows, "streams": ch0,
                                      "ms": ms["detect_batch_8_streams"]},
           "channelize_over_detect": ms[SHAPES[0][0]]["median"] / ms["detect_batch_8_streams"]["median"]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(ms), "channelize/detect", out["channelize_over_detect"], "equal", equal)
    d.close()
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
