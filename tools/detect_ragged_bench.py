#!/usr/bin/env python3
"""lphy_hip_detect_ragged against the uniform detector call of the parent
commit, same box, same process.

Shapes: SF 7 x 65,536 frames and SF 12 x 4,096 frames of 66 symbols, each
with LPHY_DET_DECHIRP; per shape
  ragged_uniform  detect_ragged on a table of equal lengths (ragged_layout)
  ragged_mixed    detect_ragged on frames of 8 and 66 symbols in turn, back to
                  back, with a last frame that brings the total to the same
                  number of symbols
  uniform         detect_batch of this tree on the same windows (first 0,
                  hop N, step 1)
  parent_uniform  detect_batch of the library given with --parent-lib (the
                  parent commit's build: the yardstick)
The work is the same in the four (one transform per symbol); the ragged form
also reads its table, 32 B per frame.

HIP events around each call, warm-up runs, then timed repetitions with the
variants alternating; medians and min-max.  Before timing, the records of the
four are compared byte for byte (outputs_equal; the mixed table covers the
same symbols in the same order, so its records are the same too).

The bar for the two ragged medians: the yardstick's median times
(1 + table bytes / IQ bytes + the yardstick's own (max - min) / median in this
run); `bar` and `within_bar` per variant.

    python tools/detect_ragged_bench.py --parent-lib PATH/liblphy_hip.so \\
        --out profiles/detect_ragged/bench.json
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "lora-sdr-lightweight-standalone-library-clean_amd"))
import lphy  # noqa: E402

SHAPES = [(7, 65536), (12, 4096)]
SYMBOLS, LO = 66, 8


class ParentDetector:
    """lphy_hip_detect_batch of another build of the library, which need not
    have this tree's newer entry points (lphy.load binds them all)."""

    def __init__(self, path, sf):
        import ctypes as C
        self.lib = C.CDLL(str(path))
        vp, sz = C.c_void_p, C.c_size_t
        self.lib.lphy_hip_ctx_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_int]
        self.lib.lphy_hip_ctx_destroy.argtypes = [vp]
        self.lib.lphy_hip_ctx_destroy.restype = None
        self.lib.lphy_hip_detect_batch.argtypes = [vp, vp, sz, sz, sz, sz, sz, vp, C.c_uint, vp]
        self.ctx = vp()
        rc = self.lib.lphy_hip_ctx_create(C.byref(self.ctx), 0, sf, 125000, 1, lphy.WINDOW_NONE)
        assert rc == 0, f"parent lphy_hip_ctx_create: {rc}"

    def detect_batch(self, iq, total_samples, first, hop, step, windows, out, flags, stream=None):
        rc = self.lib.lphy_hip_detect_batch(self.ctx, iq.data_ptr(), total_samples, first, hop, step, windows,
                                            out.data_ptr(), flags, stream)
        assert rc == 0, f"parent lphy_hip_detect_batch: {rc}"

    def close(self):
        self.lib.lphy_hip_ctx_destroy(self.ctx)


def mixed_lengths(total_symbols):
    """8 and 66 symbols in turn, then what is left of total_symbols in one frame."""
    pairs = total_symbols // (LO + SYMBOLS)
    lens = [LO, SYMBOLS] * pairs
    rest = total_symbols - pairs * (LO + SYMBOLS)
    return lens + ([rest] if rest else [])


def bench_shape(sf, frames, parent_lib, reps, warmup):
    dev = torch.device("cuda:0")
    N = 1 << sf
    fs = SYMBOLS * N
    units = frames * SYMBOLS
    total = units * N
    d = lphy.Demodulator(sf)
    p = ParentDetector(parent_lib, sf) if parent_lib else None
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev).manual_seed(11 + sf)
    iq = torch.randn(total * 2, dtype=torch.float32, device=dev, generator=gen)
    tables = {"uniform": d.ragged_layout([fs] * frames, lphy.MODE_DEMODULATE),
              "mixed": d.ragged_layout(np.array(mixed_lengths(units), np.uint64) * N, lphy.MODE_DEMODULATE)}
    for t in tables.values():
        assert int(t["unit_offset"][-1]) == units and int(t["iq_offset"][-1]) == total
    t_desc = {k: torch.from_numpy(v.view(np.uint8).copy()).to(dev) for k, v in tables.items()}
    nframes = {k: v.size - 1 for k, v in tables.items()}
    out = {k: torch.zeros(units * 16, dtype=torch.uint8, device=dev)
           for k in ("ragged_uniform", "ragged_mixed", "uniform", "parent_uniform")}
    fl = lphy.DET_DECHIRP
    variants = [
        ("ragged_uniform", lambda: d.detect_ragged(iq, t_desc["uniform"], nframes["uniform"], out["ragged_uniform"], 0,
                                                   fl, stream=st, iq_samples=total, units=units)),
        ("ragged_mixed", lambda: d.detect_ragged(iq, t_desc["mixed"], nframes["mixed"], out["ragged_mixed"], 0, fl,
                                                 stream=st, iq_samples=total, units=units)),
        ("uniform", lambda: d.detect_batch(iq, total, 0, N, 1, units, out["uniform"], fl, stream=st)),
    ]
    if p:
        variants.append(("parent_uniform",
                         lambda: p.detect_batch(iq, total, 0, N, 1, units, out["parent_uniform"], fl, stream=st)))
    # the results first
    for o in out.values():
        o.fill_(0xA5)
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    names = [name for name, _ in variants]
    equal = all(torch.equal(out[names[0]], out[name]) for name in names[1:])
    assert equal, f"SF {sf}: the records of the variants differ"
    walked = d.detect_serial_count()

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
    times = {name: [] for name in names}
    for _ in range(reps):
        for name, fn in variants:
            times[name].append(timed(fn))
    res = {"sf": sf, "frames": frames, "frame_samples": fs, "symbols": units, "iq_bytes": total * 8,
           "table_bytes": {k: (n + 1) * 32 for k, n in nframes.items()}, "mixed_frames": nframes["mixed"],
           "serial_walks_this_tree": walked, "outputs_equal": bool(equal), "variants": {}}
    for name, t in times.items():
        med = float(np.median(t))
        res["variants"][name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t),
                                 "ns_per_symbol": med * 1e6 / units}
    res["yardstick"] = "parent_uniform" if p else "uniform"
    y = res["variants"][res["yardstick"]]
    spread = (y["max_ms"] - y["min_ms"]) / y["median_ms"]
    res["yardstick_spread"] = spread
    for name, v in res["variants"].items():
        v["time_over_yardstick"] = v["median_ms"] / y["median_ms"]
        if name.startswith("ragged_"):
            v["bar"] = 1.0 + res["table_bytes"][name[len("ragged_"):]] / res["iq_bytes"] + spread
            v["within_bar"] = bool(v["time_over_yardstick"] <= v["bar"])
    print(json.dumps(res))
    d.close()
    if p:
        p.close()
    del iq, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="", help="liblphy_hip.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("detect_ragged_bench: no HIP device")
    if a.parent_lib and not Path(a.parent_lib).exists():
        sys.exit(f"detect_ragged_bench: {a.parent_lib} missing")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "parent_lib": bool(a.parent_lib), "symbols_per_frame": SYMBOLS, "mixed_symbols": [LO, SYMBOLS],
           "flags": "LPHY_DET_DECHIRP", "shapes": []}
    for sf, frames in SHAPES:
        res["shapes"].append(bench_shape(sf, frames, a.parent_lib, a.reps, a.warmup))
    res["outputs_equal"] = all(s["outputs_equal"] for s in res["shapes"])
    res["within_bar"] = all(v.get("within_bar", True) for s in res["shapes"] for v in s["variants"].values())
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
