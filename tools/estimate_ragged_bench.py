#!/usr/bin/env python3
"""lphy_hip_estimate_ragged against the uniform call of the parent commit,
same box, same process.

Shapes: SF 7 x 65,536 frames and SF 12 x 4,096 frames of 66 symbols, with
est_samples = 2 and 8 symbols; per shape
  ragged_uniform  estimate_ragged on a table of equal lengths (ragged_layout)
  ragged_mixed    estimate_ragged on the same number of frames with lengths
                  uniform in 8..66 symbols (fixed seed), frames back to back
  uniform         estimate_batch of this tree on the equal-length frames
  parent_uniform  estimate_batch of the library given with --parent-lib (the
                  parent commit's build: the yardstick)
The work is the same in the four (frames x est symbols transforms); the
ragged form also reads its table, 32 B per frame.

HIP events around each call, warm-up runs, then timed repetitions with the
variants alternating; medians and min-max.  Before timing, the ragged records
on the equal-length table are compared byte for byte with both uniform calls
(outputs_equal).

    python tools/estimate_ragged_bench.py --parent-lib PATH/liblphy_hip.so \\
        --out profiles/estimate_ragged/bench.json
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
EST_SYMBOLS = (2, 8)


class ParentEstimator:
    """lphy_hip_estimate_batch of another build of the library, which need not
    have this tree's newer entry points (lphy.load binds them all)."""

    def __init__(self, path, sf):
        import ctypes as C
        self.lib = C.CDLL(str(path))
        vp, sz = C.c_void_p, C.c_size_t
        self.lib.lphy_hip_ctx_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_int]
        self.lib.lphy_hip_ctx_destroy.argtypes = [vp]
        self.lib.lphy_hip_ctx_destroy.restype = None
        self.lib.lphy_hip_estimate_batch.argtypes = [vp, vp, sz, sz, sz, vp, vp]
        self.ctx = vp()
        rc = self.lib.lphy_hip_ctx_create(C.byref(self.ctx), 0, sf, 125000, 1, lphy.WINDOW_NONE)
        assert rc == 0, f"parent lphy_hip_ctx_create: {rc}"

    def estimate_batch(self, iq, frames, frame_samples, est_samples, meta, stream=None):
        rc = self.lib.lphy_hip_estimate_batch(self.ctx, iq.data_ptr(), frames, frame_samples, est_samples,
                                              meta.data_ptr(), stream)
        assert rc == 0, f"parent lphy_hip_estimate_batch: {rc}"

    def close(self):
        self.lib.lphy_hip_ctx_destroy(self.ctx)


def bench_shape(sf, frames, parent_lib, reps, warmup):
    dev = torch.device("cuda:0")
    N = 1 << sf
    fs = SYMBOLS * N
    d = lphy.Demodulator(sf)
    p = ParentEstimator(parent_lib, sf) if parent_lib else None
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev).manual_seed(7 + sf)
    iq = torch.randn(frames * fs * 2, dtype=torch.float32, device=dev, generator=gen)
    lens = np.random.default_rng(2026 + sf).integers(LO, SYMBOLS + 1, frames) * N
    tables = {"uniform": d.ragged_layout([fs] * frames, lphy.MODE_DEMODULATE),
              "mixed": d.ragged_layout(lens, lphy.MODE_DEMODULATE)}
    t_desc = {k: torch.from_numpy(v.view(np.uint8).copy()).to(dev) for k, v in tables.items()}
    extent = {k: int(v["iq_offset"][-1]) for k, v in tables.items()}
    meta = {k: torch.zeros(frames * 32, dtype=torch.uint8, device=dev)
            for k in ("ragged_uniform", "ragged_mixed", "uniform", "parent_uniform")}
    out = []
    for est_syms in EST_SYMBOLS:
        est = est_syms * N
        variants = [
            ("ragged_uniform", lambda: d.estimate_ragged(iq, t_desc["uniform"], frames, est, meta["ragged_uniform"],
                                                         stream=st, iq_samples=extent["uniform"])),
            ("ragged_mixed", lambda: d.estimate_ragged(iq, t_desc["mixed"], frames, est, meta["ragged_mixed"],
                                                       stream=st, iq_samples=extent["mixed"])),
            ("uniform", lambda: d.estimate_batch(iq, frames, fs, est, meta["uniform"], stream=st)),
        ]
        if p:
            variants.append(("parent_uniform",
                             lambda: p.estimate_batch(iq, frames, fs, est, meta["parent_uniform"], stream=st)))
        # the results first
        for m in meta.values():
            m.fill_(0xA5)
        for _, fn in variants:
            fn()
        torch.cuda.synchronize()
        equal = torch.equal(meta["ragged_uniform"], meta["uniform"])
        if p:
            equal = equal and torch.equal(meta["ragged_uniform"], meta["parent_uniform"])
        assert equal, f"SF {sf}, {est_syms} symbols: the ragged records differ from estimate_batch's"

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
        times = {name: [] for name, _ in variants}
        for _ in range(reps):
            for name, fn in variants:
                times[name].append(timed(fn))
        res = {"sf": sf, "frames": frames, "frame_samples": fs, "est_symbols": est_syms,
               "transforms": frames * est_syms, "table_bytes": frames * 32, "outputs_equal": bool(equal),
               "variants": {}}
        for name, t in times.items():
            med = float(np.median(t))
            res["variants"][name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t),
                                     "ns_per_transform": med * 1e6 / (frames * est_syms)}
        base = res["variants"].get("parent_uniform", res["variants"]["uniform"])["median_ms"]
        res["yardstick"] = "parent_uniform" if p else "uniform"
        for v in res["variants"].values():
            v["time_over_yardstick"] = v["median_ms"] / base
        print(json.dumps(res))
        out.append(res)
    d.close()
    if p:
        p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="", help="liblphy_hip.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("estimate_ragged_bench: no HIP device")
    if a.parent_lib and not Path(a.parent_lib).exists():
        sys.exit(f"estimate_ragged_bench: {a.parent_lib} missing")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "parent_lib": bool(a.parent_lib), "symbols_per_frame": SYMBOLS, "mixed_symbols": [LO, SYMBOLS],
           "shapes": []}
    for sf, frames in SHAPES:
        res["shapes"] += bench_shape(sf, frames, a.parent_lib, a.reps, a.warmup)
    res["outputs_equal"] = all(s["outputs_equal"] for s in res["shapes"])
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
