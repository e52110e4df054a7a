#!/usr/bin/env python3
"""Ragged call against the grouped loop it replaces, same box, same session.

Workload (mode 2 with LPHY_F_DECODE, fixed seed):
  SF 7:  65,536 frames, data symbols drawn uniformly from {8, 16, ..., 128}
  SF 12:  4,096 frames, data symbols from {4, 8, ..., 64}
(+ 2 sync symbols each).  Baseline: the frames grouped by length, one
lphy_hip_demod_batch per group with the default crossover, the whole loop
between two HIP events.  Candidate: one lphy_hip_demod_ragged on the frames
packed in arrival order.  5 warm-up runs, 20 timed repetitions each,
alternating, medians and the min-max spread.  Roofline fraction: algorithmic
bytes (IQ read once, symbols + bytes + records written once, summed over the
actual lengths) over the median time, against 8 TB/s.

    python tools/ubench/ragged_bench.py --out profiles/ragged/ragged_bench.json
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


def workload(sf, nframes, step, seed, dev):
    N = 1 << sf
    rng = np.random.default_rng(seed)
    data = rng.integers(1, 17, nframes) * step          # data symbols per frame
    d = lphy.Demodulator(sf)
    lengths = (data + 2) * N
    desc = d.ragged_layout(lengths, 2)
    packed = torch.empty(int(desc["iq_offset"][-1]), dtype=torch.complex64, device=dev)
    groups = []
    for n in np.unique(data):
        idx = np.nonzero(data == n)[0]
        syms = torch.from_numpy(rng.integers(0, N, (idx.size, int(n)), dtype=np.int64).astype(np.int16)).to(dev)
        iq = torch.empty((idx.size, int(n + 2) * N), dtype=torch.complex64, device=dev)
        d.modulate_batch(syms, idx.size, int(n), torch.view_as_real(iq))
        torch.cuda.synchronize()
        off = torch.from_numpy(desc["iq_offset"][idx].astype(np.int64)).to(dev)
        for k0 in range(0, idx.size, 512):  # scatter the group's frames to their packed places
            o = off[k0:k0 + 512]
            dst = (o[:, None] + torch.arange(iq.shape[1], device=dev)[None, :]).reshape(-1)
            packed[dst] = iq[k0:k0 + 512].reshape(-1)
        groups.append({"n": int(n), "frames": idx.size, "iq": iq,
                       "syms": torch.zeros(idx.size * int(n), dtype=torch.int16, device=dev),
                       "pay": torch.zeros(idx.size * int(n) // 2, dtype=torch.uint8, device=dev),
                       "meta": torch.zeros(idx.size * 32, dtype=torch.uint8, device=dev), "idx": idx})
    return d, data, desc, packed, groups


def run(sf, nframes, step, reps, warm):
    dev = torch.device("cuda:0")
    N = 1 << sf
    d, data, desc, packed, groups = workload(sf, nframes, step, 20260 + sf, dev)
    n_out = int(desc["sym_offset"][-1])
    t_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    r_syms = torch.zeros(n_out, dtype=torch.int16, device=dev)
    r_pay = torch.zeros(n_out // 2 + 1, dtype=torch.uint8, device=dev)
    r_meta = torch.zeros(nframes * 32, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    flags = lphy.F_DECODE

    def grouped():
        for g in groups:
            d.demod_batch(torch.view_as_real(g["iq"]), g["frames"], (g["n"] + 2) * N, g["syms"], g["meta"], 2, flags,
                          payload=g["pay"], stream=st)

    def ragged():
        d.demod_ragged(torch.view_as_real(packed), t_desc, nframes, r_syms, r_meta, 2, flags, payload=r_pay,
                       stream=st, iq_samples=packed.numel(), out_syms=n_out)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(warm):
        grouped()
        ragged()
    torch.cuda.synchronize()
    tg, tr = [], []
    for _ in range(reps):
        tg.append(timed(grouped))
        tr.append(timed(ragged))
    # same results: every frame's symbols, bytes and records
    rs = r_syms.cpu().numpy()
    rm = r_meta.cpu().numpy().reshape(nframes, 32)
    rp = r_pay.cpu().numpy()
    for g in groups:
        gs = g["syms"].cpu().numpy().reshape(g["frames"], g["n"])
        gp = g["pay"].cpu().numpy().reshape(g["frames"], g["n"] // 2)
        gm = g["meta"].cpu().numpy().reshape(g["frames"], 32)
        so = desc["sym_offset"][g["idx"]].astype(np.int64)
        assert np.array_equal(rs[so[:, None] + np.arange(g["n"])[None, :]], gs), "symbols differ"
        assert np.array_equal(rp[so[:, None] // 2 + np.arange(g["n"] // 2)[None, :]], gp), "bytes differ"
        assert np.array_equal(rm[g["idx"]], gm), "records differ"
    nbytes = int(((data + 2) * N * 8 + data * 2 + data // 2 + 32).sum())
    med = lambda v: float(np.median(v))
    out = {"sf": sf, "frames": nframes, "groups": len(groups), "data_symbols": int(data.sum()),
           "algorithmic_bytes": nbytes, "reps": reps, "warmup": warm,
           "grouped_ms": {"median": med(tg), "min": min(tg), "max": max(tg)},
           "ragged_ms": {"median": med(tr), "min": min(tr), "max": max(tr)},
           "grouped_roofline": nbytes / (med(tg) * 1e-3) / HBM, "ragged_roofline": nbytes / (med(tr) * 1e-3) / HBM,
           "ragged_over_grouped": med(tr) / med(tg), "outputs_equal": True}
    d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    res = [run(7, 65536, 8, a.reps, a.warmup), run(12, 4096, 4, a.reps, a.warmup)]
    for r in res:
        print(json.dumps(r))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": res}, indent=1) + "\n")


if __name__ == "__main__":
    main()
