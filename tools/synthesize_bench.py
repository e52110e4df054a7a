#!/usr/bin/env python3
"""Times lphy_hip_synthesize on 2^26 wideband outputs by default (512 MiB of
IQ written): 8 channels at interpolation 16 with 129 and 257 taps, one channel
at interpolation 8 with 65 taps, and beside each its mirror, lphy_hip_channelize
with the same channels, decimation and taps over a capture of as many samples,
in the same loop (boxes differ by a few percent, so the two ratios come from one
session).  Device events around each call, warm, the calls alternating in one
loop.  Next to every median: the time to read the inputs once and write the
outputs at 8 TB/s, and the VALU bound of the complex multiply-accumulates (8
float32 operations each, none fused, 256 CUs x 4 SIMDs x 32 lanes a clock at
2.4 GHz; the synthesiser has ceil(T / U) of them per channel and output, less
where a phase has one tap fewer).  Every synthesiser shape's first and last
tile are compared with the numpy model.  Writes profiles/synthesize/bench.json.
Needs a HIP device.

  python tools/synthesize_bench.py [--log2-outputs 26] [--reps 20] [--warmup 3] [--out PATH]

  python tools/synthesize_bench.py --codeobj [--out PATH]
compiles csrc/lphy_hip.hip for the device alone with the product flags and
writes the registers, LDS and scratch of every k_synth instance, from the
compiler's resource-usage remarks, to profiles/synthesize/codeobj.json.  Needs
hipcc, no device.
"""
import argparse
import json
import re
import statistics
import subprocess
import sys
import tempfile
from fractions import Fraction as F
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "lora-sdr-lightweight-standalone-library-clean_amd"
sys.path.insert(0, str(PKG))
sys.path.insert(0, str(ROOT / "tests"))

HBM_BYTES_PER_S = 8.0e12
VALU_OPS_PER_S = 256 * 4 * 32 * 2.4e9   # one non-fused float32 operation per lane and clock
SGPR_SPILL_ALLOWED = {"k_synth<8, true>": 4}
SHAPES = [("c8_u16_t129", 8, 16, 129), ("c8_u16_t257", 8, 16, 257), ("c1_u8_t65", 1, 8, 65)]


def codeobj(out):
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC",
             "-I", str(ROOT / "include")]
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["hipcc", *flags, "--offload-device-only", "--no-gpu-bundle-output",
                            "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(Path(tmp) / "lphy_hip.co"),
                            str(PKG / "csrc" / "lphy_hip.hip")], capture_output=True, text=True, check=True)
    kernels = {}
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    for blk in blocks:
        m = re.match(r"\S*k_synthILi(\d)ELb(\d)E", blk)
        if not m:
            continue

        def field(name):
            return int(re.search(r"remark:\s+" + re.escape(name) + r": (\d+)", blk).group(1))
        kernels[f"k_synth<{m.group(1)}, {'true' if m.group(2) == '1' else 'false'}>"] = {
            "vgpr": field("VGPRs"), "sgpr": field("TotalSGPRs"), "vgpr_spill": field("VGPRs Spill"),
            "sgpr_spill": field("SGPRs Spill"), "scratch": field("ScratchSize [bytes/lane]"),
            "lds": field("LDS Size [bytes/block]"), "waves_per_simd": field("Occupancy [waves/SIMD]")}
    assert len(kernels) == 7, sorted(kernels)   # CG 1, 2, 4, 8 on the LDS path; 2, 4, 8 on the global path
    doc = {"what": "gfx950 code object of lphy_hip.hip, product flags: the synthesiser's kernels k_synth<CG, LDS> "
                   "(hipcc -Rpass-analysis=kernel-resource-usage). lds is static; the LDS instances take up to 65536 "
                   "bytes of dynamic LDS per workgroup, by the plan (synth_lds_bytes). waves_per_simd is the "
                   "compiler's, by registers. There is no k_synth<1, false>: one channel's image always fits. "
                   "sgpr_spill counts SGPRs kept in VGPR lanes, not memory.",
           "kernels": kernels}
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(kernels))
    # The pass condition: no scratch and no spill of either kind in any instance, with one
    # exception stated here: k_synth<8, true> may keep up to SGPR_SPILL_ALLOWED SGPRs in VGPR
    # lanes (v_writelane / v_readlane outside the tap loop, register to register, no memory).
    bad = [n for n, k in kernels.items()
           if k["scratch"] or k["vgpr_spill"] or k["sgpr_spill"] > SGPR_SPILL_ALLOWED.get(n, 0)]
    if bad:
        print("spill or scratch in:", bad)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-outputs", type=int, default=26)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--codeobj", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.codeobj:
        return codeobj(a.out or str(ROOT / "profiles" / "synthesize" / "codeobj.json"))
    out_path = a.out or str(ROOT / "profiles" / "synthesize" / "bench.json")
    import torch

    import lphy
    import synthesize_model as model
    assert torch.cuda.is_available(), "needs a HIP device"
    n_wide = 1 << a.log2_outputs
    dev = torch.device("cuda:0")
    d = lphy.Demodulator(7)
    g = torch.Generator(device=dev).manual_seed(11)
    wide_in = torch.randn(2 * n_wide, generator=g, device=dev, dtype=torch.float32)   # the channeliser's capture
    st = torch.cuda.current_stream().cuda_stream
    K = lphy.SYNTH_TILE

    def up(x):
        return torch.from_numpy(x.view(np.float32).copy()).to(dev)

    calls, shapes, checks = [], {}, {}
    for name, ch, U, T in SHAPES:
        centres = [F(2 * c - ch + 1, 2 * ch * 5) for c in range(ch)]    # centres 1/40 of a cycle apart: R = 5 at U = 16
        taps, rot, R, _ = lphy.synth_design(centres, U, T, 0.4 / U, 8.0)
        n_in = n_wide // U
        assert lphy.synthesize_outputs(n_in, 0, T, U) >= n_wide - U
        x = torch.randn(2 * ch * n_in, generator=g, device=dev, dtype=torch.float32)
        t_taps, t_rot = up(taps), up(rot)
        t_out = torch.zeros(2 * n_wide, dtype=torch.float32, device=dev)
        plan = lphy.synth_plan(0, n_in, n_in, n_wide, 0, ch, T, U, R)
        calls.append((name, lambda p=plan, tx=x, tt=t_taps, tr=t_rot, to=t_out: d.synthesize(tx, p, tt, tr, to, stream=st)))
        chain = sum((T - 1 - p) // U + 1 for p in range(U) if p < T) / U    # multiply-accumulates per channel and output
        macs = n_wide * ch * chain
        nbytes = 8 * (ch * n_in + n_wide)
        shapes[name] = {"channels": ch, "interp": U, "taps": T, "rot_period": R, "in_samples": n_in, "outputs": n_wide,
                        "complex_macs": macs, "bytes_moved": nbytes, "hbm_bound_ms": 1e3 * nbytes / HBM_BYTES_PER_S,
                        "valu_bound_ms": 1e3 * 8 * macs / VALU_OPS_PER_S,
                        "valu_bound_ms_ceil": 1e3 * 8 * n_wide * ch * ((T - 1) // U + 1) / VALU_OPS_PER_S}
        checks[name] = (x, taps, rot, U, T, n_in, t_out)
        # the mirror: the channeliser with the same channels, decimation and taps
        ctaps, crot, cR, _ = lphy.chan_design(centres, U, T, 0.4 / U, 8.0)
        c_out_n = lphy.channelize_outputs(n_wide, 0, T, U)
        tc_taps, tc_rot = up(ctaps), up(crot)
        tc_out = torch.zeros(2 * ch * c_out_n, dtype=torch.float32, device=dev)
        cplan = lphy.chan_plan(0, n_wide, c_out_n, c_out_n, 0, ch, T, U, cR)
        calls.append(("chan_" + name, lambda p=cplan, tt=tc_taps, tr=tc_rot, to=tc_out: d.channelize(wide_in, p, tt, tr, to, stream=st)))
        shapes[name]["channelize"] = {"outputs": c_out_n, "complex_macs": c_out_n * ch * T,
                                      "valu_bound_ms": 1e3 * 8 * c_out_n * ch * T / VALU_OPS_PER_S}
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
    for name, (x, taps, rot, U, T, n_in, t_out) in checks.items():
        ch = taps.shape[0]
        xs = x.cpu().numpy().view(np.complex64).reshape(ch, n_in)
        got = t_out.cpu().numpy().view(np.complex64)
        w0 = n_wide - K
        j0 = max(0, w0 // U - (T - 1) // U)
        ok = (np.array_equal(got[:K].view(np.uint8),
                             model.synthesize(xs[:, : K // U + 1], taps, rot, U, 0, K, 0).view(np.uint8))
              and np.array_equal(got[w0:].view(np.uint8),
                                 model.synthesize(xs[:, j0:], taps, rot, U, w0 - j0 * U, K, j0).view(np.uint8)))
        shapes[name]["tiles_equal_model"] = bool(ok)
        equal = equal and ok
    ms = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
    for name in shapes:
        s, med = shapes[name], ms[name]["median"]
        s["ms"] = ms[name]
        s["median_over_hbm_bound"] = med / s["hbm_bound_ms"]
        s["median_over_valu_bound"] = med / s["valu_bound_ms"]
        s["median_over_valu_bound_ceil"] = med / s["valu_bound_ms_ceil"]
        s["outputs_per_s"] = n_wide / (med * 1e-3)
        c = s["channelize"]
        c["ms"] = ms["chan_" + name]
        c["median_over_valu_bound"] = c["ms"]["median"] / c["valu_bound_ms"]
        s["ratio_over_channelize_ratio"] = s["median_over_valu_bound_ceil"] / c["median_over_valu_bound"]
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "assumed": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "valu_f32_ops_per_s": VALU_OPS_PER_S,
                       "ops_per_complex_mac": 8},
           "shapes": shapes}
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: {"ms": v["ms"], "valu": v["median_over_valu_bound_ceil"],
                          "chan_ms": v["channelize"]["ms"], "chan_valu": v["channelize"]["median_over_valu_bound"]}
                      for k, v in shapes.items()}), "equal", equal)
    d.close()
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
