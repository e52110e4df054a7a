#!/usr/bin/env python3
"""lphy_hip_lorawan_crypt_batch at several group widths G (the lanes that share
one range, csrc/lphy_lorawan.hip: LPHY_LW_CRYPT_G) against
lphy_hip_lorawan_mic_batch of the parent commit on the same jobs, same box, same
process.

    python tools/lorawan_crypt_bench.py build --parent-src DIR 1 2 4 8 16
        compiles csrc/lphy_lorawan.hip alone, once per G, into
        tools/ab_lib/lw_crypt_g<G>.so, and DIR's copy of it (a checkout of the
        parent commit) into tools/ab_lib/lw_parent.so; needs no device
    python tools/lorawan_crypt_bench.py run --chosen G --out profiles/lorawan_crypt/bench.json
        times what `build` left, on the device

Jobs: 65,536 ranges of 16 bytes and of 242 bytes (the largest LoRaWAN payload:
1 and 16 keystream blocks), byte-adjacent from offset 1, so every range starts
at an odd address; 1,024 keys.  The yardstick computes a CMAC over the same
ranges: the same number of AES blocks per job plus two, one after the other in
one thread.

HIP events around each launch, 3 warm-up rounds, then 20 timed rounds with the
variants alternating; medians and min-max.  Before timing, every variant
ciphers the buffer once (all must give the same bytes, and a sample of ranges is
checked against the CPU oracle's AES when it is built) and once more (the buffer
must be restored).

The expectation on record: the chosen G's median does not exceed the
yardstick's median by more than the yardstick's own max - min in this run
(`bar_ms`, `within_bar` per variant and size)."""
import argparse
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "lora-sdr-lightweight-standalone-library-clean_amd"
AB = ROOT / "tools" / "ab_lib"
sys.path.insert(0, str(PKG))
sys.path.insert(0, str(ROOT / "tests"))

JOBS, NKEYS, SIZES = 65536, 1024, (16, 242)
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared"]


def build(a):
    AB.mkdir(parents=True, exist_ok=True)
    procs = []
    for g in a.g:
        cmd = [HIPCC, *FLAGS, f"-DLPHY_LW_CRYPT_G={g}", f"-I{ROOT}/include", f"-I{PKG}/csrc", "-o",
               str(AB / f"lw_crypt_g{g}.so"), str(PKG / "csrc" / "lphy_lorawan.hip")]
        procs.append((f"G={g}", subprocess.Popen(cmd)))
    if a.parent_src:
        src = Path(a.parent_src)
        pkg = src / PKG.name
        cmd = [HIPCC, *FLAGS, f"-I{src}/include", f"-I{pkg}/csrc", "-o", str(AB / "lw_parent.so"),
               str(pkg / "csrc" / "lphy_lorawan.hip")]
        procs.append(("parent", subprocess.Popen(cmd)))
    for name, p in procs:
        if p.wait() != 0:
            sys.exit(f"lorawan_crypt_bench: building {name} failed")
        print("built", name)


def _lib(path):
    vp, sz = C.c_void_p, C.c_size_t
    L = C.CDLL(str(path))
    L.lphy_hip_lorawan_mic_batch.argtypes = [vp, vp, sz, vp, sz, vp, C.c_uint, vp]
    if hasattr(L, "lphy_hip_lorawan_crypt_batch"):
        L.lphy_hip_lorawan_crypt_batch.argtypes = [vp, vp, sz, vp, sz, vp, vp]
    return L


def bench_size(torch, lphy, size, variants, parent, reps, warmup):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7 + size)
    jobs = np.zeros(JOBS, lphy.LORAWAN_DESC_DTYPE)
    jobs["offset"], jobs["len"] = 1 + np.arange(JOBS, dtype=np.uint64) * size, size
    jobs["devaddr"] = rng.integers(0, 2 ** 32, JOBS, dtype=np.uint64)
    jobs["fcnt"] = rng.integers(0, 2 ** 32, JOBS, dtype=np.uint64)
    jobs["key"], jobs["uplink"] = rng.integers(0, NKEYS, JOBS), rng.integers(0, 2, JOBS)
    keys = rng.integers(0, 256, (NKEYS, 16), dtype=np.uint8)
    plain = rng.integers(0, 256, 1 + JOBS * size + 7, dtype=np.uint8)
    t_plain = torch.from_numpy(plain).to(dev)
    t_buf = t_plain.clone()
    t_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    t_keys = torch.from_numpy(keys.reshape(-1).copy()).to(dev)
    t_status = torch.zeros(JOBS, dtype=torch.int32, device=dev)
    t_mic = torch.zeros(JOBS, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def crypt(L):
        def fn():
            rc = L.lphy_hip_lorawan_crypt_batch(t_buf.data_ptr(), t_jobs.data_ptr(), JOBS, t_keys.data_ptr(), NKEYS,
                                                t_status.data_ptr(), st)
            assert rc == 0, rc
        return fn

    def mic():
        rc = parent.lphy_hip_lorawan_mic_batch(t_buf.data_ptr(), t_jobs.data_ptr(), JOBS, t_keys.data_ptr(), NKEYS,
                                               t_mic.data_ptr(), 0, st)
        assert rc == 0, rc

    calls = [(name, crypt(L)) for name, L in variants] + [("parent_mic_batch", mic)]
    # the results first: one pass ciphers, the next restores; all variants agree
    first = None
    for name, fn in calls[:-1]:
        fn()
        torch.cuda.synchronize()
        assert not t_status.any(), name
        out = t_buf.clone()
        first = out if first is None else first
        assert torch.equal(out, first), f"{name}: bytes differ from {calls[0][0]}"
        fn()
        torch.cuda.synchronize()
        assert torch.equal(t_buf, t_plain), f"{name}: the second pass does not restore the buffer"
    checked = 0
    try:
        from lorawan_crypt_model import Cipher
        from checkers import Oracle
        cipher, got = Cipher(Oracle()), first.cpu().numpy()
        for j in range(0, JOBS, 4099):
            o = int(jobs["offset"][j])
            want = plain[o:o + size] ^ cipher.keystream(keys[jobs["key"][j]], bool(jobs["uplink"][j]),
                                                        int(jobs["devaddr"][j]), int(jobs["fcnt"][j]), size)
            assert np.array_equal(got[o:o + size], want), j
            checked += 1
    except (ImportError, OSError, FileNotFoundError) as e:
        print(f"oracle check skipped: {e}", file=sys.stderr)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        for _, fn in calls:
            timed(fn)
    times = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            times[name].append(timed(fn))
    # an even number of passes per variant: the buffer is the plaintext again
    if (warmup + reps) % 2 == 0:
        assert torch.equal(t_buf, t_plain)
    res = {"range_bytes": size, "jobs": JOBS, "keys": NKEYS, "buffer_bytes": int(plain.size),
           "keystream_blocks_per_job": (size + 15) // 16, "yardstick_aes_blocks_per_job": (size + 15) // 16 + 2,
           "outputs_equal": True, "ranges_checked_against_oracle": checked, "variants": {}}
    for name, t in times.items():
        res["variants"][name] = {"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t)}
    y = res["variants"]["parent_mic_batch"]
    res["yardstick"] = "parent_mic_batch"
    res["yardstick_spread_ms"] = y["max_ms"] - y["min_ms"]
    res["yardstick_spread"] = (y["max_ms"] - y["min_ms"]) / y["median_ms"]
    for name, v in res["variants"].items():
        v["time_over_yardstick"] = v["median_ms"] / y["median_ms"]
        if name != "parent_mic_batch":
            v["bar_ms"] = y["median_ms"] + res["yardstick_spread_ms"]
            v["within_bar"] = bool(v["median_ms"] <= v["bar_ms"])
    print(json.dumps(res))
    return res


def run(a):
    import torch
    import lphy
    if not torch.cuda.is_available():
        sys.exit("lorawan_crypt_bench: no HIP device")
    parent_path = AB / "lw_parent.so"
    if not parent_path.exists():
        sys.exit(f"lorawan_crypt_bench: {parent_path} missing (build --parent-src)")
    gs = sorted(int(p.stem.rsplit("g", 1)[1]) for p in AB.glob("lw_crypt_g*.so"))
    if not gs:
        sys.exit("lorawan_crypt_bench: no tools/ab_lib/lw_crypt_g*.so (build first)")
    variants = [(f"G{g}", _lib(AB / f"lw_crypt_g{g}.so")) for g in gs]
    product = lphy.DEFAULT_SO
    if product.exists():
        variants.append(("product", _lib(product)))
    parent = _lib(parent_path)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "groups_tried": gs,
           "chosen": f"G{a.chosen}", "sizes": []}
    for size in SIZES:
        res["sizes"].append(bench_size(torch, lphy, size, variants, parent, a.reps, a.warmup))
    res["chosen_within_bar"] = all(s["variants"][res["chosen"]]["within_bar"] for s in res["sizes"])
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    b = sub.add_parser("build")
    b.add_argument("--parent-src", default="", help="a checkout of the parent commit")
    b.add_argument("g", nargs="+", type=int)
    r = sub.add_parser("run")
    r.add_argument("--out", default="")
    r.add_argument("--chosen", type=int, required=True, help="the G the library is built with")
    r.add_argument("--reps", type=int, default=20)
    r.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    (build if a.what == "build" else run)(a)


if __name__ == "__main__":
    main()
