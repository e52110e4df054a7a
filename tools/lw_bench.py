"""Throughput of the LoRaWAN batch kernels (csrc/lphy_lorawan.hip) and the
codes kernels on one MI355X: frames/s for compute_mic (MIC append) and for
parse_frame's checks over decoded rows, HIP-event timed on one stream.
usage: python tools/lw_bench.py [frames] [row_bytes]
       python tools/lw_bench.py ragged [frames] [out.json]
The ragged case (default 65,536 frames of mixed lengths 12..64 bytes on one
lphy_ragged_desc table) times lphy_hip_lorawan_parse_ragged and
lphy_hip_lorawan_build_ragged against the routes without them (and, on its
own, lphy_hip_lorawan_crypt_rx_ragged over the rows the parse accepted):
  parse  a device gather of the packed bytes into padded rows (index and mask
         tensors made beforehand, a length array) + lphy_hip_lorawan_parse_batch;
  build  the frames' MHDR..FRMPayload assembled on the host (not timed), then
         the upload of those bytes and of one lphy_lorawan_desc per frame +
         lphy_hip_lorawan_mic_batch(LPHY_LW_APPEND), against the upload of one
         lphy_lorawan_tx per frame + the build kernel (payloads device-resident).
Each pair alternates in the same process, `rounds` times; the figures are the
medians, with the extremes next to them."""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "lora-sdr-lightweight-standalone-library-clean_amd"))
import lphy  # noqa: E402


def timed(fn, reps=20):
    s = torch.cuda.current_stream()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps / 1e3


def walled(fn, reps=20):
    """Host clock around `reps` calls that end in a device synchronise (for
    routes with host-to-device copies in them)."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def _stats(xs):
    xs = sorted(xs)
    return {"median_ms": xs[len(xs) // 2] * 1e3, "min_ms": xs[0] * 1e3, "max_ms": xs[-1] * 1e3}


def ragged(nf, out_path, rounds=7):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2)
    N, nkeys, stride = 128, 1024, 64
    lens = rng.integers(12, 65, nf)
    offs = np.concatenate([[0], np.cumsum(lens)])
    desc = np.zeros(nf + 1, lphy.RAGGED_DESC_DTYPE)
    desc["samples"][:-1] = (2 * lens + 2) * N
    desc["sym_offset"] = 2 * offs
    desc["unit_offset"] = np.concatenate([[0], np.cumsum(2 * lens + 2)])
    desc["iq_offset"] = desc["unit_offset"] * N
    total = int(offs[-1])
    st = torch.cuda.current_stream().cuda_stream
    keys = torch.from_numpy(rng.integers(0, 256, 16 * nkeys, dtype=np.uint8)).to(dev)
    t_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)

    # frames to build: FOpts + FRMPayload of frame f at src[offs[f] - 12 f]
    tx = np.zeros(nf, lphy.LORAWAN_TX_DTYPE)
    tx["fopts_len"] = np.minimum(rng.integers(0, 16, nf), lens - 12)
    tx["payload_len"] = lens - 12 - tx["fopts_len"]
    tx["src_offset"] = offs[:-1] - 12 * np.arange(nf)
    tx["devaddr"] = rng.integers(0, 2 ** 32, nf, dtype=np.uint64)
    tx["key"], tx["fcnt"] = rng.integers(0, nkeys, nf), rng.integers(0, 65536, nf)
    tx["mtype"], tx["fctrl"] = rng.integers(0, 8, nf), 0x80
    src = rng.integers(0, 256, total - 12 * nf + 4, dtype=np.uint8)
    t_src = torch.from_numpy(src).to(dev)
    t_bytes = torch.zeros(total + 4, dtype=torch.uint8, device=dev)
    t_status = torch.zeros(nf, dtype=torch.int32, device=dev)
    tx_bytes = tx.view(np.uint8)

    def build_new():
        lphy.lorawan_build_ragged(t_src, torch.from_numpy(tx_bytes).to(dev), t_desc, nf, N, keys, t_bytes, t_status,
                                  stream=st, src_bytes=src.size, out_syms=2 * total)

    t_tx = torch.from_numpy(tx_bytes.copy()).to(dev)

    def build_new_kernel():
        lphy.lorawan_build_ragged(t_src, t_tx, t_desc, nf, N, keys, t_bytes, t_status, stream=st,
                                  src_bytes=src.size, out_syms=2 * total)

    # the route without it: the host assembles MHDR..FRMPayload (not timed) and uploads them with a MIC job each
    build_new_kernel()
    torch.cuda.synchronize()
    assert bool((t_status == torch.from_numpy((2 * lens).astype(np.int32)).to(dev)).all())
    built = t_bytes.cpu().numpy()
    host_frames = built.copy()
    mic_at = (offs[1:] - 4)[:, None] + np.arange(4)[None, :]
    host_frames[mic_at] = 0
    jobs = np.zeros(nf, lphy.LORAWAN_DESC_DTYPE)
    jobs["offset"], jobs["len"], jobs["devaddr"], jobs["fcnt"] = offs[:-1], lens - 4, tx["devaddr"], tx["fcnt"]
    jobs["key"], jobs["uplink"] = tx["key"], (tx["mtype"] & 1) == 0
    jobs_bytes = jobs.view(np.uint8)
    t_old = torch.zeros_like(t_bytes)

    def build_old():
        t_old.copy_(torch.from_numpy(host_frames))
        lphy.lorawan_mic_batch(t_old, torch.from_numpy(jobs_bytes).to(dev), keys, None, lphy.LW_APPEND, stream=st)

    t_jobs = torch.from_numpy(jobs_bytes.copy()).to(dev)

    def build_old_kernel():
        lphy.lorawan_mic_batch(t_old, t_jobs, keys, None, lphy.LW_APPEND, stream=st)

    build_old()
    torch.cuda.synchronize()
    assert torch.equal(t_old, t_bytes), "the two build routes disagree"

    # parse: the built frames, every fifth with a wrong MIC
    rows = built.copy()
    rows[offs[1::5] - 1] ^= 0x01
    t_rows = torch.from_numpy(rows).to(dev)
    t_kidx = torch.from_numpy(tx["key"].astype(np.int32)).to(dev)
    t_out = torch.zeros(nf * 32, dtype=torch.uint8, device=dev)
    t_ref = torch.zeros(nf * 32, dtype=torch.uint8, device=dev)

    def parse_new():
        lphy.lorawan_parse_ragged(t_rows, t_desc, nf, N, 1, keys, t_out, key_index=t_kidx, stream=st,
                                  out_syms=2 * total)

    col = np.arange(stride)[None, :]
    t_idx = torch.from_numpy(np.minimum(offs[:-1, None] + col, total - 1)).to(dev)
    t_mask = torch.from_numpy((col < lens[:, None]).astype(np.uint8)).to(dev)
    t_lens = torch.from_numpy(lens.astype(np.int32)).to(dev)

    def parse_old():
        padded = (t_rows[t_idx] * t_mask).reshape(-1)
        lphy.lorawan_parse_batch(padded, nf, stride, 0, keys, t_ref, lens=t_lens, key_index=t_kidx, stream=st)

    parse_new(), parse_old()
    torch.cuda.synchronize()
    assert torch.equal(t_out, t_ref), "the two parse routes disagree"

    # the payload cipher on the rows the parse accepted, in place (applied twice it restores them)
    t_plain = t_rows.clone()

    def crypt_rx():
        lphy.lorawan_crypt_rx_ragged(t_plain, t_desc, t_out, nf, N, 1, keys, stream=st, out_syms=2 * total)

    crypt_rx()
    torch.cuda.synchronize()
    assert not torch.equal(t_plain, t_rows)
    crypt_rx()
    torch.cuda.synchronize()
    assert torch.equal(t_plain, t_rows), "the cipher applied twice does not restore the rows"

    res = {k: [] for k in ("parse_ragged", "parse_gather_batch", "build_ragged_kernel", "mic_batch_kernel",
                           "crypt_rx_ragged", "build_ragged_with_upload", "mic_batch_with_upload")}
    for _ in range(rounds):
        res["parse_ragged"].append(timed(parse_new, 200))
        res["parse_gather_batch"].append(timed(parse_old, 200))
        res["build_ragged_kernel"].append(timed(build_new_kernel, 200))
        res["mic_batch_kernel"].append(timed(build_old_kernel, 200))
        res["crypt_rx_ragged"].append(timed(crypt_rx, 200))
        res["build_ragged_with_upload"].append(walled(build_new, 50))
        res["mic_batch_with_upload"].append(walled(build_old, 50))
    out = {"frames": nf, "frame_bytes": "12..64", "total_bytes": total, "rounds": rounds,
           "timing": "device events over 200 calls (kernel routes), host clock to a synchronise over 50 calls "
                     "(routes with uploads); the pairs alternate in one process",
           "device": torch.cuda.get_device_name(0)}
    out.update({k: _stats(v) for k, v in res.items()})
    line = json.dumps(out)
    print(line)
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(out, indent=1) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "ragged":
        return ragged(int(sys.argv[2]) if len(sys.argv) > 2 else 65536, sys.argv[3] if len(sys.argv) > 3 else None)
    nf = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    rows = torch.from_numpy(rng.integers(0, 256, nf * L, dtype=np.uint8)).to(dev)
    keys = torch.from_numpy(rng.integers(0, 256, 16 * 1024, dtype=np.uint8)).to(dev)
    d = np.zeros(nf, lphy.LORAWAN_DESC_DTYPE)
    d["offset"] = np.arange(nf) * L
    d["len"] = L - 4
    d["devaddr"] = rng.integers(0, 2**32, nf, dtype=np.uint64).astype(np.uint32)
    d["fcnt"] = np.arange(nf)
    d["key"] = rng.integers(0, 1024, nf)
    d["uplink"] = 1
    desc = torch.from_numpy(d.view(np.uint8).copy()).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    t_mic = timed(lambda: lphy.lorawan_mic_batch(rows, desc, keys, None, lphy.LW_APPEND, stream=st))
    out = torch.empty(nf * 32, dtype=torch.uint8, device=dev)
    kidx = torch.from_numpy(d["key"].astype(np.int32)).to(dev)
    t_parse = timed(lambda: lphy.lorawan_parse_batch(rows, nf, L, L, keys, out, key_index=kidx, stream=st))
    blocks = (L - 4 + 16 + 15) // 16 + 1  # CMAC blocks + the subkey block
    res = {"frames": nf, "row_bytes": L, "mic_ms": t_mic * 1e3, "mic_frames_per_s": nf / t_mic,
           "parse_ms": t_parse * 1e3, "parse_frames_per_s": nf / t_parse,
           "aes_blocks_per_s": nf * blocks / t_mic}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
