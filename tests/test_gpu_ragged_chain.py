"""The receive chain of the reference (phy.hpp: estimate_offsets ->
compensate_offsets -> demodulate -> decode) for frames of different lengths,
device-resident on one stream with no host copy between the calls:
estimate_ragged leaves cfo / time_offset in d_meta, compensate_ragged reads
them there, demod_ragged takes the corrected IQ, all three on one
lphy_ragged_desc table.  Per frame the expectation is the oracle's chain on
that frame alone, bit for bit."""
import numpy as np
import pytest
import torch

from test_gpu_estimate import _bits

pytestmark = pytest.mark.gpu

FRAMES = 12


def _frames(oracle, sf, seed):
    """12 frames of 4..20 symbols (1..9 payload bytes), each with its own small
    CFO and integer delay, as test_gpu_osr._frames makes them."""
    rng = np.random.default_rng(seed)
    N = 1 << sf
    out = []
    for f in range(FRAMES):
        plen = 1 + (5 * f + 3) % 9
        iq = oracle.modulate(oracle.encode(rng.integers(0, 256, plen, dtype=np.uint8).tobytes()), sf)
        cfo = float(rng.uniform(-0.08, 0.08))
        iq = (iq * np.exp(2j * np.pi * cfo / N * np.arange(iq.size))).astype(np.complex64)
        d = int(rng.integers(0, 4))
        if d:
            iq = np.concatenate([np.zeros(d, np.complex64), iq[:-d]])
        out.append(iq)
    lens = sorted({x.size // N for x in out})
    assert lens[0] == 4 and lens[-1] == 20 and len(lens) >= 6
    return out


@pytest.mark.parametrize("sf", [7, 9])
def test_estimate_compensate_demod_on_one_stream(oracle, lphy, sf):
    N = 1 << sf
    frames = _frames(oracle, sf, 50 + sf)
    # the oracle's chain, frame by frame
    want = []
    for x in frames:
        est = oracle.estimate_offsets(x[: 2 * N], sf)
        comp = oracle.compensate_offsets(x, sf, float(est[0]), float(est[1]), 1)
        r, syms, sync, met = oracle.demodulate(comp, sf)
        assert r == x.size // N - 2
        nb, data, _ = oracle.decode(syms)
        assert nb == r // 2
        want.append((est, comp, syms, sync, met, data))

    d = lphy.Demodulator(sf)
    mode = lphy.MODE_DEMODULATE
    desc = d.ragged_layout([x.size for x in frames], mode)
    n_iq, n_out = d._ragged_extent(desc, mode)
    dev = torch.device("cuda", d.device)
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(s):
        t_in = torch.from_numpy(np.concatenate(frames).view(np.float32).copy()).to(dev)
        t_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        t_out = torch.full((n_iq * 2,), float("nan"), dtype=torch.float32, device=dev)
        t_meta = torch.full((FRAMES * 32,), 0xA5, dtype=torch.uint8, device=dev)
        t_syms = torch.full((n_out,), -1, dtype=torch.int16, device=dev)
        t_pay = torch.full(((n_out + 1) // 2,), 0xA5, dtype=torch.uint8, device=dev)
        d.estimate_ragged(t_in, t_desc, FRAMES, 2 * N, t_meta, stream=s.cuda_stream, iq_samples=n_iq)
        estimated = t_meta.clone()  # (a device copy in stream order: not a synchronisation)
        d.compensate_ragged(t_in, t_out, t_desc, FRAMES, t_meta, stream=s.cuda_stream, iq_samples=n_iq)
        d.demod_ragged(t_out, t_desc, FRAMES, t_syms, t_meta, mode, lphy.F_DECODE, payload=t_pay,
                       stream=s.cuda_stream, iq_samples=n_iq, out_syms=n_out)
        s.synchronize()
    est_meta = estimated.cpu().numpy().view(lphy.META_DTYPE)
    meta = t_meta.cpu().numpy().view(lphy.META_DTYPE)
    comp = t_out.cpu().numpy().view(np.complex64)
    syms = t_syms.cpu().numpy().view(np.uint16)
    pay = t_pay.cpu().numpy()
    for f, (w_est, w_comp, w_syms, w_sync, w_met, w_data) in enumerate(want):
        what = f"frame {f} ({frames[f].size // N} symbols)"
        assert _bits(est_meta["cfo"][f]) == _bits(w_est[0]), f"{what}: estimated cfo"
        assert _bits(est_meta["time_offset"][f]) == _bits(w_est[1]), f"{what}: estimated time_offset"
        o, n = int(desc["iq_offset"][f]), int(desc["samples"][f])
        assert comp[o: o + n].tobytes() == w_comp.tobytes(), f"{what}: compensated IQ"
        so = int(desc["sym_offset"][f])
        assert np.array_equal(syms[so: so + w_syms.size], w_syms), f"{what}: symbols"
        assert np.array_equal(pay[so // 2: so // 2 + w_data.size], w_data), f"{what}: bytes"
        assert meta["status"][f] == 0 and meta["sync_word"][f] == w_sync, f"{what}: sync word"
        # the demodulator's own estimate on the corrected frame, as the reference leaves it in the metrics
        assert _bits(meta["cfo"][f]) == _bits(w_met[0]), f"{what}: cfo"
        assert _bits(meta["time_offset"][f]) == _bits(w_met[1]), f"{what}: time_offset"
