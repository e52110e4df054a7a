"""Transmit and receive closed over a wideband signal, on the device:
lphy_hip_tx_ragged (per channel) -> lphy_hip_synthesize -> lphy_hip_channelize
-> per channel lphy_hip_detect_batch (dechirp, hop = N) -> lphy_hip_find_frames
-> lphy_hip_demod_ragged (mode 2, decode), on one stream with no host copy
between the calls.

SF 7, three channels at -3/10, +1/10 and +3/10 cycles per wideband sample
(R = 5), interpolation and decimation 8, Kaiser(8)-windowed sincs of 129 taps
with their edge at 0.09 cycles per wideband sample on both sides
(lphy.synth_design, lphy.chan_design).  Narrow sample j is centred at wideband
sample 8 j + 64; the channeliser's output m, with first = 0, is centred at
wideband sample 8 m + 64: output m falls back on narrow sample m, so the frames
come back on the symbol lattice where they were put, and all SYMBOLS * N
samples of every stream come back.

Each channel carries three frames, symbol-aligned in silence, of 1 to 5 payload
bytes each between the two header bytes and the sx1272 checksum that
lora_phy::decode takes its crc_ok from (5 to 9 bytes a frame).  On the CPU the
frames are the oracle's encode + modulate, which lphy_hip_tx_ragged equals bit
for bit (asserted here on the streams)."""
from fractions import Fraction as F

import numpy as np
import pytest

import channelize_model
import synthesize_model as model
from resample_helpers import frames_of, rx_buffers

pytestmark = pytest.mark.gpu

SF, N, U, T = 7, 128, 8, 129
CENTRES = [F(-3, 10), F(1, 10), F(3, 10)]
CUTOFF, BETA = 0.09, 8.0
GAPS = [[3, 2, 4], [2, 5, 2], [4, 3, 3]]           # symbols of silence in front of each frame
SYMBOLS = 80                                        # per channel stream
MAX_FRAMES = 5
FILL = 0xEE


def places_of(frames, ch):
    at, places = 0, []
    for frame, g in zip(frames, GAPS[ch]):
        at += g * N
        places.append(at)
        at += (2 * frame.size + 2) * N
    assert at + 2 * N <= SYMBOLS * N
    return places


def narrow_stream(oracle, frames, places):
    """The stream of SYMBOLS symbols, by the oracle's encode + modulate."""
    s = np.zeros(SYMBOLS * N, np.complex64)
    for frame, at in zip(frames, places):
        iq = np.asarray(oracle.modulate(oracle.encode(frame.tobytes()), SF), np.complex64)
        assert iq.size == (2 * frame.size + 2) * N
        s[at: at + iq.size] = iq
    return s


@pytest.fixture(scope="module")
def setup(oracle, lphy):
    frames = [frames_of(oracle, ch) for ch in range(3)]
    places = [places_of(frames[ch], ch) for ch in range(3)]
    streams = np.stack([narrow_stream(oracle, frames[ch], places[ch]) for ch in range(3)])
    n = SYMBOLS * N
    s_taps, s_rot, R, delay = lphy.synth_design(CENTRES, U, T, CUTOFF, BETA)
    c_taps, c_rot, cR, c_delay = lphy.chan_design(CENTRES, U, T, CUTOFF, BETA)
    assert R == cR == 5 and delay == c_delay == 64
    n_wide = model.outputs(n, 0, T, U)
    assert n_wide == (n - 1) * U + T and channelize_model.outputs(n_wide, 0, T, U) == n
    wide = model.synthesize(streams, s_taps, s_rot, U, 0, n_wide, 0)
    back = channelize_model.channelize(wide, c_taps, c_rot, U, 0, n, 0)
    return dict(frames=frames, places=places, streams=streams, n=n, n_wide=n_wide, wide=wide, back=back,
                s_taps=s_taps, s_rot=s_rot, c_taps=c_taps, c_rot=c_rot)


def test_model_round_trip_decodes_on_the_cpu(oracle, setup):
    """A condition on the input, before any device call: the model's synthesize
    followed by the model's channelize gives three streams that the oracle
    demodulates and decodes to the frames sent, where they were put."""
    for ch in range(3):
        s = setup["back"][ch]
        for frame, at in zip(setup["frames"][ch], setup["places"][ch]):
            n = (2 * frame.size + 2) * N
            r, syms, sync, _ = oracle.lora_demodulate(oracle.dechirp(s[at: at + n], SF), SF)
            assert r == 2 * frame.size, (ch, at)
            r, data, crc = oracle.decode(syms)
            assert r == frame.size and crc == 1, (ch, at)
            np.testing.assert_array_equal(data, frame)


def test_tx_to_rx_over_the_wideband_stream(lphy, setup):
    import torch
    d = lphy.Demodulator(SF)
    dev = torch.device("cuda", d.device)
    n, n_wide = setup["n"], setup["n_wide"]
    windows = n // N
    n_sym = n // N + 2
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    res = []
    with torch.cuda.stream(s):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(-1).copy()).to(dev)  # noqa: E731
        t_st, t_sr, t_ct, t_cr = (up(setup[k]) for k in ("s_taps", "s_rot", "c_taps", "c_rot"))
        t_tx = torch.zeros(3 * n * 2, dtype=torch.float32, device=dev)       # the zeroed per-channel streams
        t_wide = torch.full((n_wide * 8,), FILL, dtype=torch.uint8, device=dev)
        t_rx = torch.zeros(3 * n * 2, dtype=torch.float32, device=dev)
        tx, per = [], []
        for ch in range(3):
            frames = setup["frames"][ch]
            desc = d.tx_layout([f.size for f in frames])
            desc["iq_offset"][:3] = setup["places"][ch]
            desc["iq_offset"][3] = n
            tx.append(dict(data=torch.from_numpy(np.concatenate(frames)).to(dev),
                           desc=torch.from_numpy(desc.view(np.uint8).copy()).to(dev),
                           bytes=int(sum(f.size for f in frames))))
            per.append(rx_buffers(d, dev, windows, n_sym, MAX_FRAMES, FILL))
        # everything below is enqueued on the one stream; the host reads nothing until the end
        for ch, b in enumerate(tx):
            d.tx_ragged(b["data"], b["desc"], 3, t_tx[ch * n * 2: (ch + 1) * n * 2], stream=s.cuda_stream,
                        iq_samples=n, out_syms=2 * b["bytes"])
        d.synthesize(t_tx, lphy.synth_plan(0, n, n, n_wide, 0, 3, T, U, 5), t_st, t_sr, t_wide, stream=s.cuda_stream)
        d.channelize(t_wide, lphy.chan_plan(0, n_wide, n, n, 0, 3, T, U, 5), t_ct, t_cr, t_rx, stream=s.cuda_stream)
        prm = lphy.find_params(first=0, hop=N, lead=0, total_samples=n, threshold_db=10.0, max_gap=0, min_symbols=1)
        for ch, b in enumerate(per):
            t_iq = t_rx[ch * n * 2: (ch + 1) * n * 2]
            d.detect_batch(t_iq, n, 0, N, 1, windows, b["rec"], lphy.DET_DECHIRP, stream=s.cuda_stream)
            d.find_frames(b["rec"], windows, prm, 2, MAX_FRAMES, b["desc"], b["info"], b["work"],
                          stream=s.cuda_stream)
            d.demod_ragged(t_iq, b["desc"], MAX_FRAMES, b["syms"], b["meta"], lphy.MODE_DECHIRP_LORA_DEMODULATE,
                           lphy.F_DECODE, payload=b["data"], stream=s.cuda_stream, iq_samples=n, out_syms=n_sym)
        s.synchronize()
        got_tx = t_tx.cpu().numpy().view(np.complex64).reshape(3, n)
        got_wide = t_wide.cpu().numpy().view(np.complex64)
        got_rx = t_rx.cpu().numpy().view(np.complex64).reshape(3, n)
        for b in per:
            res.append((b["desc"].cpu().numpy().view(lphy.RAGGED_DESC_DTYPE).copy(),
                        b["info"].cpu().numpy().view(lphy.FIND_INFO).copy()[0],
                        b["data"].cpu().numpy().copy(), b["meta"].cpu().numpy().view(lphy.META_DTYPE).copy()))
    d.close()
    np.testing.assert_array_equal(got_tx.view(np.uint8), setup["streams"].view(np.uint8),
                                  err_msg="tx_ragged's streams are not the oracle's")
    np.testing.assert_array_equal(got_wide.view(np.uint8), setup["wide"].view(np.uint8),
                                  err_msg="the wideband stream is not the model's")
    np.testing.assert_array_equal(got_rx.view(np.uint8), setup["back"].view(np.uint8))
    for ch, (desc, info, data, meta) in enumerate(res):
        frames, places = setup["frames"][ch], setup["places"][ch]
        assert int(info["frames"]) == 3 and int(info["bursts"]) == 3, (ch, info)
        assert int(info["dropped_short"]) == int(info["dropped_long"]) == int(info["overflow"]) == 0
        for f, (frame, at) in enumerate(zip(frames, places)):
            assert int(desc["iq_offset"][f]) == at and int(desc["samples"][f]) == (2 * frame.size + 2) * N, (ch, f)
            o = int(desc["sym_offset"][f]) // 2
            np.testing.assert_array_equal(data[o: o + frame.size], frame, err_msg=f"channel {ch} frame {f}")
            assert meta["status"][f] == 0 and meta["have_sync"][f] == 1 and meta["crc_ok"][f] == 1, (ch, f)
