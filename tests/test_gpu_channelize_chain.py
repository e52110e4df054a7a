"""The receive chain from a wideband capture: lphy_hip_channelize ->
lphy_hip_detect_batch (dechirp, hop = N) -> lphy_hip_find_frames ->
lphy_hip_demod_ragged (mode 2, decode), per channel, on one stream with no host
copy between the calls.

SF 7, three channels at -3/10, +1/10 and +3/10 cycles per wideband sample
(-300, +100, +300 kHz at 1 MS/s; R = 5), decimation 8 to 125 kS/s, a
Kaiser(8)-windowed sinc of 129 taps with its edge at 0.09 cycles per sample:
the delay is 64 input samples, 8 output samples.  Each channel carries three
frames from tx_ragged_host, symbol-aligned in silence, of 1 to 5 payload bytes
each between the two header bytes and the sx1272 checksum that lora_phy::decode
takes its crc_ok from (a frame of fewer than 4 bytes has crc_ok = 0 by that
rule, so the frames sent are 5 to 9 bytes long).

The wideband capture is made in float64: every channel's stream FFT-interpolated
by 8, mixed to its centre, the three summed behind 64 zeros - the filter's
delay then puts the frames back on the symbol lattice - and rounded to complex64."""
from fractions import Fraction as F

import numpy as np
import pytest

import channelize_model as model
from resample_helpers import frames_of, rx_buffers

pytestmark = pytest.mark.gpu

SF, N, D, T = 7, 128, 8, 129
CENTRES = [F(-3, 10), F(1, 10), F(3, 10)]
CUTOFF, BETA = 0.09, 8.0
GAPS = [[3, 2, 4], [2, 5, 2], [4, 3, 3]]           # symbols of silence in front of each frame
SYMBOLS = 80                                        # per channel stream
MAX_FRAMES = 5
FILL = 0xEE


def narrow_stream(lphy, frames, ch):
    """(stream complex64 of SYMBOLS symbols, the frames' first samples)."""
    d = lphy.Demodulator(SF)
    iq, _, sent = d.tx_ragged_host(frames, want_syms=False)
    d.close()
    s = np.zeros(SYMBOLS * N, np.complex64)
    at, places = 0, []
    for f, g in enumerate(GAPS[ch]):
        at += g * N
        a, n = int(sent["iq_offset"][f]), int(sent["samples"][f])
        assert n == (2 * frames[f].size + 2) * N
        s[at: at + n] = iq[a: a + n]
        places.append(at)
        at += n
    assert at + 2 * N <= s.size
    return s, places


def wideband(streams):
    n = SYMBOLS * N
    wide = np.zeros(n * D, np.complex128)
    t = np.arange(n * D)
    for s, c in zip(streams, CENTRES):
        spec = np.fft.fft(s.astype(np.complex128))
        up = np.zeros(n * D, np.complex128)
        up[: n // 2] = spec[: n // 2]
        up[-(n // 2):] = spec[n // 2:]
        phase = np.array([float((c * int(i)) % 1) for i in t])
        wide += np.fft.ifft(up) * D * np.exp(2j * np.pi * phase)
    return np.concatenate([np.zeros((T - 1) // 2, np.complex128), wide]).astype(np.complex64)


@pytest.fixture(scope="module")
def setup(oracle, lphy):
    frames = [frames_of(oracle, ch) for ch in range(3)]
    streams, places = zip(*[narrow_stream(lphy, frames[ch], ch) for ch in range(3)])
    cap = wideband(streams)
    taps, rot, R, delay = model.design(CENTRES, D, T, CUTOFF, BETA)
    assert R == 5 and delay == 64 and delay % D == 0
    n_out = model.outputs(cap.size, 0, T, D)
    assert n_out == SYMBOLS * N - (T - 1) // 2 // D   # the filter's delay, in output samples, is lost at the end
    want = model.channelize(cap, taps, rot, D, 0, n_out, 0)
    return dict(frames=frames, places=places, cap=cap, taps=taps, rot=rot, n_out=n_out, want=want)


def test_model_streams_decode_on_the_cpu(oracle, setup):
    """A condition on the input, before any device call: the model's three
    streams demodulate and decode, by the oracle, to the frames sent."""
    for ch in range(3):
        s = setup["want"][ch]
        for frame, at in zip(setup["frames"][ch], setup["places"][ch]):
            n = (2 * frame.size + 2) * N
            r, syms, sync, _ = oracle.lora_demodulate(oracle.dechirp(s[at: at + n], SF), SF)
            assert r == 2 * frame.size, (ch, at)
            r, data, crc = oracle.decode(syms)
            assert r == frame.size and crc == 1, (ch, at)
            np.testing.assert_array_equal(data, frame)


def test_device_streams_equal_the_model(lphy, setup):
    import torch
    d = lphy.Demodulator(SF)
    dev = torch.device("cuda", d.device)
    cap, n_out = setup["cap"], setup["n_out"]
    t_out = torch.zeros(3 * n_out * 2, dtype=torch.float32, device=dev)
    d.channelize(torch.from_numpy(cap.view(np.float32).copy()).to(dev),
                 lphy.chan_plan(0, cap.size, n_out, n_out, 0, 3, T, D, 5),
                 torch.from_numpy(setup["taps"].view(np.float32).copy()).to(dev),
                 torch.from_numpy(setup["rot"].view(np.float32).copy()).to(dev), t_out,
                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = t_out.cpu().numpy().view(np.complex64).reshape(3, n_out)
    d.close()
    np.testing.assert_array_equal(got.view(np.uint8), setup["want"].view(np.uint8))


def test_chain_from_the_wideband_capture(lphy, setup):
    import torch
    d = lphy.Demodulator(SF)
    dev = torch.device("cuda", d.device)
    cap, n_out = setup["cap"], setup["n_out"]
    windows = n_out // N
    n_sym = n_out // N + 2
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    res = []
    with torch.cuda.stream(s):
        t_cap = torch.from_numpy(cap.view(np.float32).copy()).to(dev)
        t_taps = torch.from_numpy(setup["taps"].view(np.float32).copy()).to(dev)
        t_rot = torch.from_numpy(setup["rot"].view(np.float32).copy()).to(dev)
        t_streams = torch.zeros(3 * n_out * 2, dtype=torch.float32, device=dev)
        per = [rx_buffers(d, dev, windows, n_sym, MAX_FRAMES, FILL) for ch in range(3)]
        # everything below is enqueued on the one stream; the host reads nothing until the end
        d.channelize(t_cap, lphy.chan_plan(0, cap.size, n_out, n_out, 0, 3, T, D, 5), t_taps, t_rot, t_streams,
                     stream=s.cuda_stream)
        prm = lphy.find_params(first=0, hop=N, lead=0, total_samples=n_out, threshold_db=10.0, max_gap=0,
                               min_symbols=1)
        for ch, b in enumerate(per):
            t_iq = t_streams[ch * n_out * 2: (ch + 1) * n_out * 2]
            d.detect_batch(t_iq, n_out, 0, N, 1, windows, b["rec"], lphy.DET_DECHIRP, stream=s.cuda_stream)
            d.find_frames(b["rec"], windows, prm, 2, MAX_FRAMES, b["desc"], b["info"], b["work"],
                          stream=s.cuda_stream)
            d.demod_ragged(t_iq, b["desc"], MAX_FRAMES, b["syms"], b["meta"], lphy.MODE_DECHIRP_LORA_DEMODULATE,
                           lphy.F_DECODE, payload=b["data"], stream=s.cuda_stream, iq_samples=n_out, out_syms=n_sym)
        s.synchronize()
        for b in per:
            res.append((b["desc"].cpu().numpy().view(lphy.RAGGED_DESC_DTYPE).copy(),
                        b["info"].cpu().numpy().view(lphy.FIND_INFO).copy()[0],
                        b["data"].cpu().numpy().copy(), b["meta"].cpu().numpy().view(lphy.META_DTYPE).copy()))
    d.close()
    for ch, (desc, info, data, meta) in enumerate(res):
        frames, places = setup["frames"][ch], setup["places"][ch]
        assert int(info["frames"]) == 3 and int(info["bursts"]) == 3, (ch, info)
        assert int(info["dropped_short"]) == int(info["dropped_long"]) == int(info["overflow"]) == 0
        for f, (frame, at) in enumerate(zip(frames, places)):
            assert int(desc["iq_offset"][f]) == at and int(desc["samples"][f]) == (2 * frame.size + 2) * N, (ch, f)
            o = int(desc["sym_offset"][f]) // 2
            np.testing.assert_array_equal(data[o: o + frame.size], frame, err_msg=f"channel {ch} frame {f}")
            assert meta["status"][f] == 0 and meta["have_sync"][f] == 1 and meta["crc_ok"][f] == 1, (ch, f)
