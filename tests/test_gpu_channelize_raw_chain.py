"""The receive chain from a wideband capture as a radio writes it:
lphy_hip_channelize_raw -> lphy_hip_detect_batch (dechirp, hop = N) ->
lphy_hip_find_frames -> lphy_hip_demod_ragged (mode 2, decode), per channel, on
one stream with no host copy between the calls.

The capture is that of tests/test_gpu_channelize_chain.py (three channels of
three frames each, amplitude 1 a channel), quantised to SC16 at 8192 levels a
unit and to CU8 at 32 levels a unit (byte = round(32 v + 127.5), clipped; the
three channels together stay inside +-3 < 127.5 / 32).  The power-of-two scale
is folded into the taps, which is exact.

Quantisation noise makes the silent windows non-zero, so the float test's
threshold of 10 dB is not safe here: over N = 128 bins of noise the peak passes
the mean by 10 dB about once in 170 windows.  The threshold here is 20 dB; a
chirp leads its window's mean by far more even at 8 bits.  What keeps that
honest is test_model_streams_mark_and_decode_on_the_cpu, which runs before any
device call: the model's streams and the oracle's detector alone mark exactly
the frames' windows active at that threshold."""
import numpy as np
import pytest

import channelize_model as model
import detect_cases as dc
import sample_formats as sf
from resample_helpers import frames_of, rx_buffers
from test_gpu_channelize_chain import (BETA, CENTRES, CUTOFF, D, FILL, MAX_FRAMES, N, SF, SYMBOLS, T, narrow_stream,
                                       wideband)

pytestmark = pytest.mark.gpu

SCALE = {sf.FMT_SC16: 8192, sf.FMT_CU8: 32}        # levels a unit; the taps carry 1 / SCALE
THRESHOLD_DB = 20.0
FORMATS = pytest.mark.parametrize("fmt", list(SCALE), ids=[sf.NAMES[f] for f in SCALE])


@pytest.fixture(scope="module")
def setup(oracle, lphy):
    frames = [frames_of(oracle, ch) for ch in range(3)]
    streams, places = zip(*[narrow_stream(lphy, frames[ch], ch) for ch in range(3)])
    cap = wideband(streams)
    taps, rot, R, delay = model.design(CENTRES, D, T, CUTOFF, BETA)
    assert R == 5 and delay == 64 and delay % D == 0
    n_out = model.outputs(cap.size, 0, T, D)
    assert n_out == SYMBOLS * N - (T - 1) // 2 // D
    per = {}
    for fmt, scale in SCALE.items():
        q = sf.quantise(cap, fmt, scale)
        lo, hi = (0, 255) if fmt == sf.FMT_CU8 else (-32768, 32767)
        assert q.min() > lo and q.max() < hi       # nothing clipped
        t = (taps.view(np.float32) * np.float32(1.0 / scale)).view(np.complex64)
        assert (t.view(np.float32) * np.float32(scale)).tobytes() == taps.view(np.float32).tobytes()  # exact
        per[fmt] = dict(cap=q, taps=t, want=model.channelize(sf.to_float(q, fmt), t, rot, D, 0, n_out, 0))
    return dict(frames=frames, places=places, rot=rot, n_out=n_out, per=per)


@FORMATS
def test_model_streams_mark_and_decode_on_the_cpu(oracle, lphy, setup, fmt):
    """A condition on the input, before any device call: on the model's three
    streams the oracle's detector marks, at THRESHOLD_DB, exactly the frames'
    windows active, and the oracle decodes the streams to the frames sent."""
    windows = setup["n_out"] // N
    for ch in range(3):
        s = setup["per"][fmt]["want"][ch]
        rec = dc.expected(oracle, lphy, s, SF, 0, N, 1, windows, True, False)
        with np.errstate(invalid="ignore"):
            active = (rec["power"] - rec["power_avg"]).astype(np.float32) >= np.float32(THRESHOLD_DB)
        want = np.zeros(windows, bool)
        for frame, at in zip(setup["frames"][ch], setup["places"][ch]):
            assert at % N == 0
            want[at // N: at // N + 2 * frame.size + 2] = True
        np.testing.assert_array_equal(active, want, err_msg=f"{sf.NAMES[fmt]} channel {ch}")
        for frame, at in zip(setup["frames"][ch], setup["places"][ch]):
            n = (2 * frame.size + 2) * N
            r, syms, sync, _ = oracle.lora_demodulate(oracle.dechirp(s[at: at + n], SF), SF)
            assert r == 2 * frame.size, (ch, at)
            r, data, crc = oracle.decode(syms)
            assert r == frame.size and crc == 1, (ch, at)
            np.testing.assert_array_equal(data, frame)


def upload(dev, setup, fmt):
    import torch
    p = setup["per"][fmt]
    t_cap = torch.from_numpy(p["cap"].reshape(-1).copy()).to(dev)
    t_taps = torch.from_numpy(p["taps"].view(np.float32).copy()).to(dev)
    t_rot = torch.from_numpy(setup["rot"].view(np.float32).copy()).to(dev)
    return t_cap, t_taps, t_rot


@FORMATS
def test_device_streams_equal_the_model(lphy, setup, fmt):
    import torch
    d = lphy.Demodulator(SF)
    dev = torch.device("cuda", d.device)
    n_out, cap = setup["n_out"], setup["per"][fmt]["cap"]
    t_cap, t_taps, t_rot = upload(dev, setup, fmt)
    t_out = torch.zeros(3 * n_out * 2, dtype=torch.float32, device=dev)
    d.channelize_raw(t_cap, fmt, lphy.chan_plan(0, cap.shape[0], n_out, n_out, 0, 3, T, D, 5), t_taps, t_rot, t_out,
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = t_out.cpu().numpy().view(np.complex64).reshape(3, n_out)
    d.close()
    np.testing.assert_array_equal(got.view(np.uint8), setup["per"][fmt]["want"].view(np.uint8))


@FORMATS
def test_chain_from_the_integer_capture(lphy, setup, fmt):
    import torch
    d = lphy.Demodulator(SF)
    dev = torch.device("cuda", d.device)
    n_out, cap = setup["n_out"], setup["per"][fmt]["cap"]
    windows = n_out // N
    n_sym = n_out // N + 2
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    res = []
    with torch.cuda.stream(s):
        t_cap, t_taps, t_rot = upload(dev, setup, fmt)
        t_streams = torch.zeros(3 * n_out * 2, dtype=torch.float32, device=dev)
        per = [rx_buffers(d, dev, windows, n_sym, MAX_FRAMES, FILL) for ch in range(3)]
        # everything below is enqueued on the one stream; the host reads nothing until the end
        d.channelize_raw(t_cap, fmt, lphy.chan_plan(0, cap.shape[0], n_out, n_out, 0, 3, T, D, 5), t_taps, t_rot,
                         t_streams, stream=s.cuda_stream)
        prm = lphy.find_params(first=0, hop=N, lead=0, total_samples=n_out, threshold_db=THRESHOLD_DB, max_gap=0,
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
