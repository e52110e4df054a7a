"""The receive chain from the capture: lphy_hip_detect_batch (hop = N, dechirp)
-> lphy_hip_find_frames -> lphy_hip_demod_ragged (frames = max_frames, mode 2,
decode) on one stream with no host copy between the calls.

The capture holds eight frames of 1 .. 9 payload bytes from tx_ragged_host,
symbol-aligned in silence.  The table must equal the definition
(tests/find_frames_model.py) applied to the oracle's detector records of the
capture - lphy_hip_detect_batch is pinned to those bit for bit by
tests/test_gpu_detect.py - and the known placement; the bytes at sym_offset / 2
must be the ones sent, and the padding frames give what a frame of 0 samples
gives in any ragged call."""
import numpy as np
import pytest

import detect_cases as dc
import find_frames_model as model

pytestmark = pytest.mark.gpu

LENS = [1, 9, 2, 5, 3, 8, 4, 6]   # payload bytes: frames of 4 .. 20 symbols
GAPS = [3, 2, 5, 4, 2, 3, 5, 4]   # symbols of silence in front of each frame
TRAIL = 4                         # ... and behind the last
MAX_FRAMES = 12
FILL = 0xEE

# The noisy case: complex AWGN of this sigma per component over the whole
# capture (signal amplitude 1), from this seed.  MARGIN_DB is read off the
# oracle's records of that capture on the CPU: every frame window has power -
# power_avg >= THRESHOLD_DB + MARGIN_DB (the least is 16.48 dB), every other finite
# window <= THRESHOLD_DB - MARGIN_DB (the largest is -16.05 dB: power_avg of a
# noise window is above its peak's power).  Asserted before any device call: a
# condition on the input, not a result of the search.
NOISE_SEED, NOISE_SIGMA, THRESHOLD_DB, MARGIN_DB = 4242, 0.1, 0.0, 12.0


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def capture(lphy, sf, noise=False):
    """(capture complex64, payloads, the frames' first samples, their table as sent)."""
    N = 1 << sf
    rng = np.random.default_rng(100 + sf)
    payloads = [rng.integers(0, 256, n, dtype=np.uint8) for n in LENS]
    d = lphy.Demodulator(sf)
    iq, _, sent = d.tx_ragged_host(payloads, want_syms=False)
    d.close()
    total = sum(GAPS) + TRAIL + sum(2 * n + 2 for n in LENS)
    cap = np.zeros(total * N, np.complex64)
    at, places = 0, []
    for f, g in enumerate(GAPS):
        at += g * N
        a, n = int(sent["iq_offset"][f]), int(sent["samples"][f])
        cap[at: at + n] = iq[a: a + n]
        places.append(at)
        at += n
    assert at + TRAIL * N == cap.size
    if noise:
        g = np.random.default_rng(NOISE_SEED)
        cap = (cap + NOISE_SIGMA * (g.standard_normal(cap.size) + 1j * g.standard_normal(cap.size))).astype(np.complex64)
    return cap, payloads, places, sent


def placed_table(lphy, places, sent):
    """The table the search must find: tx_layout's, each frame where it was put."""
    want = np.zeros(MAX_FRAMES + 1, lphy.RAGGED_DESC_DTYPE)
    want[: len(LENS)] = sent[:-1]
    want["iq_offset"][: len(LENS)] = places
    want[len(LENS):] = (places[-1] + int(sent["samples"][len(LENS) - 1]), 0, int(sent["sym_offset"][-1]),
                        int(sent["unit_offset"][-1]))
    return want


def run_chain(lphy, sf, cap, p, hop, demod=True):
    """detect_batch -> find_frames [-> demod_ragged] on one stream:
    (records, table, info, symbols, bytes, meta)."""
    import torch
    N = 1 << sf
    d = lphy.Demodulator(sf)
    dev = torch.device("cuda", d.device)
    windows = (cap.size - N) // hop + 1
    n_out = cap.size // N + 2
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(s):
        t_iq = torch.from_numpy(cap.view(np.float32).copy()).to(dev)
        t_rec = torch.full((windows * 16,), FILL, dtype=torch.uint8, device=dev)
        t_desc = torch.full(((MAX_FRAMES + 1) * 32,), FILL, dtype=torch.uint8, device=dev)
        t_info = torch.full((32,), FILL, dtype=torch.uint8, device=dev)
        t_work = torch.full((d.find_frames_workspace(windows),), FILL, dtype=torch.uint8, device=dev)
        t_syms = torch.full((n_out,), -1, dtype=torch.int16, device=dev)
        t_bytes = torch.full((n_out // 2 + 1,), FILL, dtype=torch.uint8, device=dev)
        t_meta = torch.full((MAX_FRAMES * 32,), FILL, dtype=torch.uint8, device=dev)
        d.detect_batch(t_iq, cap.size, 0, hop, 1, windows, t_rec, lphy.DET_DECHIRP, stream=s.cuda_stream)
        d.find_frames(t_rec, windows, lphy.find_params(**p), 2, MAX_FRAMES, t_desc, t_info, t_work,
                      stream=s.cuda_stream)
        if demod:
            d.demod_ragged(t_iq, t_desc, MAX_FRAMES, t_syms, t_meta, lphy.MODE_DECHIRP_LORA_DEMODULATE, lphy.F_DECODE,
                           payload=t_bytes, stream=s.cuda_stream, iq_samples=cap.size, out_syms=n_out)
        s.synchronize()
    out = (t_rec.cpu().numpy().view(lphy.DETECT_DTYPE).copy(), t_desc.cpu().numpy().view(lphy.RAGGED_DESC_DTYPE).copy(),
           t_info.cpu().numpy().view(lphy.FIND_INFO).copy()[0], t_syms.cpu().numpy().view(np.uint16).copy(),
           t_bytes.cpu().numpy().copy(), t_meta.cpu().numpy().view(lphy.META_DTYPE).copy())
    d.close()
    return out


def assert_table(lphy, desc, info, want):
    wdesc, winfo = want
    np.testing.assert_array_equal(_u8(desc), _u8(wdesc.astype(lphy.RAGGED_DESC_DTYPE)))
    assert {k: int(info[k]) for k in model.INFO_FIELDS} == winfo
    assert not info["reserved"].any()


def zero_frame_meta(lphy, sf, n):
    """What a ragged demodulation gives for n frames of 0 samples."""
    d = lphy.Demodulator(sf)
    _, _, meta, _ = d.demod_ragged_host(np.zeros(0, np.complex64), [0] * n, lphy.MODE_DECHIRP_LORA_DEMODULATE,
                                        lphy.F_DECODE)
    d.close()
    return meta


def check_chain(oracle, lphy, sf, noise, threshold):
    N = 1 << sf
    cap, payloads, places, sent = capture(lphy, sf, noise)
    windows = cap.size // N
    orc = dc.expected(oracle, lphy, cap, sf, 0, N, 1, windows, True, False)
    p = model.params(hop=N, total_samples=cap.size, threshold_db=threshold)
    if noise:  # the threshold's margin on the input, on the CPU
        with np.errstate(invalid="ignore"):
            diff = orc["power"] - orc["power_avg"]
        inside = np.zeros(windows, bool)
        for at, n in zip(places, LENS):
            inside[at // N: at // N + 2 * n + 2] = True
        assert (diff[inside] >= threshold + MARGIN_DB).all(), diff[inside].min()
        rest = diff[~inside]
        assert (rest[np.isfinite(rest)] <= threshold - MARGIN_DB).all(), rest[np.isfinite(rest)].max()
    want = model.find_frames(orc, p, N, 2, MAX_FRAMES)
    placed = placed_table(lphy, places, sent)
    np.testing.assert_array_equal(_u8(want[0].astype(lphy.RAGGED_DESC_DTYPE)), _u8(placed))  # (the model, CPU only)

    rec, desc, info, syms, data, meta = run_chain(lphy, sf, cap, p, N)
    dc.assert_records_equal(rec, orc, "the detector's records")
    assert_table(lphy, desc, info, want)
    np.testing.assert_array_equal(_u8(desc), _u8(placed))
    assert int(info["frames"]) == len(LENS) and int(info["overflow"]) == 0
    for f, pay in enumerate(payloads):
        at = int(desc["sym_offset"][f]) // 2
        np.testing.assert_array_equal(data[at: at + pay.size], pay, err_msg=f"frame {f}")
        assert meta["status"][f] == 0 and meta["have_sync"][f] == 1
    # the padding frames: a frame of 0 samples, and nothing written behind the totals
    pad = MAX_FRAMES - len(LENS)
    np.testing.assert_array_equal(_u8(meta[len(LENS):]), _u8(zero_frame_meta(lphy, sf, pad)))
    n_sym = int(desc["sym_offset"][-1])
    assert (syms[n_sym:] == 0xFFFF).all() and (data[n_sym // 2:] == FILL).all()


@pytest.mark.parametrize("sf", [7, 9])
def test_clean_capture(oracle, lphy, sf):
    check_chain(oracle, lphy, sf, False, 10.0)


def test_noisy_capture(oracle, lphy):
    check_chain(oracle, lphy, 9, True, THRESHOLD_DB)


def test_sliding_windows(oracle, lphy):
    """hop = N / 4: the windows overlap; against the model alone."""
    sf, N = 7, 128
    cap, _, places, _ = capture(lphy, sf)
    hop = N // 4
    windows = (cap.size - N) // hop + 1
    orc = dc.expected(oracle, lphy, cap, sf, 0, hop, 1, windows, True, False)
    # at 0 dB a window halfway onto a frame is active and one a quarter onto it is not, so lead = N / 2
    p = model.params(hop=hop, lead=N // 2, total_samples=cap.size, threshold_db=0.0, max_gap=2, min_symbols=2)
    want = model.find_frames(orc, p, N, 2, MAX_FRAMES)
    assert want[1]["frames"] == len(LENS)   # (of the model: the case finds something)
    rec, desc, info, _, _, _ = run_chain(lphy, sf, cap, p, hop, demod=False)
    dc.assert_records_equal(rec, orc, "the detector's records")
    assert_table(lphy, desc, info, want)
