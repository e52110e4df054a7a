"""lphy_hip_detect_ragged / lphy_hip_detect_ragged_host (k_detect over the
DetRagged geometry, csrc/lphy_detect.h): the reference's LoRaDetector::detect on every whole
symbol of every frame of a lphy_ragged_desc table in one launch, the record
of symbol s of frame f at unit_offset[f] + s.

Every record is compared bit for bit with orc_detect on the symbol's input
(tests/detect_ragged_cases.py over tests/detect_cases.py, pinned to the
reference build by tests/test_detect_cpu.py and, for the SF 7 and SF 10
tables, tests/test_detect_ragged_cpu.py with tests/golden/detect_ragged_v1.npz)
and byte for byte with lphy_hip_detect_host on each frame alone.

SF 7, 8 (several symbols per wavefront: the frame search runs per team), 10
(one per wavefront: on wave-uniform values) and 12 (four wavefronts per
symbol, a tile is one symbol)."""
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc
import detect_ragged_cases as rc

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ENOTSUP = -22, -34, -95
GUARD = 3  # records behind the call's, which it must leave alone


def _demod(lphy, sf, hann, **kw):
    return lphy.Demodulator(sf, window=lphy.WINDOW_HANN if hann else lphy.WINDOW_NONE, **kw)


def _flags(lphy, dechirp):
    return lphy.DET_DECHIRP if dechirp else 0


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def device_call(lphy, d, flat, desc, phase=0, flags=0, units_arg=True):
    """The device form into records pre-filled with 0xAB, GUARD records behind
    them: (records, the guard's bytes)."""
    import torch
    dev = torch.device("cuda", d.device)
    frames, units = desc.size - 1, int(desc["unit_offset"][-1])
    t_iq = torch.from_numpy(np.ascontiguousarray(flat, np.complex64).view(np.float32).copy()).to(dev)
    t_desc = torch.from_numpy(_u8(desc).copy()).to(dev)
    t_out = torch.full(((units + GUARD) * 16,), 0xAB, dtype=torch.uint8, device=dev)
    n_iq = int((desc["iq_offset"][:-1] + desc["samples"][:-1]).max()) if frames else 0
    d.detect_ragged(t_iq, t_desc, frames, t_out, phase, flags, stream=torch.cuda.current_stream().cuda_stream,
                    iq_samples=n_iq, units=units if units_arg else None)
    torch.cuda.synchronize()
    out = t_out.cpu().numpy()
    return out[: units * 16].view(lphy.DETECT_DTYPE).copy(), out[units * 16:]


def per_frame_detect_host(lphy, d, flat, desc, phase, flags):
    """lphy_hip_detect_host on each frame alone, concatenated in table order."""
    step = d.N * d.osr
    parts = [d.detect_host(flat, int(desc["iq_offset"][f]) + phase, step, d.osr, int(desc["samples"][f]) // step,
                           flags) for f in range(desc.size - 1)]
    return np.concatenate(parts) if parts else np.zeros(0, lphy.DETECT_DTYPE)


@pytest.fixture(scope="module")
def mixed(oracle):
    """(sf, dechirp) -> the frames of COUNTS[sf] as that call is given them, made once."""
    cache = {}

    def get(sf, dechirp):
        if (sf, dechirp) not in cache:
            cache[sf, dechirp] = rc.frames_of(oracle, sf, dechirp)
        return cache[sf, dechirp]
    return get


@pytest.fixture(scope="module")
def want_mixed(oracle, lphy, mixed):
    """(sf, hann, dechirp) -> the oracle's records of the packed mixed table, made once."""
    cache = {}

    def get(sf, hann, dechirp):
        key = (sf, hann, dechirp)
        if key not in cache:
            frames = mixed(sf, dechirp)
            desc = rc.packed_table(lphy, [x.size for x in frames], 1 << sf)
            cache[key] = rc.expected_table(oracle, lphy, np.concatenate(frames), desc, sf, dechirp, hann)
        return cache[key]
    return get


# ---- 1. mixed lengths against the oracle -----------------------------------------
@pytest.mark.parametrize("sf", [7, 8, 10, 12])
@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("dechirp", [False, True])
def test_mixed_lengths(oracle, lphy, mixed, want_mixed, sf, hann, dechirp):
    N, T = 1 << sf, rc.tile_of(sf)
    counts = rc.COUNTS[sf]
    frames = mixed(sf, dechirp)
    flat = np.concatenate(frames)
    d = _demod(lphy, sf, hann)
    got, desc = d.detect_ragged_host(flat, [x.size for x in frames], 0, _flags(lphy, dechirp))
    units = int(desc["unit_offset"][-1])
    assert units == sum(counts) == got.size
    assert T == 1 or units % T != 0   # a partial last tile
    assert [int(s) % N for s in desc["samples"][:-1]] == [N // 2 if k in rc.tailed(counts) else 0
                                                          for k in range(len(counts))]
    np.testing.assert_array_equal(_u8(desc), _u8(rc.packed_table(lphy, [x.size for x in frames], N)))
    for f, n in enumerate(counts):
        u, first = int(desc["unit_offset"][f]), int(desc["iq_offset"][f])
        if f in (1, len(counts) - 1):   # (want_mixed is this, frame by frame, made once)
            np.testing.assert_array_equal(_u8(dc.expected(oracle, lphy, flat, sf, first, N, 1, n, dechirp, hann)),
                                          _u8(want_mixed(sf, hann, dechirp)[u: u + n]))
        dc.assert_records_equal(got[u: u + n], want_mixed(sf, hann, dechirp)[u: u + n],
                                f"SF{sf} hann {hann} dechirp {dechirp} frame {f}")
    dc.assert_records_equal(got, want_mixed(sf, hann, dechirp), f"SF{sf} hann {hann} dechirp {dechirp}")
    # the parent's call on each frame alone, same library
    alone = per_frame_detect_host(lphy, d, flat, desc, 0, _flags(lphy, dechirp))
    np.testing.assert_array_equal(_u8(got), _u8(alone))
    if sf in rc.GOLDEN_SFS and dechirp and not hann:   # what the reference build gave
        gdesc, grec = rc.load_golden()[sf]
        np.testing.assert_array_equal(_u8(desc), _u8(gdesc))
        np.testing.assert_array_equal(_u8(got), _u8(grec))
    d.close()


# ---- 2. a hand-written table ----------------------------------------------------
def hand_written(lphy, N):
    """Reverse address order, gaps, an n == 0 frame between two others, two
    frames that overlap in the IQ (the fourth and the fifth)."""
    spans = [(20 * N + 5, 3 * N), (15 * N + 1, 2 * N + N // 2), (14 * N, N - 1), (11 * N, 3 * N),
             (9 * N + 7, 4 * N), (0, 2 * N)]
    desc = np.zeros(len(spans) + 1, lphy.RAGGED_DESC_DTYPE)
    for f, (o, n) in enumerate(spans):
        desc[f] = (o, n, 0xDEAD0000 + f, 0)   # (sym_offset is not read)
    desc["unit_offset"] = np.concatenate([[0], np.cumsum(desc["samples"][:-1] // np.uint64(N))])
    return desc


@pytest.mark.parametrize("sf", [7, 10])
@pytest.mark.parametrize("hann", [False, True])
def test_hand_written_table(oracle, lphy, sf, hann):
    N = 1 << sf
    iq = dc.packets(oracle, sf, True)
    desc = hand_written(lphy, N)
    o, n = desc["iq_offset"][:-1].astype(np.int64), desc["samples"][:-1].astype(np.int64)
    assert (np.diff(o) < 0).all() and n[2] // N == 0 and o[4] < o[3] < o[4] + n[4]
    assert int((o + n).max()) <= iq.size and int(desc["unit_offset"][-1]) == 14
    want = rc.expected_table(oracle, lphy, iq, desc, sf, True, hann)
    d = _demod(lphy, sf, hann)
    got, guard = device_call(lphy, d, iq, desc, 0, lphy.DET_DECHIRP)
    dc.assert_records_equal(got, want, f"SF{sf} hann {hann}")
    assert (guard == 0xAB).all()
    # the neighbours of the frame without a symbol, each alone
    for f in (1, 3):
        u = int(desc["unit_offset"][f])
        alone = d.detect_host(iq, int(o[f]), N, 1, int(n[f]) // N, lphy.DET_DECHIRP)
        np.testing.assert_array_equal(_u8(got[u: u + alone.size]), _u8(alone))
    # the host form takes the same table
    host, _ = d.detect_ragged_host(iq, desc, 0, lphy.DET_DECHIRP)
    np.testing.assert_array_equal(_u8(host), _u8(got))
    # without the caller's unit count the binding checks no record buffer: the same records
    again, guard = device_call(lphy, d, iq, desc, 0, lphy.DET_DECHIRP, units_arg=False)
    np.testing.assert_array_equal(_u8(again), _u8(got))
    assert (guard == 0xAB).all()
    d.close()


# ---- 3. osr 2 and 4, every phase ------------------------------------------------
@pytest.mark.parametrize("sf", [7, 10])
@pytest.mark.parametrize("osr", [2, 4])
@pytest.mark.parametrize("hann", [False, True])
def test_osr_phases(oracle, lphy, sf, osr, hann):
    from test_gpu_osr import _frames
    N = 1 << sf
    step = N * osr
    counts = [3, 0, 5, 1, 2]
    tails = [0, step - 1, step // 2, 0, 3]
    whole = _frames(oracle, sf, osr, len(counts), 2, seed=sf + 10 * osr, snr=-3.0)   # 6 symbols each
    frames = [np.ascontiguousarray(whole[k][: c * step + t]) for k, (c, t) in enumerate(zip(counts, tails))]
    flat = np.concatenate(frames)
    d = _demod(lphy, sf, hann, osr=osr)
    desc = d.ragged_layout([x.size for x in frames], lphy.MODE_DEMODULATE)
    assert list(np.diff(desc["unit_offset"].astype(np.int64))) == counts
    for phase in range(osr):
        for dechirp in (False, True):
            got, guard = device_call(lphy, d, flat, desc, phase, _flags(lphy, dechirp))
            assert (guard == 0xAB).all()
            for f, c in enumerate(counts):
                u, first = int(desc["unit_offset"][f]), int(desc["iq_offset"][f])
                want = dc.expected(oracle, lphy, flat, sf, first + phase, step, osr, c, dechirp, hann)
                dc.assert_records_equal(got[u: u + c], want, f"SF{sf} osr {osr} phase {phase} frame {f}")
            host, _ = d.detect_ragged_host(flat, desc, phase, _flags(lphy, dechirp))
            np.testing.assert_array_equal(_u8(host), _u8(got))
    d.close()


# ---- 4. special windows inside frames ---------------------------------------------
@pytest.mark.parametrize("sf", dc.SFS)
@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("dechirp", [False, True])
def test_special_windows(oracle, lphy, sf, hann, dechirp):
    from pathlib import Path
    N = 1 << sf
    normal = dc.detector_feed(oracle, dc.packets(oracle, sf, True)[: 2 * N], sf, dechirp)
    a, b = normal[:N], normal[N:]
    raw = np.fromfile(Path(__file__).parent / "golden" / "equal_power_iq.bin", np.complex64)
    tie = np.resize(raw, N).astype(np.complex64)
    nan_w, inf_w = a.copy(), b.copy()
    nan_w[N // 3] = np.complex64(complex(np.nan, 0.25))
    inf_w[N - 2] = np.complex64(complex(-0.5, np.inf))
    frames = [np.concatenate([np.zeros(N, np.complex64), tie, a]), np.zeros(N // 4, np.complex64),
              np.concatenate([nan_w, b, inf_w, a, a[: N // 2]])]
    flat = np.concatenate(frames)
    d = _demod(lphy, sf, hann)
    got, desc = d.detect_ragged_host(flat, [x.size for x in frames], 0, _flags(lphy, dechirp))
    assert list(desc["unit_offset"]) == [0, 3, 3, 7]
    with np.errstate(all="ignore"):
        want = rc.expected_table(oracle, lphy, flat, desc, sf, dechirp, hann)
    dc.assert_records_equal(got, want, "special")
    for w in (3, 5):   # the NaN and the inf symbol: not an ordinary record in the oracle either
        assert not (np.isfinite(want["power"][w]) and np.isfinite(want["power_avg"][w]))
    # the all-zero window
    assert got["index"][0] == 0 and got["findex"][0] == 0
    assert got["power"][0] == -np.inf and got["power_avg"][0] == -np.inf
    if not dechirp and not hann:
        assert got["index"][1] == 0  # equal power in bins 0 and N/2: the lowest
    # the other symbols of the same frames are what they are alone
    alone = d.detect_host(np.concatenate([a, b, a]), 0, N, 1, 3, _flags(lphy, dechirp))
    np.testing.assert_array_equal(_u8(got[[2, 4, 6]]), _u8(alone))
    assert np.isfinite(alone["power_avg"]).all()
    d.close()


# ---- 5. the serial counter ------------------------------------------------------
@pytest.mark.parametrize("sf", dc.SFS)
@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("dechirp", [False, True])
@pytest.mark.parametrize("noisy", [True, False])
def test_serial_counter(oracle, lphy, sf, hann, dechirp, noisy):
    """The windows that take the in-order walk count in the same counter as
    lphy_hip_detect_batch's: the fixture sets of detect_cases cut into frames
    give the count of the uniform call on the same windows."""
    N, W = 1 << sf, dc.NOISE_WINDOWS[sf]
    iq = dc.detector_feed(oracle, dc.packets(oracle, sf, noisy), sf, dechirp)
    counts = [W // 4, 0, 1, W - W // 4 - 1]
    d = _demod(lphy, sf, hann)
    d.detect_serial_count(reset=True)
    uniform = d.detect_host(iq, 0, N, 1, W, _flags(lphy, dechirp))
    n_uniform = d.detect_serial_count()
    got, desc = d.detect_ragged_host(iq, [c * N for c in counts], 0, _flags(lphy, dechirp))
    n_ragged = d.detect_serial_count()
    print(f"sf {sf} hann {hann} dechirp {dechirp} noisy {noisy}: {n_ragged} of {W} symbols walked in order "
          f"(uniform call: {n_uniform})")
    assert int(desc["unit_offset"][-1]) == W
    np.testing.assert_array_equal(_u8(got), _u8(uniform))
    assert n_ragged == n_uniform
    if not noisy and not hann:   # (test_gpu_detect.test_fixture_sets: pure cancellation in every window)
        assert n_ragged == W
    assert d.detect_serial_count() == 0   # read and cleared
    d.close()


# ---- 6. later trips of the persistent grid ----------------------------------------
@pytest.mark.parametrize("sf", [7, 8, 10, 12])
@pytest.mark.parametrize("hann,dechirp", [(False, True), (True, False)])
def test_later_trips(oracle, lphy, mixed, want_mixed, sf, hann, dechirp):
    T = rc.tile_of(sf)
    frames = mixed(sf, dechirp)
    flat = np.concatenate(frames)
    d = _demod(lphy, sf, hann, test_build=True)
    d.bounds_violations(reset=True)
    desc = d.ragged_layout([x.size for x in frames], lphy.MODE_DEMODULATE)
    units = int(desc["unit_offset"][-1])
    assert -(-units // T) >= 3 and (T == 1 or units % T != 0)
    d.detect_serial_count(reset=True)
    ref, guard = device_call(lphy, d, flat, desc, 0, _flags(lphy, dechirp))
    walked = d.detect_serial_count()
    assert (guard == 0xAB).all()
    what = f"SF{sf} hann {hann} dechirp {dechirp}"
    dc.assert_records_equal(ref, want_mixed(sf, hann, dechirp), f"{what} uncapped")
    for cap in ((1, 2, 3) if sf == 12 else (1, 3)):
        d.grid_cap(cap)
        got, guard = device_call(lphy, d, flat, desc, 0, _flags(lphy, dechirp))
        assert (guard == 0xAB).all()
        np.testing.assert_array_equal(_u8(got), _u8(ref), err_msg=f"{what} cap {cap} against the uncapped call")
        assert d.detect_serial_count() == walked, f"{what} cap {cap}"
        # the host form sizes its grid by the table's units, then the cap
        host, _ = d.detect_ragged_host(flat, desc, 0, _flags(lphy, dechirp))
        np.testing.assert_array_equal(_u8(host), _u8(ref), err_msg=f"{what} cap {cap}, host form")
        d.detect_serial_count(reset=True)
    assert d.bounds_violations() == 0
    d.close()


# ---- 7. the chain on one table ------------------------------------------------------
CHAIN_LENS = [1, 4, 9, 2, 16, 3, 7]   # payload bytes: frames of 4 .. 34 symbols
# (payload bytes, seed): payloads whose frames the reference's own chain leaves in place, see
# test_chain_data_symbols_are_the_transmitted
KEPT = [(2, 78), (5, 10821), (2, 278), (5, 25396), (2, 306), (5, 28796), (2, 10084)]


def run_chain(lphy, payloads, est_samples):
    """tx_ragged -> estimate_ragged -> compensate_ragged -> detect_ragged
    (dechirp), device-resident on one stream and one table, SF 7:
    (table, records)."""
    import torch
    sf = 7
    lens = [p.size for p in payloads]
    d = _demod(lphy, sf, False)
    desc = d.tx_layout(lens)
    frames, units = len(lens), int(desc["unit_offset"][-1])
    n_iq, n_sym = int(desc["iq_offset"][-1]), int(desc["sym_offset"][-1])
    assert units == sum(2 * n + 2 for n in lens)
    dev = torch.device("cuda", d.device)
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(s):
        data = np.zeros(n_sym // 2 + 1, np.uint8)
        for f, p in enumerate(payloads):
            at = int(desc["sym_offset"][f]) // 2
            data[at: at + p.size] = p
        t_data = torch.from_numpy(data).to(dev)
        t_desc = torch.from_numpy(_u8(desc).copy()).to(dev)
        t_iq = torch.zeros(n_iq * 2, dtype=torch.float32, device=dev)
        t_comp = torch.full((n_iq * 2,), float("nan"), dtype=torch.float32, device=dev)
        t_meta = torch.zeros(frames * 32, dtype=torch.uint8, device=dev)
        t_out = torch.full(((units + GUARD) * 16,), 0xAB, dtype=torch.uint8, device=dev)
        d.tx_ragged(t_data, t_desc, frames, t_iq, None, 1.0, 0x12, stream=s.cuda_stream, iq_samples=n_iq,
                    out_syms=n_sym)
        d.estimate_ragged(t_iq, t_desc, frames, est_samples, t_meta, stream=s.cuda_stream, iq_samples=n_iq)
        d.compensate_ragged(t_iq, t_comp, t_desc, frames, t_meta, stream=s.cuda_stream, iq_samples=n_iq)
        d.detect_ragged(t_comp, t_desc, frames, t_out, 0, lphy.DET_DECHIRP, stream=s.cuda_stream, iq_samples=n_iq,
                        units=units)
        s.synchronize()
    out = t_out.cpu().numpy()
    assert (out[units * 16:] == 0xAB).all()
    d.close()
    return desc, out[: units * 16].view(lphy.DETECT_DTYPE).copy()


def oracle_chain(oracle, lphy, payload, est_symbols):
    """(symbols, estimate, records) of the oracle's estimate_offsets (over
    est_symbols symbols, 0: the whole frame) -> compensate_offsets -> detect
    on one frame alone."""
    sf, N = 7, 128
    syms = oracle.encode(payload.tobytes())
    x = oracle.modulate(syms, sf)
    est = oracle.estimate_offsets(x[: est_symbols * N] if est_symbols else x, sf)
    comp = oracle.compensate_offsets(x, sf, float(est[0]), float(est[1]), 1)
    return syms, est, dc.expected(oracle, lphy, comp, sf, 0, N, 1, x.size // N, True, False)


def test_chain_on_one_table(oracle, lphy):
    """Seven frames of 4 to 34 symbols, estimate on the two sync symbols:
    per frame the records are the oracle's chain on that frame alone."""
    rng = np.random.default_rng(77)
    payloads = [rng.integers(0, 256, n, dtype=np.uint8) for n in CHAIN_LENS]
    desc, got = run_chain(lphy, payloads, 2 * 128)
    for f, p in enumerate(payloads):
        _, _, want = oracle_chain(oracle, lphy, p, 2)
        u = int(desc["unit_offset"][f])
        dc.assert_records_equal(got[u: u + want.size], want, f"frame {f}")


def test_chain_data_symbols_are_the_transmitted(oracle, lphy):
    """The records equal the oracle's chain, and the data symbols' peak bins
    equal the transmitted symbols.

    The second holds only for frames that the reference's own chain leaves in
    place, and the payloads are chosen for that, on the oracle alone.
    estimate_offsets reads the raw, undechirped symbols (phy.cpp:100-123),
    whose spectrum is flat, so what it returns for a clean frame is no offset
    of that frame: with the estimate on the two sync symbols every frame gets
    cfo = 0.5226237, time_offset = -42.668945 (and none of the 256 sync
    words gives one that leaves it in place), the compensation advances it by 43 samples
    and every peak lands about 43 bins off, in the oracle as on the device
    (test_chain_on_one_table's frames).  With the estimate over the whole
    frame (est_samples = 0) the result depends on the payload; of the seeds
    0..99,999 per length of 1, 2, 3, 4, 5, 6 and 8 bytes the oracle's chain
    keeps every data symbol for 704 payloads of 2 bytes and 6 of 5 bytes and
    for no other.  KEPT takes frames of both lengths (6 and 12 symbols) in
    turn; that the oracle's estimate leaves them in place (|time_offset| <
    0.5 sample, 0 <= cfo < 0.5 bin) is asserted here before the device's
    records are looked at."""
    payloads = [np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8) for n, seed in KEPT]
    desc, got = run_chain(lphy, payloads, 0)
    for f, p in enumerate(payloads):
        syms, est, want = oracle_chain(oracle, lphy, p, 0)
        assert round(float(est[1])) == 0 and 0.0 <= est[0] < 0.5, f"frame {f}: the oracle's estimate {est}"
        u = int(desc["unit_offset"][f])
        dc.assert_records_equal(got[u: u + want.size], want, f"frame {f}")
        np.testing.assert_array_equal(got["index"][u + 2: u + 2 + syms.size], syms, err_msg=f"frame {f}: data symbols")


# ---- 8. return codes --------------------------------------------------------------
def test_return_codes(lphy):
    """In the header's order, all before any device call: the sentinel
    outputs of both forms are unchanged at the end."""
    import torch
    sf, N = 7, 128
    dev = torch.device("cuda:0")
    d2 = lphy.Demodulator(sf, osr=2)
    L = d2.lib
    step = 2 * N
    desc = d2.ragged_layout([3 * step, step], lphy.MODE_DEMODULATE)
    units = int(desc["unit_offset"][-1])
    t_iq = torch.zeros(2 * 4 * step, dtype=torch.float32, device=dev)
    t_desc = torch.from_numpy(_u8(desc).copy()).to(dev)
    t_out = torch.full((units * 16,), 0xAB, dtype=torch.uint8, device=dev)
    h_iq = np.zeros(4 * step, np.complex64)
    h_out = np.full(units * 16, 0xAB, np.uint8)

    def both(ctx, iq_ok, desc_ok, out_ok, frames, phase, flags, table=desc):
        r1 = L.lphy_hip_detect_ragged(ctx, t_iq.data_ptr() if iq_ok else None, t_desc.data_ptr() if desc_ok else None,
                                      frames, phase, t_out.data_ptr() if out_ok else None, flags, None)
        r2 = L.lphy_hip_detect_ragged_host(ctx, h_iq.ctypes.data if iq_ok else None,
                                           table.ctypes.data if desc_ok else None, frames, phase,
                                           h_out.ctypes.data if out_ok else None, flags)
        assert r1 == r2, (r1, r2)
        return r1

    c = d2.ctx
    assert both(None, True, True, True, 2, 0, 0) == EINVAL          # 1. null ctx ...
    assert both(None, True, True, True, 0, 0, 0) == EINVAL          # ... before frames == 0
    assert both(c, False, False, False, 0, 9, 0xF0) == 0            # 2. frames == 0 before everything else
    assert both(c, False, True, True, 2, 0, 0) == EINVAL            # 3. null pointers,
    assert both(c, True, False, True, 2, 0, 0) == EINVAL
    assert both(c, True, True, False, 2, 0, 0) == EINVAL
    assert both(c, True, True, True, 2, 0, 2) == EINVAL             #    an unknown flag bit,
    assert both(c, True, True, True, 2, 0, 0x80000001) == EINVAL
    assert both(c, True, True, True, 2, 2, 0) == EINVAL             #    phase == osr
    assert both(c, True, True, True, 2, 0xFFFFFFFF, 1) == EINVAL
    assert both(c, True, True, True, 2 ** 31, 2, 0) == EINVAL       #    ... before 4.
    assert both(c, True, True, True, 2 ** 31, 1, 1) == ERANGE       # 4. frames >= 2^31
    assert both(c, True, True, True, 2 ** 40, 0, 0) == ERANGE
    d6 = lphy.Demodulator(6)
    assert both(d6.ctx, True, True, True, 2, 0, 0) == ENOTSUP       # 5. SF < 7
    assert both(d6.ctx, True, True, True, 2 ** 31, 0, 0) == ERANGE  #    ... after 4.
    assert both(d6.ctx, True, True, True, 2, 1, 0) == EINVAL        #    (osr 1: phase 1 is out of range)
    d6.close()

    # the host form's table check
    def host(table, ctx=c, out=h_out):
        return L.lphy_hip_detect_ragged_host(ctx, h_iq.ctypes.data, table.ctypes.data, table.size - 1, 0,
                                             out.ctypes.data, 0)
    bad = desc.copy()
    bad["samples"][1] = 2 ** 31
    assert host(bad) == ERANGE
    bad = desc.copy()
    bad["iq_offset"][0] = 2 ** 48 + 1
    assert host(bad) == ERANGE
    d1 = lphy.Demodulator(sf)   # the ragged demodulator takes osr 1 only: compare there
    good = d1.ragged_layout([3 * N, 0, N], lphy.MODE_DEMODULATE)
    h_meta = np.zeros(3, lphy.META_DTYPE)
    h_syms = np.zeros(8, np.uint16)
    for field, f, v in (("unit_offset", 1, 2), ("unit_offset", 3, 5), ("unit_offset", 0, 1)):
        bad = good.copy()
        bad[field][f] = v
        demod = L.lphy_hip_demod_ragged_host(d1.ctx, h_iq.ctypes.data, bad.ctypes.data, 3, h_syms.ctypes.data, None,
                                             h_meta.ctypes.data, lphy.MODE_DEMODULATE, 0)
        assert host(bad, d1.ctx) == demod == EINVAL
    # a prefix that is right for osr 1 is wrong for this context's step
    assert host(good, d1.ctx, np.zeros(4, lphy.DETECT_DTYPE)) == 0
    assert host(good) == EINVAL
    d1.close()
    torch.cuda.synchronize()
    assert (t_out.cpu().numpy() == 0xAB).all() and (h_out == 0xAB).all()
    # the binding: a record buffer one record short
    short = torch.zeros((units - 1) * 16, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="out"):
        d2.detect_ragged(t_iq, t_desc, 2, short, units=units)
    with pytest.raises(lphy.LphyError) as e:
        d2.detect_ragged_host(h_iq, desc, phase=2)
    assert e.value.rc == EINVAL
    n = C.c_ulonglong(7)
    assert L.lphy_hip_detect_serial_count(c, C.byref(n), 0) == 0 and n.value == 0
    d2.close()
