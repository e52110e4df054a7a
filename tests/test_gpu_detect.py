"""lphy_hip_detect_batch / lphy_hip_detect_host (csrc/lphy_detect.h): the
reference's LoRaDetector::detect on a batch of windows, every record bit for
bit against orc_detect on the window's input (tests/detect_cases.py, itself
pinned to the reference build by tests/test_detect_cpu.py).

SF 7, 8 (several windows per wavefront), 10 (one) and 12 (four wavefronts per
window); with and without the Hann window and LPHY_DET_DECHIRP.

The serial counter (windows whose power_avg took the in-order walk):
* noise set (-8 dB): at most windows / 64.  The certificate fails when a
  float rounding boundary falls inside an interval of relative width
  2 N 2^-50 around total - maxValue, about N 2^-25 per window; the cap only
  keeps the fast path from being silently absent;
* clean-tone set without the Hann window: total - maxValue is pure
  cancellation in every window (test_detect_cpu.py), no certificate can
  hold: exactly `windows`;
* clean-tone set through the Hann window: the tone spreads over three bins,
  nothing cancels (test_detect_cpu.py): as the noise set.
"""
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ENOTSUP = -22, -34, -95


def _demod(lphy, sf, hann, **kw):
    return lphy.Demodulator(sf, window=lphy.WINDOW_HANN if hann else lphy.WINDOW_NONE, **kw)


def _flags(lphy, dechirp):
    return lphy.DET_DECHIRP if dechirp else 0


@pytest.fixture(scope="module")
def sets(oracle):
    """(sf, noisy) -> the packets, made once."""
    return {(sf, noisy): dc.packets(oracle, sf, noisy) for sf in dc.SFS for noisy in (True, False)}


@pytest.mark.parametrize("sf", dc.SFS)
@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("dechirp", [False, True])
@pytest.mark.parametrize("noisy", [True, False])
def test_fixture_sets(oracle, lphy, sets, sf, hann, dechirp, noisy):
    N, W = 1 << sf, dc.NOISE_WINDOWS[sf]
    iq = dc.detector_feed(oracle, sets[sf, noisy], sf, dechirp)
    d = _demod(lphy, sf, hann)
    d.detect_serial_count(reset=True)
    got = d.detect_host(iq, 0, N, 1, W, _flags(lphy, dechirp))
    n = d.detect_serial_count()
    print(f"sf {sf} hann {hann} dechirp {dechirp} noisy {noisy}: {n} of {W} windows walked in order")
    dc.assert_records_equal(got, dc.expected(oracle, lphy, iq, sf, 0, N, 1, W, dechirp, hann), "set")
    if noisy or hann:
        assert n <= W / 64
    else:
        assert n == W
    d.close()


@pytest.mark.parametrize("sf", [7, 10])
@pytest.mark.parametrize("hop", ["N/4", "1"])
@pytest.mark.parametrize("hann,dechirp", [(False, True), (True, False)])
def test_sliding(oracle, lphy, sets, sf, hop, hann, dechirp):
    N = 1 << sf
    hop = N // 4 if hop == "N/4" else 1
    for noisy in (True, False):
        iq = dc.detector_feed(oracle, sets[sf, noisy][: 3 * N], sf, dechirp)
        first = 5
        W = (3 * N - first - N) // hop + 1
        d = _demod(lphy, sf, hann)
        got = d.detect_host(iq, first, hop, 1, W, _flags(lphy, dechirp))
        dc.assert_records_equal(got, dc.expected(oracle, lphy, iq, sf, first, hop, 1, W, dechirp, hann),
                                f"hop {hop} noisy {noisy}")
        d.close()


@pytest.mark.parametrize("sf", [7, 10])
@pytest.mark.parametrize("osr", [2, 4])
@pytest.mark.parametrize("hann", [False, True])
def test_decimated_osr_phases(oracle, lphy, sf, osr, hann):
    """hop = 1, step = osr, windows = osr: the reference's osr phases of a symbol."""
    from test_gpu_osr import _frames
    N = 1 << sf
    iq = _frames(oracle, sf, osr, 1, 4, seed=sf + osr, snr=-3.0).reshape(-1)
    d = _demod(lphy, sf, hann)
    for dechirp in (False, True):
        for s in (0, 3, iq.size // (N * osr) - 1):
            first = s * N * osr
            got = d.detect_host(iq, first, 1, osr, osr, _flags(lphy, dechirp))
            dc.assert_records_equal(got, dc.expected(oracle, lphy, iq, sf, first, 1, osr, osr, dechirp, hann),
                                    f"symbol {s} dechirp {dechirp}")
    d.close()


@pytest.mark.parametrize("sf", dc.SFS)
@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("dechirp", [False, True])
def test_special_inputs(oracle, lphy, sets, sf, hann, dechirp):
    from pathlib import Path
    N = 1 << sf
    normal = dc.detector_feed(oracle, sets[sf, True][: 2 * N], sf, dechirp)
    a, b = normal[:N], normal[N:]
    raw = np.fromfile(Path(__file__).parent / "golden" / "equal_power_iq.bin", np.complex64)
    tie = np.resize(raw, N).astype(np.complex64)
    nan_w, inf_w = a.copy(), b.copy()
    nan_w[N // 3] = np.complex64(complex(np.nan, 0.25))
    inf_w[N - 2] = np.complex64(complex(-0.5, np.inf))
    iq = np.concatenate([np.zeros(N, np.complex64), tie, a, nan_w, b, inf_w, a])
    W = iq.size // N
    d = _demod(lphy, sf, hann)
    got = d.detect_host(iq, 0, N, 1, W, _flags(lphy, dechirp))
    want = dc.expected(oracle, lphy, iq, sf, 0, N, 1, W, dechirp, hann)
    dc.assert_records_equal(got, want, "special")
    # the all-zero window
    assert got["index"][0] == 0 and got["findex"][0] == 0
    assert got["power"][0] == -np.inf and got["power_avg"][0] == -np.inf
    if not dechirp and not hann:
        assert got["index"][1] == 0  # equal power in bins 0 and N/2: the lowest
    # the neighbours of the NaN and inf windows are what they are alone
    alone = d.detect_host(np.concatenate([a, b, a]), 0, N, 1, 3, _flags(lphy, dechirp))
    np.testing.assert_array_equal(got[[2, 4, 6]].view(np.uint8), alone.view(np.uint8))
    assert np.isfinite(alone["power_avg"]).all()
    d.close()


@pytest.mark.parametrize("sf", dc.SFS)
def test_device_form_matches_host_form_and_stays_in_its_slots(oracle, lphy, sets, sf):
    import torch
    N, W = 1 << sf, min(dc.NOISE_WINDOWS[sf], 37)
    iq = sets[sf, True]
    d = _demod(lphy, sf, True)
    host = d.detect_host(iq, 3, N - 1, 1, W, lphy.DET_DECHIRP)
    dev = torch.device("cuda:0")
    t_iq = torch.from_numpy(iq.view(np.float32).copy()).to(dev)
    t_out = torch.full(((W + 3) * 16,), 0xAB, dtype=torch.uint8, device=dev)
    d.detect_batch(t_iq, iq.size, 3, N - 1, 1, W, t_out, lphy.DET_DECHIRP,
                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = t_out.cpu().numpy()
    np.testing.assert_array_equal(out[: W * 16], host.view(np.uint8))
    assert (out[W * 16:] == 0xAB).all()
    dc.assert_records_equal(host, dc.expected(oracle, lphy, iq, sf, 3, N - 1, 1, W, True, True), "host")
    d.close()


def test_argument_checks(lphy):
    import torch
    sf, N = 7, 128
    d = _demod(lphy, sf, False)
    L = d.lib
    dev = torch.device("cuda:0")
    t_iq = torch.zeros(2 * 4 * N, dtype=torch.float32, device=dev)
    t_out = torch.zeros(8 * 16, dtype=torch.uint8, device=dev)
    h_iq = np.zeros(4 * N, np.complex64)
    h_out = np.zeros(8, lphy.DETECT_DTYPE)
    total = 4 * N

    def both(ctx, iq_ok, out_ok, total, first, hop, step, windows, flags):
        r1 = L.lphy_hip_detect_batch(ctx, t_iq.data_ptr() if iq_ok else None, total, first, hop, step, windows,
                                     t_out.data_ptr() if out_ok else None, flags, None)
        r2 = L.lphy_hip_detect_host(ctx, h_iq.ctypes.data if iq_ok else None, total, first, hop, step, windows,
                                    h_out.ctypes.data if out_ok else None, flags)
        assert r1 == r2, (r1, r2)
        return r1

    assert both(d.ctx, True, True, total, 0, N, 1, 4, 0) == 0
    assert both(d.ctx, True, True, total, 0, N, 1, 0, 0) == 0            # windows == 0
    assert both(d.ctx, True, True, 0, 99, 1, 1, 0, 1) == 0
    assert both(None, True, True, total, 0, N, 1, 4, 0) == EINVAL
    assert both(d.ctx, False, True, total, 0, N, 1, 4, 0) == EINVAL
    assert both(d.ctx, True, False, total, 0, N, 1, 4, 0) == EINVAL
    assert both(d.ctx, True, True, total, 0, 0, 1, 4, 0) == EINVAL        # hop == 0
    assert both(d.ctx, True, True, total, 0, N, 0, 4, 0) == EINVAL        # step == 0
    assert both(d.ctx, True, True, total, 0, N, 1, 4, 2) == EINVAL        # unknown flag bit
    assert both(d.ctx, True, True, total, 0, N, 1, 4, 0x80000001) == EINVAL
    # the last index: first + (windows - 1) * hop + (N - 1) * step
    assert both(d.ctx, True, True, total, 1, N, 1, 4, 0) == ERANGE
    assert both(d.ctx, True, True, total, 1, N, 1, 3, 0) == 0
    assert both(d.ctx, True, True, total, 0, N, 1, 5, 0) == ERANGE
    assert both(d.ctx, True, True, total, 0, 1, 4, 5, 0) == ERANGE        # 4 + 4 (N - 1) = 4N
    assert both(d.ctx, True, True, total, 0, 1, 4, 4, 0) == 0             # last index 4N - 1
    assert both(d.ctx, True, True, total, total, 1, 1, 1, 0) == ERANGE
    assert both(d.ctx, True, True, 0, 0, 1, 1, 1, 0) == ERANGE
    big = 2 ** 64 - 1
    assert both(d.ctx, True, True, total, big, 1, 1, 1, 0) == ERANGE      # no overflow
    assert both(d.ctx, True, True, total, 0, big, 1, 2, 0) == ERANGE
    assert both(d.ctx, True, True, total, 0, 1, big, 1, 0) == ERANGE
    assert both(d.ctx, True, True, total, 0, 2 ** 63, 1, 3, 0) == ERANGE
    assert both(d.ctx, True, True, big, 0, 1, 1, 2 ** 32, 0) == ERANGE    # windows >= 2^32
    assert both(d.ctx, True, True, big, 0, 1, 1, 2 ** 40, 0) == ERANGE
    d.close()
    d6 = lphy.Demodulator(6)
    assert both(d6.ctx, True, True, total, 0, 64, 1, 2, 0) == ENOTSUP     # as the ragged call
    d6.close()
    # the binding raises on them
    d = _demod(lphy, sf, False)
    with pytest.raises(lphy.LphyError) as e:
        d.detect_host(h_iq, 1, N, 1, 4)
    assert e.value.rc == ERANGE
    n = C.c_ulonglong(7)
    assert L.lphy_hip_detect_serial_count(None, C.byref(n), 0) == EINVAL
    assert L.lphy_hip_detect_serial_count(d.ctx, None, 0) == EINVAL
    d.close()


def test_serial_count_accumulates_and_resets(oracle, lphy, sets):
    sf, N = 7, 128
    iq = oracle.dechirp(sets[sf, False][: 8 * N], sf)
    d = _demod(lphy, sf, False)
    d.detect_serial_count(reset=True)
    d.detect_host(iq, 0, N, 1, 8)
    assert d.detect_serial_count(reset=False) == 8
    d.detect_host(iq, 0, N, 1, 5)
    assert d.detect_serial_count(reset=True) == 13
    assert d.detect_serial_count() == 0
    d.close()


@pytest.mark.parametrize("sf", dc.SFS)
def test_bounds_checked_build(oracle, lphy, sets, sf):
    """The test build's index checks (LDS slots, the strided IQ reads, the
    record stores) stay at zero, and its records are the product's."""
    N = 1 << sf
    t = _demod(lphy, sf, True, test_build=True)
    p = _demod(lphy, sf, True, lib_path=lphy.HIP_SO)
    t.bounds_violations(reset=True)
    for noisy in (True, False):
        iq = sets[sf, noisy]
        W = dc.NOISE_WINDOWS[sf]
        for first, hop, step, w, fl in ((0, N, 1, W, lphy.DET_DECHIRP), (7, 3, 1, 41, 0),
                                        (1, 1, 2, (iq.size - 2 - 2 * (N - 1)) // 64, lphy.DET_DECHIRP)):
            w = min(w, 64)
            a = t.detect_host(iq, first, hop, step, w, fl)
            b = p.detect_host(iq, first, hop, step, w, fl)
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    # the last window ends on the buffer's last sample
    iq = sets[sf, True]
    t.detect_host(iq, iq.size - N - 2, 1, 1, 3, 0)
    assert t.bounds_violations() == 0
    t.close()
    p.close()
