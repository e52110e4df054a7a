"""Speculative normalisation of the fused kernels (modes 1/2: k_wave at SF
7-12, which every row of test_speculative_normalisation runs today - units
spanning frames at SF 7-10, SF 5 on k_frames - and k_frames where the rows
below force it): the
frame is estimated with the max-abs of its first two symbols, each symbol
unit folds its own samples' max-abs, and the frame end either confirms the
normalisation or settles the frame in k_post (exact estimate + certificate
check against the exact rate, else the whole-frame re-run).  The separate
launches' form of it at SF 11-12 (DemodArgs::spec_big, k_spec_settle) is
tests/test_gpu_separate_sf11_12.py's.  Every output
bit against the oracle (LoRaDemod.cpp:50-197) and against the pre-scan
schedule (LPHY_F_SCAN_FIRST), on frames built to take each branch:
  - the maximum inside the two estimate symbols (confirmed),
  - a larger sample late in the frame (settled: exact scale, exact rate),
  - CFO so that the time shift is negative or positive (the samples no
    symbol window covers are scanned at the frame end),
  - mode 1 frames with a partial last symbol holding the maximum,
  - NaN / inf late in the frame (whole-frame re-run),
  - no-scratch frames (the speculation is off: -ERANGE as the reference)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


from demod_frames import bits as _bits, spec_frames as _build  # noqa: E402


@pytest.mark.parametrize("sf,nf", [(7, 515), (5, 301), (8, 203), (9, 97), (10, 41), (11, 29), (12, 15)])
@pytest.mark.parametrize("mode", [1, 2])
def test_speculative_normalisation(oracle, lphy, sf, nf, mode):
    tail = (1 << sf) // 2 + 3 if mode == 1 else 0  # a partial last symbol
    iq = _build(oracle, sf, nf, seed=sf * 31 + mode, tail=tail)
    fs = iq.shape[1]
    d = lphy.Demodulator(sf)
    a = d.demod_host(iq, nf, fs, mode, lphy.F_DECODE)
    dt = lphy.Demodulator(sf, test_build=True)  # the pre-scan schedule: test build only
    b = dt.demod_host(iq, nf, fs, mode, lphy.F_DECODE | lphy.F_SCAN_FIRST)
    assert dt.bounds_violations() == 0
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2].view(np.uint8), b[2].view(np.uint8))
    for f in range(0, nf, max(1, nf // 60)):
        src = iq[f] if mode == 1 else oracle.dechirp(iq[f], sf)
        r, osyms, osync, omet = oracle.lora_demodulate(src, sf)
        ctx = f"sf {sf} mode {mode} frame {f}"
        assert a[2]["status"][f] == 0, ctx
        np.testing.assert_array_equal(a[0][f], osyms, err_msg=ctx)
        assert a[2]["sync_word"][f] == osync, ctx
        assert _bits(a[2]["cfo"][f]) == _bits(omet[0]), ctx
        assert _bits(a[2]["time_offset"][f]) == _bits(omet[1]), ctx


@pytest.mark.parametrize("sf", [9, 10])
@pytest.mark.parametrize("how", ["hann", "exact_rotation", "frames_hann"])
def test_estimate_maxabs_in_symbol0(oracle, lphy, sf, how):
    """Frames whose max-abs lies in sync symbol 0, with symbol 1's own
    maximum smaller but still > 1: both estimate units must be scaled by the
    frame's (symbol 0's) maximum, LoRaDemod.cpp:60-78.  LPHY_F_EXACT_ROTATION
    routes SF 9-10 modes 1/2 to k_frames (csrc/lphy_route.h), whose EB tiles
    fold the estimate symbols' max-abs only when both units share a tile
    (SF <= 9); at SF 10 the two-symbol scan must supply it.  "hann": the
    windowed k_wave, units spanning frames, whose estimate unit holds both
    symbols of a frame.  "frames_hann": LPHY_F_FRAMES_KERNEL (test build)
    keeps the windowed frames on k_frames, its EB-tile path with the window,
    which the product takes for frames shorter than a wave unit."""
    N = 1 << sf
    rng = np.random.default_rng(1000 + sf)
    base = oracle.modulate(oracle.encode(bytes(range(12))), sf)
    t = np.arange(base.size, dtype=np.float64)
    nf = 24
    iq = np.zeros((nf, base.size), np.complex64)
    for f in range(nf):
        x = base * np.exp(2j * np.pi * rng.uniform(-0.4, 0.4) / N * t) * (1.5 + 0.1 * (f % 5))
        x = x + 0.05 * (rng.standard_normal(base.size) + 1j * rng.standard_normal(base.size))
        x = x.astype(np.complex64)
        j = int(rng.integers(0, N))
        x[j] = np.complex64(complex(3.0 + 0.25 * (f % 4), -0.5))  # the frame's maximum, symbol 0
        iq[f] = x
    hann = how != "exact_rotation"
    window = lphy.WINDOW_HANN if hann else lphy.WINDOW_NONE
    flags = lphy.F_DECODE | {"hann": 0, "exact_rotation": lphy.F_EXACT_ROTATION,
                             "frames_hann": lphy.F_FRAMES_KERNEL}[how]
    d = lphy.Demodulator(sf, window=window, test_build=how != "hann")
    syms, _, meta = d.demod_host(iq, nf, iq.shape[1], 2, flags)
    for f in range(nf):
        dech = oracle.dechirp(iq[f], sf)
        m0 = np.max(np.maximum(np.abs(dech[:N].real), np.abs(dech[:N].imag)))
        m1 = np.max(np.maximum(np.abs(dech[N:2 * N].real), np.abs(dech[N:2 * N].imag)))
        assert m0 > m1 > 1.0
        r, osyms, osync, omet = oracle.lora_demodulate(dech, sf, hann=hann)
        ctx = f"sf {sf} {how} frame {f}"
        assert meta["status"][f] == 0, ctx
        assert _bits(meta["cfo"][f]) == _bits(omet[0]), ctx
        assert _bits(meta["time_offset"][f]) == _bits(omet[1]), ctx
        assert meta["sync_word"][f] == osync, ctx
        np.testing.assert_array_equal(syms[f], osyms, err_msg=ctx)


def test_speculation_off_without_scratch(oracle, lphy):
    sf = 7
    iq = _build(oracle, sf, 64, seed=5)
    d = lphy.Demodulator(sf)
    syms, _, meta = d.demod_host(iq, 64, iq.shape[1], 2, lphy.F_NO_SCRATCH)
    for f in range(64):
        dech = oracle.dechirp(iq[f], sf)
        mx = np.max(np.maximum(np.abs(dech.real), np.abs(dech.imag)))
        if mx > 1.0:
            assert meta["status"][f] == -34
        elif np.isfinite(iq[f]).all():
            r, osyms, osync, omet = oracle.lora_demodulate(dech, sf)
            np.testing.assert_array_equal(syms[f], osyms)
