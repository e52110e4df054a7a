"""CPU-side foundations of tests/test_gpu_detect.py (no GPU):

* the helper that builds a window's expected input (tests/detect_cases.py:
  the strided slice, oracle.dechirp on the N-sample slice, the Hann table
  from glibc cosf in float32 steps) feeds orc_detect and the reference's own
  LoRaDetector the same thing: orc_detect == reference.detect on those
  inputs, bit for bit (skipped when oracle/_ref is absent);
* the Hann restatement is pinned against the oracle: for a one-symbol mode-1
  frame of amplitude <= 1 with hann=True, lora_demodulate's cfo is
  (idx + findex) / N of orc_detect on the table-windowed symbol;
* the fixture sets have the properties the GPU test relies on: in every
  window of the clean-tone set total - maxValue is below 2^-20 of total, so
  no certificate built on a reordered sum can hold and every window must
  take the in-order walk; the noise set has no such window.  (Through the
  Hann window a clean tone spreads over three bins, so the windowed
  clean-tone set has no such window either: there the GPU test asserts what
  it asserts of the noise set.)
"""
import numpy as np
import pytest

import detect_cases as dc


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or _bits(a) == _bits(b)


@pytest.mark.parametrize("sf", dc.SFS)
@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("dechirp", [False, True])
def test_window_input_helper_against_reference(oracle, reference, sf, hann, dechirp):
    N = 1 << sf
    cases = []
    for noisy in (True, False):
        iq = dc.detector_feed(oracle, dc.packets(oracle, sf, noisy), sf, dechirp)
        cases += [(iq, 0, N, 1, w) for w in range(3)]
        cases += [(iq, 5, N // 4, 1, w) for w in (0, 1, 6)] + [(iq, 5, 1, 1, 3)]
    iq2 = dc.packets(oracle, sf, True, osr=2)
    cases += [(iq2, 2 * N, 1, 2, t) for t in range(2)]
    special = np.zeros(3 * N, np.complex64)
    special[N:2 * N] = 0.5
    special[N + 3] = np.complex64(complex(np.inf, 0.0))
    cases += [(special, 0, N, 1, w) for w in range(3)]
    for iq, first, hop, step, w in cases:
        x = dc.window_input(oracle, iq, sf, first, hop, step, w, dechirp, hann)
        oi, op, opa, ofi, obins = dc.orc_detect(oracle, x)
        ri, rp, rpa, rfi, rbins = reference.detect(x)
        assert oi == ri
        assert _same(op, rp) and _same(opa, rpa) and _same(ofi, rfi), (sf, hann, dechirp, first, hop, step, w)
        fin = np.isfinite(rbins.view(np.float32))
        np.testing.assert_array_equal(obins.view(np.uint32)[fin], rbins.view(np.uint32)[fin])


@pytest.mark.parametrize("sf", dc.SFS)
def test_hann_table_pinned_by_lora_demodulate(oracle, sf):
    N = 1 << sf
    rng = np.random.default_rng(sf)
    for k in range(6):
        tone = np.exp(2j * np.pi * (rng.integers(0, N) + rng.uniform(-0.4, 0.4)) * np.arange(N) / N)
        sym = (rng.uniform(0.2, 0.7) * tone + 0.05 * (rng.standard_normal(N) + 1j * rng.standard_normal(N)))
        sym = sym.astype(np.complex64)
        assert np.abs(sym.view(np.float32)).max() <= 1.0  # no normalisation
        _, _, _, met = oracle.lora_demodulate(sym, sf, hann=True)
        x = dc.window_input(oracle, sym, sf, 0, N, 1, 0, False, True)
        idx, _, _, fi, _ = dc.orc_detect(oracle, x)
        want = np.float32(np.float32(np.float32(idx) + fi) / np.float32(N))
        assert _bits(met[0]) == _bits(want), (sf, k)


@pytest.mark.parametrize("sf", dc.SFS)
@pytest.mark.parametrize("dechirp", [False, True])
def test_fixture_sets_cancel_as_the_gpu_test_assumes(oracle, sf, dechirp):
    N, W = 1 << sf, dc.NOISE_WINDOWS[sf]
    for noisy, hann in ((True, False), (True, True), (False, False), (False, True)):
        iq = dc.detector_feed(oracle, dc.packets(oracle, sf, noisy), sf, dechirp)
        ws = range(W)
        c = np.array([dc.cancellation(oracle, dc.window_input(oracle, iq, sf, 0, N, 1, w, dechirp, hann))
                      for w in ws])
        if not noisy and not hann:
            assert (c < 2.0 ** -20).all(), (sf, c.max())
        else:
            assert (c > 2.0 ** -6).all(), (sf, noisy, hann, c.min())
