"""Adversarial near-ties for the certified fast path.

Symbol units of the fused kernels do not run KISS's exact arithmetic: they
rotate with a per-frame table and (k_wave) 64th-root twiddles, and prove
the argmax with a certificate (|X_best| - 4B > |X_second|); a symbol the
certificate cannot prove is re-run exactly (k_post).  If the bound B were
too small, a near-tie could flip silently.  These frames are built to sit
on both sides of the threshold: every data symbol is two tones (symbols a
and b, the reference's strict `>` with the first maximum winning,
LoRaDetector.hpp:46-58) whose amplitude ratio is 1 + k 2^-23, k swept
geometrically from 1 to 2^10 over the frame's symbols, under CFO and delay.
Every output (symbols, sync word, cfo / time_offset bits) must equal the
oracle's, and lphy_hip_recheck_count must show the exact re-run fired.

Kernels: SF 7-12 k_wave (with and without the Hann window; SF 7-9 with
units spanning frames); SF 7-9 also k_frames (the test build's
LPHY_F_FRAMES_KERNEL), which the product takes for frames shorter than a
wave unit.  (Round 6 removed k_frames' f16 matrix-core symbol tiles: same-box
A/B on those frames within 0.5-2 %)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


from demod_frames import (assert_straddle as _assert_straddle, bits as _bits,  # noqa: E402
                          two_tone_frames as _two_tone_frames)


@pytest.mark.parametrize("sf,nf", [(7, 48), (8, 24), (9, 20), (11, 6), (12, 4)])
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("kernel", ["default", "hann", "frames"])
def test_near_ties_straddling_the_certificate(oracle, lphy, sf, nf, mode, kernel):
    hann = kernel == "hann"
    if kernel == "frames" and sf > 9:
        pytest.skip("k_frames: SF <= 10")
    iq = _two_tone_frames(oracle, sf, nf, seed=sf * 13 + mode + 7 * hann)
    d = lphy.Demodulator(sf, window=lphy.WINDOW_HANN if hann else lphy.WINDOW_NONE,
                         test_build=kernel == "frames")
    flags = lphy.F_DECODE | (lphy.F_FRAMES_KERNEL if kernel == "frames" else 0)
    d.recheck_count(reset=True)
    syms, _, meta = d.demod_host(iq, nf, iq.shape[1], mode, flags)
    n_exact = d.recheck_count(reset=True)
    for f in range(nf):
        if mode == 0:
            r, osyms, osync, omet = oracle.demodulate(iq[f], sf, hann=hann)
        else:
            r, osyms, osync, omet = oracle.lora_demodulate(oracle.dechirp(iq[f], sf), sf, hann=hann)
        ctx = f"sf {sf} mode {mode} hann {hann} frame {f}"
        assert meta["status"][f] == 0, ctx
        np.testing.assert_array_equal(syms[f], osyms, err_msg=ctx)
        assert meta["sync_word"][f] == osync, ctx
        assert _bits(meta["cfo"][f]) == _bits(omet[0]), ctx
        assert _bits(meta["time_offset"][f]) == _bits(omet[1]), ctx
    # the sweep reaches margins far below the bound: some symbols must have
    # gone to the exact re-run, and far above it: not all of them
    assert 0 < n_exact < nf * 66, f"{n_exact} exact re-runs of {nf * 66} symbols"
    if kernel == "frames":
        # the same frames through the product library (its k_wave), bit for bit
        dp = lphy.Demodulator(sf)
        psyms, _, pmeta = dp.demod_host(iq, nf, iq.shape[1], mode, lphy.F_DECODE)
        np.testing.assert_array_equal(psyms, syms)
        np.testing.assert_array_equal(pmeta.view(np.uint8), meta.view(np.uint8))


def _pure_two_tone_frame(sf, ratio, seed, nsym=64):
    """Mode-1 input (dechirped samples) built directly: sync symbols at bin
    0 (the estimate finds cfo 0, time offset 0), then data symbols of two
    pure integer tones of amplitude 1/2 and ratio / 2 (or 1 / ratio / 2),
    so the two peaks differ by the ratio alone (a modulated chirp's dechirp
    has a wrap-around phase step that leaks energy and breaks ties by much
    more)."""
    rng = np.random.default_rng(seed)
    N = 1 << sf
    n = np.arange(N)
    tone = lambda k: np.exp(2j * np.pi * k * n / N)
    out = [tone(0), tone(0)]
    for s in range(nsym):
        a, b = rng.choice(N, 2, replace=False)
        g = ratio if s % 2 else 1.0 / ratio
        out.append(0.5 * tone(int(a)) + 0.5 * g * tone(int(b)))
    return np.concatenate(out).astype(np.complex64)


@pytest.mark.parametrize("sf", [7, 8])
def test_frames_kernel_threshold_straddled(oracle, lphy, sf):
    """SF 7-8 modes 1/2 in k_frames (frames shorter than a wave unit, or any
    frame with the test build's LPHY_F_FRAMES_KERNEL): its symbol tiles'
    certificate, cert_bound's B with no extra charge (the per-frame rotation
    table of SF <= 8): with A = N sqrt2 and two tones of amplitude 1/2, a
    lead N (r - 1) / 2 must exceed 4 B, i.e. r - 1 > ~5e-5.  One frame per
    call (mode 1), every data symbol two pure tones at a constant ratio r,
    r - 1 swept geometrically from 2^-20 to 2^-8: frames below the
    threshold re-run every data symbol exactly, frames above it certify
    every one, the switch lies within a factor 2 of the predicted threshold,
    and near-tie symbols are counted on both sides.  Every output bit
    equals the oracle's."""
    N = 1 << sf
    L = (sf + 1) // 2
    thr = 4.0 * 2.0 ** -24 * np.sqrt(2.0) * (24 + 12 * L) * 1.001 / 0.5  # r - 1 at the bound
    ks = 2.0 ** np.linspace(-20, -8, 37)
    d = lphy.Demodulator(sf, test_build=True)  # (k_frames: LPHY_F_FRAMES_KERNEL)
    rows = []
    for i, k in enumerate(ks):
        x = _pure_two_tone_frame(sf, 1.0 + k, seed=4000 + 97 * sf + i)
        d.recheck_count(reset=True)
        syms, _, meta = d.demod_host(x[None, :], 1, x.size, 1, lphy.F_DECODE | lphy.F_FRAMES_KERNEL)
        n_exact = d.recheck_count(reset=True)
        r, osyms, osync, omet = oracle.lora_demodulate(x, sf)
        ctx = f"sf {sf} r-1 {k:.3g}"
        assert meta["status"][0] == 0, ctx
        np.testing.assert_array_equal(syms[0], osyms, err_msg=ctx)
        assert meta["sync_word"][0] == osync, ctx
        assert _bits(meta["cfo"][0]) == _bits(omet[0]), ctx
        assert _bits(meta["time_offset"][0]) == _bits(omet[1]), ctx
        rows.append((k, n_exact))
    _assert_straddle(rows, 64, thr)
    # The product library (lib/liblphy_hip.so) takes k_frames for frames
    # shorter than a wave unit (4096 / N symbols: k_wave's units span frames
    # only from there, csrc/lphy_route.h): the same sweep on such frames
    # through the shipped code objects, no test flag.
    nsym = {7: 20, 8: 10}[sf]
    dp = lphy.Demodulator(sf)
    rows = []
    for i, k in enumerate(ks):
        x = _pure_two_tone_frame(sf, 1.0 + k, seed=4500 + 97 * sf + i, nsym=nsym)
        dp.recheck_count(reset=True)
        syms, _, meta = dp.demod_host(x[None, :], 1, x.size, 1, lphy.F_DECODE)
        n_exact = dp.recheck_count(reset=True)
        r, osyms, osync, omet = oracle.lora_demodulate(x, sf)
        ctx = f"product sf {sf} r-1 {k:.3g} ({nsym} data symbols)"
        assert meta["status"][0] == 0, ctx
        np.testing.assert_array_equal(syms[0], osyms, err_msg=ctx)
        assert meta["sync_word"][0] == osync, ctx
        assert _bits(meta["cfo"][0]) == _bits(omet[0]), ctx
        assert _bits(meta["time_offset"][0]) == _bits(omet[1]), ctx
        rows.append((k, n_exact))
    _assert_straddle(rows, nsym, thr)


@pytest.mark.parametrize("sf", [7, 8])
def test_frames_kernel_weak_symbols(oracle, lphy, sf):
    """Weak data symbols under loud sync symbols: the
    certificate bounds the transform's error against A with amax = 1, the
    frame normalisation's bound, not the symbol's own amplitude, so a weak
    symbol's lead shrinks against a fixed B and a weak near-tie is re-run.
    Every output bit equals the oracle's across data gains 2^-2 .. 2^-16
    (mode 1, two pure tones at ratio 1.3, sync symbols of amplitude 2)."""
    d = lphy.Demodulator(sf, test_build=True)  # (k_frames: LPHY_F_FRAMES_KERNEL)
    counts = []
    for i, gexp in enumerate([2, 4, 6, 8, 12, 16]):
        x = _pure_two_tone_frame(sf, 1.3, seed=5000 + sf + i).astype(np.complex128)
        N = 1 << sf
        x[:2 * N] *= 2.0
        x[2 * N:] *= 2.0 ** -gexp
        x = x.astype(np.complex64)
        d.recheck_count(reset=True)
        syms, _, meta = d.demod_host(x[None, :], 1, x.size, 1, lphy.F_DECODE | lphy.F_FRAMES_KERNEL)
        counts.append(d.recheck_count(reset=True))
        r, osyms, osync, omet = oracle.lora_demodulate(x, sf)
        ctx = f"sf {sf} gain 2^-{gexp}"
        assert meta["status"][0] == 0, ctx
        np.testing.assert_array_equal(syms[0], osyms, err_msg=ctx)
        assert _bits(meta["cfo"][0]) == _bits(omet[0]), ctx
        assert _bits(meta["time_offset"][0]) == _bits(omet[1]), ctx
    # loud data certify, the weakest re-run every symbol
    assert counts[0] < 64 and counts[-1] == 64, counts
