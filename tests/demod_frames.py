"""Frame builders and checks the demodulator's GPU tests share
(test_gpu_spec.py, test_gpu_certificate.py, test_gpu_parseval.py,
test_gpu_fast_rotation.py, test_gpu_separate_sf11_12.py): one copy each, so a
test of another launch path meets the same frames.
`oracle` is the session's tests/checkers.py Oracle."""
import numpy as np


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def two_tone_frames(oracle, sf, nf, seed):
    """Mode 0 / 2 input: every data symbol two modulated tones (symbols a and
    b) whose amplitude ratio is 1 + k 2^-23 (tone b larger or smaller), k
    swept geometrically from 1 to 2^10 over the frame's 64 symbols, under a
    CFO of up to +-0.4 bin, a roll of up to +-N/4 and gains 0.7 / 1.0 / 1.9."""
    rng = np.random.default_rng(seed)
    N = 1 << sf
    S = 64
    ks = np.unique(np.round(2.0 ** np.linspace(0, 10, S)).astype(np.int64))
    frames = []
    for f in range(nf):
        a = rng.integers(0, 256, S).astype(np.uint16) % N
        b = (a + rng.integers(1, N, S)).astype(np.uint16) % N
        xa = oracle.modulate(a, sf).astype(np.complex128)
        xb = oracle.modulate(b, sf).astype(np.complex128)
        # per-symbol amplitude ratio 1 + k 2^-23 (tone b larger or smaller)
        k = ks[(np.arange(S) + f) % ks.size]
        r = 1.0 + k * 2.0 ** -23
        gain_b = np.ones(xa.size)
        for s in range(S):
            gain_b[(s + 2) * N:(s + 3) * N] = r[s] if (s + f) % 2 else 1.0 / r[s]
        x = xa + xb * gain_b
        t = np.arange(x.size)
        x = x * np.exp(2j * np.pi * rng.uniform(-0.4, 0.4) / N * t) * [0.7, 1.0, 1.9][f % 3]
        x = np.roll(x, int(rng.integers(-N // 4, N // 4 + 1)))
        frames.append(x.astype(np.complex64))
    return np.stack(frames)


def tones_frame(oracle, sf, gains, seed, cfo=0.2, roll=True):
    """One frame whose every data symbol is len(gains) tones (distinct
    random bins) with relative amplitudes `gains` (a callable of the symbol
    index giving the list), under a small CFO and delay."""
    rng = np.random.default_rng(seed)
    N = 1 << sf
    S = 64
    base = rng.integers(0, N, S)
    x = None
    g0 = gains(0)
    for t in range(len(g0)):
        # side tone t in its own part of the spectrum (never on another tone)
        off = 0 if t == 0 else int(rng.integers((2 * t - 1) * N // 8, 2 * t * N // 8 + 1))
        syms = ((base + off) % N).astype(np.uint16)
        xt = oracle.modulate(syms, sf).astype(np.complex128)
        g = np.ones(xt.size)
        for s in range(S):
            g[(s + 2) * N:(s + 3) * N] = gains(s)[t]
        if t > 0:
            g[:2 * N] = 0.0  # the sync symbols: one tone
        x = xt * g if x is None else x + xt * g
    n = np.arange(x.size)
    x = x * np.exp(2j * np.pi * rng.uniform(-cfo, cfo) / N * n)
    if roll:
        x = np.roll(x, int(rng.integers(-N // 8, N // 8 + 1)))
    return x.astype(np.complex64)


def pure_tone_frame(sf, amps, gains, seed, nsym=64):
    """Mode-1 input (dechirped samples) built directly: two sync symbols of
    one tone each, then data symbols of len(amps) pure integer tones at
    distinct random bins, tone t of symbol s with amplitude amps[t] *
    gains(s)[t].  No wrap-around phase step (a modulated chirp's dechirp
    has one, which leaks energy out of the peak and breaks an amplitude
    tie), so the peaks are the amplitudes times N."""
    rng = np.random.default_rng(seed)
    N = 1 << sf
    n = np.arange(N)
    tone = lambda k: np.exp(2j * np.pi * k * n / N)
    # both sync symbols at bin 0: the estimate (LoRaDemod.cpp:80-136) then
    # finds cfo 0 and time offset 0, so the data tones stay on integer bins
    # (a fractional rotation would leak each tone into the others' bins and
    # break a tie by far more than the sweeps' ratios)
    out = [tone(0), tone(0)]
    for s in range(nsym):
        bins = rng.choice(N, len(amps), replace=False)
        g = gains(s)
        out.append(sum(amps[t] * g[t] * tone(int(bins[t])) for t in range(len(amps))))
    return np.concatenate(out).astype(np.complex64)


def spec_frames(oracle, sf, nf, seed, tail=0):
    """Frames for each branch of the speculative normalisation, 7 kinds in
    turn (frame f: kind f % 7) under CFO, noise and gains: 0 the maximum in
    the estimate symbols, 1 a spike in a late symbol, 2 a spike inside the
    estimate symbols, 3 the frame's very last sample (with `tail`: of the
    partial symbol), 4 a barely larger late sample, 5 / 6 (odd frames) a NaN
    / an inf late in the frame."""
    rng = np.random.default_rng(seed)
    N = 1 << sf
    base = oracle.modulate(oracle.encode(bytes(range(24))), sf)
    fs = base.size + tail
    t = np.arange(base.size, dtype=np.float64)
    iq = np.zeros((nf, fs), np.complex64)
    for f in range(nf):
        x = base * np.exp(2j * np.pi * rng.uniform(-0.45, 0.45) / N * t)
        x = x + [0.0, 0.02, 0.3][f % 3] * (rng.standard_normal(base.size) + 1j * rng.standard_normal(base.size))
        x = x * [1.0, 0.7, 2.5, 1.3][f % 4]
        iq[f, :base.size] = x.astype(np.complex64)
        if tail:
            iq[f, base.size:] = (0.1 * rng.standard_normal(tail)).astype(np.complex64)
        kind = f % 7
        S = base.size // N
        if kind == 1:    # spike in a late symbol
            iq[f, int(rng.integers(3 * N, S * N))] *= np.complex64(4.0)
        elif kind == 2:  # spike inside the estimate symbols
            iq[f, int(rng.integers(0, 2 * N))] *= np.complex64(4.0)
        elif kind == 3:  # the frame's very last sample / the partial symbol
            iq[f, fs - 1] = np.complex64(complex(6.0, -1.0))
        elif kind == 4:  # a barely larger sample late (scale differs in the last bits)
            j = int(rng.integers(2 * N, S * N))
            iq[f, j] = iq[f, j] * np.complex64(1.0 + 1e-6) + np.complex64(0.001)
        elif kind == 5 and f % 2:
            iq[f, int(rng.integers(2 * N, S * N))] = np.complex64(complex(np.nan, 1.0))
        elif kind == 6 and f % 2:
            iq[f, int(rng.integers(2 * N, S * N))] = np.complex64(complex(np.inf, 0.0))
    return iq


def impaired_frames(oracle, sf, nf, seed, plen=32, snr_db=None, cfo_bins=0.4, gain=(1.0,),
                    max_delay=0):
    rng = np.random.default_rng(seed)
    N = 1 << sf
    frames = []
    for f in range(nf):
        p = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
        x = oracle.modulate(oracle.encode(p), sf).astype(np.complex128)
        t = np.arange(x.size)
        x = x * np.exp(2j * np.pi * rng.uniform(-cfo_bins, cfo_bins) / N * t)
        if max_delay:
            x = np.roll(x, int(rng.integers(-max_delay, max_delay + 1)))
        if snr_db is not None:
            s = np.sqrt(10 ** (-snr_db / 10) / 2)
            x = x + s * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
        frames.append((x * gain[f % len(gain)]).astype(np.complex64))
    return np.stack(frames)


def fast_and_exact(lphy, d, iq, mode, flags=0):
    """The product library's run and the exact rotation's (test build:
    LPHY_F_EXACT_ROTATION is not in the product library), both with the
    further `flags`; every output bit must agree."""
    nf, fs = iq.shape
    a = d.demod_host(iq, nf, fs, mode, lphy.F_DECODE | flags)
    n_fast = d.recheck_count(reset=True)
    dt = lphy.Demodulator(d.sf, d.bw_hz, d.osr, d.window, test_build=True)
    b = dt.demod_host(iq, nf, fs, mode, lphy.F_DECODE | lphy.F_EXACT_ROTATION | flags)
    n_exact = dt.recheck_count(reset=True)
    assert dt.bounds_violations() == 0
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2].view(np.uint8), b[2].view(np.uint8))
    return a, n_fast, n_exact


def assert_straddle(rows, nsym, thr):
    """Frames below the predicted threshold re-run every data symbol,
    frames above it none, the switch within a factor 2 of the prediction."""
    msg = "\n".join(f"r-1 {k:.4g}: exact {n}" for k, n in rows) + f"\npredicted r-1 {thr:.4g}"
    assert all(0 <= n <= nsym for _, n in rows), msg
    near = [(k, n) for k, n in rows if k < 16 * thr]
    certified = sum(nsym - n for _, n in near)
    rerun = sum(n for _, n in near)
    assert certified > 0 and rerun > 0, msg
    all_rerun = [k for k, n in rows if n == nsym]
    none_rerun = [k for k, n in rows if n == 0]
    assert all_rerun and none_rerun, msg
    assert max(all_rerun) < min(none_rerun) < 16 * thr, msg
    assert thr / 2 < max(all_rerun) and min(none_rerun) < 2 * thr, msg
