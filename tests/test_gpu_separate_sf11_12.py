"""The separate launches at SF 11-12 (k_maxabs / k_estimate / k_demod, then
k_spec_settle and k_post): what the library runs there for every batch below
fused_min_frames (384 frames), single packets of the lora_phy:: API included,
while the rest of the suite (tests/conftest.py: fused_min_frames 0) sends SF
11-12 to k_wave.  k_demod's symbol tiles at SF 11-12 are the one place where
the separate path leaves the reference's arithmetic, with two pieces of their
own:

* the two-table certified rotation (lphy_demod.h, FASTB): e^{j rate i} =
  e^{j rate 64h} e^{j rate l}, fft_tile<SF, true>, accepted by
  fast_certified(b2, c, am, 6.0f) - cert_bound's B with 6 u more for the
  second table - with, in mode 0, the team's measured max-abs;
* the speculative normalisation across workgroups (DemodArgs::spec_big, modes
  1/2): k_maxabs scans the two estimate symbols, k_demod folds the rest with
  atomics on a uint4 per frame, k_spec_settle (lphy_post.h) confirms the frame,
  settles it (settle_verdict) or sends it to the whole-frame re-run.

Every comparison is on bits against the oracle, every frame: symbols, sync
word, the cfo / time_offset bit patterns, status, and with LPHY_F_DECODE the
payload bytes and crc_ok.  LPHY_F_UNFUSED forces Path::Separate
(csrc/lphy_route.h, tests/cpp/route_check.cpp); the Parseval counter, which
only k_wave moves, shows which path ran."""
import functools
import math

import numpy as np
import pytest

from demod_frames import (assert_straddle, bits, fast_and_exact, impaired_frames, pure_tone_frame, spec_frames,
                          two_tone_frames)

pytestmark = pytest.mark.gpu

ERANGE = -34


# ---- the oracle's outputs of a batch, once ----------------------------------
def _reference(oracle, x, sf, mode, hann=False, scratch=True):
    if mode == 0:
        r, osyms, osync, omet = oracle.demodulate(x, sf, hann=hann)
    else:
        src = x if mode == 1 else oracle.dechirp(x, sf)
        r, osyms, osync, omet = oracle.lora_demodulate(src, sf, hann=hann, scratch=scratch)
    if r < 0:
        return int(r), None, None, None, None, None
    _, obytes, ocrc = oracle.decode(osyms)
    return int(r), osyms.copy(), osync, omet.copy(), obytes.copy(), ocrc


def _references(oracle, iq, sf, mode, hann=False, scratch=True):
    return [_reference(oracle, x, sf, mode, hann, scratch) for x in iq]


def _check(got, refs, ctx, decode=True):
    """Every frame of a demod_host result against the oracle's."""
    syms, pay, meta = got
    assert len(refs) == len(meta)
    for f, (r, osyms, osync, omet, obytes, ocrc) in enumerate(refs):
        where = f"{ctx} frame {f}"
        if r < 0:
            assert meta["status"][f] == r, where
            continue
        assert meta["status"][f] == 0, where
        np.testing.assert_array_equal(syms[f], osyms, err_msg=where)
        assert meta["sync_word"][f] == osync, where
        assert bits(meta["cfo"][f]) == bits(omet[0]), where
        assert bits(meta["time_offset"][f]) == bits(omet[1]), where
        if decode:
            np.testing.assert_array_equal(pay[f], obytes, err_msg=where)
            assert bool(meta["crc_ok"][f]) == bool(ocrc), where


def _same(a, b, ctx):
    np.testing.assert_array_equal(a[0], b[0], err_msg=ctx)
    np.testing.assert_array_equal(a[1], b[1], err_msg=ctx)
    np.testing.assert_array_equal(a[2].view(np.uint8), b[2].view(np.uint8), err_msg=ctx)


def _dechirped(oracle, iq, sf):
    return np.stack([oracle.dechirp(x, sf) for x in iq])


# ---- 1. the tests run the path they claim -----------------------------------
@functools.lru_cache(maxsize=None)
def _short_frames(oracle, sf, nf):
    """Clean frames of four whole symbols (two sync, two data) under CFO and
    gains, with the oracle's mode-2 outputs."""
    rng = np.random.default_rng(1200 + sf)
    N = 1 << sf
    n = np.arange(4 * N)
    iq = np.empty((nf, 4 * N), np.complex64)
    for f in range(nf):
        x = oracle.modulate(rng.integers(0, N, 2).astype(np.uint16), sf).astype(np.complex128)
        x = x * np.exp(2j * np.pi * rng.uniform(-0.3, 0.3) / N * n) * [1.0, 0.6, 1.7][f % 3]
        iq[f] = x.astype(np.complex64)
    return iq, _references(oracle, iq, sf, 2)


@pytest.mark.parametrize("sf", [11, 12])
def test_unfused_forces_the_separate_launches(oracle, lphy, sf):
    """A clean one-tone frame: k_wave proves its symbols by Parseval, the
    separate launches have no such certificate, so the test build's Parseval
    counter tells the two apart."""
    x = pure_tone_frame(sf, [0.5], lambda s: [1.0], seed=300 + sf, nsym=16)
    refs = _references(oracle, x[None, :], sf, 1)
    dt = lphy.Demodulator(sf, test_build=True)
    dt.parseval_count(reset=True)
    got = dt.demod_host(x[None, :], 1, x.size, 1, lphy.F_DECODE | lphy.F_UNFUSED)
    assert dt.parseval_count(reset=True) == 0
    _check(got, refs, f"sf {sf} unfused")
    fused = dt.demod_host(x[None, :], 1, x.size, 1, lphy.F_DECODE)
    assert dt.parseval_count(reset=True) > 0
    _check(fused, refs, f"sf {sf} fused")
    assert dt.bounds_violations() == 0


@pytest.mark.parametrize("sf", [11, 12])
@pytest.mark.parametrize("nf", [1, 3, 383])
def test_default_route_below_the_crossover(oracle, lphy, sf, nf):
    """The library's own crossover (set_fused_min_frames(-1): 384 frames at SF
    11-12): batches of 1, 3 and 383 frames run the separate launches - no
    symbol proven by Parseval - and give LPHY_F_UNFUSED's bits."""
    iq, refs = _short_frames(oracle, sf, nf)
    fs = iq.shape[1]
    for test_build in (False, True):
        d = lphy.Demodulator(sf, test_build=test_build)
        d.set_fused_min_frames(-1)
        if test_build:
            d.parseval_count(reset=True)
        got = d.demod_host(iq, nf, fs, 2, lphy.F_DECODE)
        if test_build:
            assert d.parseval_count(reset=True) == 0
            assert d.bounds_violations() == 0
        ctx = f"sf {sf} {nf} frames test_build {test_build}"
        _check(got, refs, ctx)
        _same(got, d.demod_host(iq, nf, fs, 2, lphy.F_DECODE | lphy.F_UNFUSED), ctx)
        d.close()


def test_crossover_batch_takes_the_wave_kernel(oracle, lphy):
    """384 frames at SF 11, four whole symbols each: the smallest batch the
    library gives to k_wave on its own, with the separate launches' bits."""
    sf, nf = 11, 384
    iq, refs = _short_frames(oracle, sf, nf)
    fs = iq.shape[1]
    dt = lphy.Demodulator(sf, test_build=True)
    dt.set_fused_min_frames(-1)
    dt.parseval_count(reset=True)
    got = dt.demod_host(iq, nf, fs, 2, lphy.F_DECODE)
    assert dt.parseval_count(reset=True) > 0
    _check(got, refs, "sf 11 384 frames")
    _same(got, dt.demod_host(iq, nf, fs, 2, lphy.F_DECODE | lphy.F_UNFUSED), "384 frames, unfused")
    assert dt.parseval_count(reset=True) == 0
    assert dt.bounds_violations() == 0
    dp = lphy.Demodulator(sf)
    dp.set_fused_min_frames(-1)
    _same(got, dp.demod_host(iq, nf, fs, 2, lphy.F_DECODE), "384 frames, product")


# ---- 2. the two-table certificate straddled ---------------------------------
@pytest.mark.parametrize("sf", [11, 12])
@pytest.mark.parametrize("test_build", [False, True])
def test_two_table_threshold_straddled(oracle, lphy, sf, test_build):
    """One frame per call (mode 1): sync symbols at bin 0 (rate = start = 0),
    16 data symbols of two pure tones of amplitude 1/2 at a constant ratio r
    alternating with 1 / r, r - 1 swept geometrically from 2^-20 to 2^-8.  The
    lead N (r - 1) / 2 meets 4 B, B = cert_bound(0, 0, 1, 6) = u N sqrt2 1.0001
    (24 + 12 L + 6) 1.001 with L = 6, at r - 1 = 6.9e-5: frames below re-run
    every data symbol exactly, frames above none, the switch within a factor 2
    of that (the 6 u of the second table move it by 6 %, less than the window
    can see).  Every output equals the oracle's on both sides, whose symbols
    are the larger tone's bin (checked here first, so the reference is not a
    matter of its own rounding)."""
    N, nsym = 1 << sf, 16
    L = (sf + 1) // 2
    thr = 4.0 * 2.0 ** -24 * np.sqrt(2.0) * 1.0001 * (24 + 12 * L + 6) * 1.001 / 0.5
    d = lphy.Demodulator(sf, test_build=test_build)
    rows = []
    for i, k in enumerate(2.0 ** np.linspace(-20, -8, 37)):
        seed = 6100 + 97 * sf + i
        x = pure_tone_frame(sf, [0.5, 0.5], lambda s, k=k: [1.0, (1.0 + k) if s % 2 else 1.0 / (1.0 + k)],
                            seed=seed, nsym=nsym)
        ref = _reference(oracle, x, sf, 1)
        rng = np.random.default_rng(seed)  # pure_tone_frame's bins
        pairs = [rng.choice(N, 2, replace=False) for _ in range(nsym)]
        larger = [int(b[1]) if s % 2 else int(b[0]) for s, b in enumerate(pairs)]
        np.testing.assert_array_equal(ref[1], larger, err_msg=f"the oracle at r-1 {k:.3g}")
        d.recheck_count(reset=True)
        got = d.demod_host(x[None, :], 1, x.size, 1, lphy.F_DECODE | lphy.F_UNFUSED)
        rows.append((k, d.recheck_count(reset=True)))
        _check(got, [ref], f"sf {sf} r-1 {k:.3g}")
    if test_build:
        assert d.bounds_violations() == 0
    print(f"\nsf {sf} test_build {test_build}: last all-re-run r-1 "
          f"{max([k for k, n in rows if n == nsym], default=0):.4g}, first none-re-run r-1 "
          f"{min([k for k, n in rows if n == 0], default=0):.4g}, predicted {thr:.4g}")
    assert_straddle(rows, nsym, thr)


# ---- 3. near-ties under CFO and delay ---------------------------------------
@functools.lru_cache(maxsize=None)
def _near_ties(oracle, sf, mode, hann):
    nf = {11: 6, 12: 4}[sf]
    iq = two_tone_frames(oracle, sf, nf, seed=sf * 17 + mode + 5 * hann)
    if mode == 1:
        iq = _dechirped(oracle, iq, sf)
    return iq, _references(oracle, iq, sf, mode, hann=hann)


@pytest.mark.parametrize("sf", [11, 12])
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("hann", [False, True])
def test_near_ties_on_the_separate_launches(oracle, lphy, sf, mode, hann):
    """Amplitude ratios 1 + k 2^-23, k = 1 .. 2^10, under CFO +-0.4 bin, a roll
    of +-N/4 and gains 0.7 / 1.0 / 1.9 (in mode 0 the certificate's amax is the
    team's measured max-abs): some symbols certify, some are re-run."""
    iq, refs = _near_ties(oracle, sf, mode, hann)
    nf, fs = iq.shape
    d = lphy.Demodulator(sf, window=lphy.WINDOW_HANN if hann else lphy.WINDOW_NONE)
    d.recheck_count(reset=True)
    got = d.demod_host(iq, nf, fs, mode, lphy.F_DECODE | lphy.F_UNFUSED)
    n_exact = d.recheck_count(reset=True)
    _check(got, refs, f"sf {sf} mode {mode} hann {hann}")
    assert 0 < n_exact < nf * 66, f"{n_exact} exact re-runs of {nf * 66} symbols"


def test_near_ties_sf12_mode1_hann_without_the_flag(oracle, lphy):
    """SF 12, mode 1 with the Hann window: wave_kernel() excludes it, so the
    suite's fused_min_frames 0 reaches the separate launches too."""
    sf = 12
    iq, refs = _near_ties(oracle, sf, 1, True)
    nf, fs = iq.shape
    for test_build in (False, True):
        d = lphy.Demodulator(sf, window=lphy.WINDOW_HANN, test_build=test_build)
        d.recheck_count(reset=True)
        if test_build:
            d.parseval_count(reset=True)
        got = d.demod_host(iq, nf, fs, 1, lphy.F_DECODE)
        n_exact = d.recheck_count(reset=True)
        if test_build:
            assert d.parseval_count(reset=True) == 0
            assert d.bounds_violations() == 0
        _check(got, refs, f"sf 12 mode 1 hann test_build {test_build}")
        assert 0 < n_exact < nf * 66, f"{n_exact} exact re-runs of {nf * 66} symbols"


# ---- 4. fast rotation equals exact rotation ---------------------------------
def _fast_exact_oracle(oracle, lphy, sf, mode, iq, hann=False):
    if mode == 1:
        iq = _dechirped(oracle, iq, sf)
    d = lphy.Demodulator(sf, window=lphy.WINDOW_HANN if hann else lphy.WINDOW_NONE)
    d.recheck_count(reset=True)
    got, n_fast, _ = fast_and_exact(lphy, d, iq, mode, flags=lphy.F_UNFUSED)
    _check(got, _references(oracle, iq, sf, mode, hann=hann), f"sf {sf} mode {mode} hann {hann}")
    return n_fast


@pytest.mark.parametrize("sf", [11, 12])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("snr", [None, -8.0, -16.0, -24.0])
def test_fast_equals_exact_on_the_separate_launches(oracle, lphy, sf, mode, snr):
    nf = {11: 12, 12: 6}[sf]
    iq = impaired_frames(oracle, sf, nf, seed=sf * 37 + mode + int(snr or 0), snr_db=snr,
                         gain=(1.0, 0.3, 2.5), max_delay=3)
    n_fast = _fast_exact_oracle(oracle, lphy, sf, mode, iq)
    if snr is None:
        assert n_fast == 0, n_fast  # clean frames: every symbol certified
    if snr == -24.0:
        assert n_fast > 0


@pytest.mark.parametrize("sf", [11, 12])
def test_fast_equals_exact_hann_big_cfo(oracle, lphy, sf):
    """Hann window, CFO up to +-3 bins and delays of up to 40 samples."""
    iq = impaired_frames(oracle, sf, {11: 12, 12: 6}[sf], seed=9 + sf, snr_db=-12.0, cfo_bins=3.0, max_delay=40)
    for mode in (0, 1, 2):
        _fast_exact_oracle(oracle, lphy, sf, mode, iq, hann=True)


# ---- 5. the branches of k_spec_settle ---------------------------------------
def _maxabs(v):
    return np.maximum(np.abs(v.real), np.abs(v.imag))


def _roundf(x):
    return int(math.copysign(math.floor(abs(float(x)) + 0.5), float(x)))


BUMP = np.float32(1.40625)  # the speculative maximum of the edge frames, at sample 0


@functools.lru_cache(maxsize=None)
def _edge_frames(oracle, sf, mode):
    """Four frames of spec_frames' length (mode 1: with its partial symbol of
    N/2 + 3 samples) that the 7 kinds do not hold; k_maxabs' speculative
    maximum is that of the first two symbols, each frame's time shift the
    oracle's round(time_offset), checked here before anything runs:
      0  the frame's maximum before the first symbol window under a positive
         shift: samples [0, t_off) are read by the two-symbol scan alone;
      1  the only sample above the speculative maximum behind the last symbol
         window under a negative shift: k_spec_settle's frame-end scan alone
         reads [S N - |t_off|, count);
      2  a late spike whose scale moves the time offset across a rounding
         boundary (e.t_off != sm.t_off): the whole frame is re-run;
      3  a late sample above the speculative maximum by one ulp: the scale
         changes in its last bit, settle_verdict stands with d ~ 0.
    Returns (iq, the whole symbols per frame)."""
    N = 1 << sf
    tail = N // 2 + 3 if mode == 1 else 0
    base = oracle.modulate(oracle.encode(bytes(range(24))), sf).astype(np.complex128)
    S = base.size // N
    n = np.arange(base.size)
    down = oracle.dechirp(np.ones(N, np.complex64), sf)

    def view(y):  # what the normalisation's max-abs runs over
        return y if mode == 1 else oracle.dechirp(y, sf)

    solved = {}

    def put(y, j, target):
        """Sample j such that its max-abs under view() is the float `target`
        exactly (mode 2: the input whose float32 dechirp gives it, found
        among the neighbours of target / down[j])."""
        if mode == 1:
            y[j] = np.complex64(complex(target, 0.25))
            return
        if (j, target) in solved:
            y[j] = solved[j, target]
            return
        z0 = np.array([complex(target, 0.25) / complex(down[j % N])], np.complex64).view(np.int32)
        sym = np.zeros(N, np.complex64)
        for da in range(-8, 9):
            for db in range(-8, 9):
                z = (z0 + np.array([da, db], np.int32)).view(np.complex64)[0]
                sym[j % N] = z
                if _maxabs(oracle.dechirp(sym, sf)[j % N:j % N + 1])[0] == target:
                    y[j] = solved[j, target] = z
                    return
        raise AssertionError(f"sf {sf}: no input near sample {j} dechirps to a max-abs of {target!r}")

    def frame(c, upto=None, bump=True):
        m = base.size if upto is None else upto
        x = (base[:m] * np.exp(2j * np.pi * c / N * n[:m]) * 1.3).astype(np.complex64)
        y = oracle.dechirp(x, sf) if mode == 1 else x
        if bump:
            put(y, 0, BUMP)
        if tail and upto is None:
            y = np.concatenate([y, np.zeros(tail, np.complex64)])
        return y

    def t_off(y):
        return _roundf(oracle.lora_demodulate(view(y), sf)[3][1])

    def only_above_spec(y, j):
        m = _maxabs(view(y))
        assert np.flatnonzero(m > m[:2 * N].max()).tolist() == [j], (sf, mode, j)

    out = []
    # 0: positive shift, the maximum inside [0, t_off)
    y = frame(-0.3, bump=False)
    j = t_off(y) // 2
    assert j >= 4
    y[j] *= np.complex64(3.0)
    assert int(_maxabs(view(y)).argmax()) == j < t_off(y)
    out.append(y)
    # 1: negative shift, the spike in [S N - |t_off|, S N)
    y = frame(0.3)
    j = S * N + t_off(y) // 2
    y[j] *= np.complex64(3.0)
    t = t_off(y)
    assert t < 0 and S * N + t <= j < S * N
    only_above_spec(y, j)
    out.append(y)
    # 2: the CFO at which the time offset under the speculative scale and
    # under the exact one round apart (time_offset falls with the CFO; bisect
    # to a half-integer under the speculative scale, then step across it)
    spike = 2 * N + 5

    def both(c):
        y = frame(c, upto=3 * N)
        v2 = view(y)[:2 * N].copy()
        y[spike] *= np.complex64(4.0)
        return oracle.lora_demodulate(view(y), sf)[3][1], oracle.lora_demodulate(v2, sf)[3][1]

    half = math.floor(both(0.3)[1]) + 0.5
    lo, hi = 0.3 - 2.0 / N, 0.3 + 2.0 / N
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        if both(mid)[1] > half:
            lo = mid
        else:
            hi = mid
    cs = [lo + k * 2e-5 / N for k in range(-400, 400)]
    c2 = next((c for c in cs if _roundf(both(c)[0]) != _roundf(both(c)[1])), None)
    assert c2 is not None, f"sf {sf} mode {mode}: no CFO near {lo} splits the two time offsets"
    y = frame(c2)
    y[spike] *= np.complex64(4.0)
    only_above_spec(y, spike)
    assert t_off(y) != _roundf(oracle.lora_demodulate(view(y)[:2 * N].copy(), sf)[3][1])
    out.append(y)
    # 3: one ulp above the speculative maximum, at a sample that is its own dechirp
    y = frame(0.2)
    spec = np.float32(_maxabs(view(y))[:2 * N].max())
    assert spec == BUMP
    up = np.nextafter(spec, np.float32(np.inf))
    assert np.float32(1.0) / up != np.float32(1.0) / spec  # (else the frame is confirmed, not settled)
    put(y, 5 * N + 7, up)
    only_above_spec(y, 5 * N + 7)
    out.append(y)
    return np.stack(out), S


@functools.lru_cache(maxsize=None)
def _spec_mix(oracle, sf, mode, nf):
    """nf frames of spec_frames' 7 kinds followed by the four edge frames,
    with the oracle's outputs with and without scratch."""
    tail = (1 << sf) // 2 + 3 if mode == 1 else 0
    edge, S = _edge_frames(oracle, sf, mode)
    iq = np.concatenate([spec_frames(oracle, sf, nf, seed=sf * 41 + mode, tail=tail), edge])
    return iq, S, _references(oracle, iq, sf, mode), _references(oracle, iq, sf, mode, scratch=False)


@pytest.mark.parametrize("sf,nf", [(11, 14), (12, 7)])
@pytest.mark.parametrize("mode", [1, 2])
def test_spec_big_branches(oracle, lphy, sf, nf, mode):
    """The product library's speculation against the test build's whole-frame
    pre-scan (LPHY_F_SCAN_FIRST: A.spec off, k_maxabs scans the frame) and
    against the oracle, on the 7 kinds and the four edge frames."""
    iq, S, refs, _ = _spec_mix(oracle, sf, mode, nf)
    n, fs = iq.shape
    d = lphy.Demodulator(sf)
    a = d.demod_host(iq, n, fs, mode, lphy.F_DECODE | lphy.F_UNFUSED)
    dt = lphy.Demodulator(sf, test_build=True)
    b = dt.demod_host(iq, n, fs, mode, lphy.F_DECODE | lphy.F_UNFUSED | lphy.F_SCAN_FIRST)
    assert dt.bounds_violations() == 0
    _check(a, refs, f"sf {sf} mode {mode} speculation")
    _check(b, refs, f"sf {sf} mode {mode} pre-scan")
    _same(a, b, f"sf {sf} mode {mode}")
    # the frame whose time shift the exact scale moves: re-run whole, every
    # symbol counted
    k = nf + 2
    d.recheck_count(reset=True)
    one = d.demod_host(iq[k:k + 1], 1, fs, mode, lphy.F_DECODE | lphy.F_UNFUSED)
    n_exact = d.recheck_count(reset=True)
    _check(one, refs[k:k + 1], f"sf {sf} mode {mode} edge frame 2 alone")
    assert n_exact >= S, f"{n_exact} exact re-runs, {S} symbols"


@pytest.mark.parametrize("sf,nf", [(11, 14), (12, 7)])
@pytest.mark.parametrize("mode", [1, 2])
def test_spec_big_mix_without_scratch(oracle, lphy, sf, nf, mode):
    """LPHY_F_NO_SCRATCH: the speculation is off and a frame that would need
    the rescale is -ERANGE, exactly where the oracle says."""
    iq, S, _, refs = _spec_mix(oracle, sf, mode, nf)
    n, fs = iq.shape
    status = [r[0] for r in refs]
    assert ERANGE in status and any(s >= 0 for s in status)
    got = lphy.Demodulator(sf).demod_host(iq, n, fs, mode, lphy.F_DECODE | lphy.F_UNFUSED | lphy.F_NO_SCRATCH)
    _check(got, refs, f"sf {sf} mode {mode} no scratch")


# ---- 6. the per-frame record under contention -------------------------------
def test_spec_big_atomics_repeatable(oracle, lphy):
    """40 frames at SF 11 (36 of the 7 kinds and the four edge frames), whose
    uint4 records many workgroups write with atomicMax / atomicMin /
    atomicOr: three runs on one context and two at once on two streams give
    the same bits, the oracle's."""
    import torch
    sf, mode = 11, 2
    iq, S, refs, _ = _spec_mix(oracle, sf, mode, 36)
    nf, fs = iq.shape
    F = lphy.F_DECODE | lphy.F_UNFUSED
    d = lphy.Demodulator(sf)
    first = d.demod_host(iq, nf, fs, mode, F)
    _check(first, refs, "40 frames")
    for rep in range(2):
        _same(d.demod_host(iq, nf, fs, mode, F), first, f"run {rep + 2}")
    dev = torch.device("cuda", 0)
    x_t = torch.from_numpy(iq.view(np.float32).copy()).to(dev)
    per = d.syms_per_frame(fs, mode)
    st = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    torch.cuda.synchronize()
    for s in st:
        with torch.cuda.stream(s):
            syms = torch.zeros(nf * per, dtype=torch.int16, device=dev)
            pay = torch.zeros(nf * (per // 2), dtype=torch.uint8, device=dev)
            meta = torch.zeros(nf * 32, dtype=torch.uint8, device=dev)
            d.demod_batch(x_t, nf, fs, syms, meta, mode, F, payload=pay, stream=s.cuda_stream)
            outs.append((syms, pay, meta))
    torch.cuda.synchronize()
    for i, (syms, pay, meta) in enumerate(outs):
        got = (syms.cpu().numpy().view(np.uint16).reshape(nf, per), pay.cpu().numpy().reshape(nf, per // 2),
               meta.cpu().numpy().view(lphy.META_DTYPE))
        _same(got, first, f"stream {i}")
