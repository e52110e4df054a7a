"""Pin the CPU oracle (oracle/lphy_oracle.c) to the reference library itself
(oracle/_ref/libloraref.so, compiled from /root/reference's sources by
oracle/Makefile) on seeded random inputs: every output bit of each function
on the hot path.  Skipped where the reference build is absent (GPU boxes)."""
import numpy as np
import pytest


def _iq(rng, n, scale=1.0):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(np.complex64)


def _frame(oracle, rng, sf, bw, plen, snr=None, delay=0, cfo=0.0):
    iq = oracle.modulate(oracle.encode(rng.integers(0, 256, plen, dtype=np.uint8).tobytes()), sf, bw_hz=bw)
    if cfo:
        iq = (iq * np.exp(2j * np.pi * cfo / (1 << sf) * np.arange(iq.size))).astype(np.complex64)
    if delay:
        iq = np.concatenate([np.zeros(delay, np.complex64), iq[:-delay]])
    if snr is not None:
        s = np.sqrt(10 ** (-snr / 10) / 2)
        iq = (iq + s * (rng.standard_normal(iq.size) + 1j * rng.standard_normal(iq.size))).astype(np.complex64)
    return iq


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("sf", range(1, 13))
def test_fft_bit_exact(oracle, reference, sf):
    rng = np.random.default_rng(sf)
    for _ in range(4):
        x = _iq(rng, 1 << sf, scale=10.0 ** rng.uniform(-3, 3))
        np.testing.assert_array_equal(oracle.fft(x).view(np.uint32), reference.fft(x).view(np.uint32))


@pytest.mark.parametrize("sf,bw", [(s, b) for s in (2, 5, 7, 9, 12) for b in (125000, 250000, 500000)])
def test_modulate_and_dechirp_bit_exact(oracle, reference, sf, bw):
    rng = np.random.default_rng(sf * 7 + bw // 125000)
    syms = rng.integers(0, 1 << min(sf, 8), 12, dtype=np.uint16)
    for sync in (0x12, 0x34, 0xAB):
        a = oracle.modulate(syms, sf, bw_hz=bw, sync=sync)
        b = reference.modulate(syms, sf, bw_hz=bw, sync=sync)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    x = _iq(rng, 5 * (1 << sf))
    np.testing.assert_array_equal(oracle.dechirp(x, sf, bw).view(np.uint32),
                                  reference.dechirp(x, sf, bw).view(np.uint32))


CASES = [(sf, bw, plen, snr, delay, cfo, hann)
         for sf, bw, plen, snr, delay, cfo, hann in [
             (7, 125000, 32, None, 0, 0.0, False), (7, 125000, 16, -10.0, 0, 0.0, False),
             (7, 125000, 20, -18.0, 3, 0.0, False), (7, 250000, 8, None, 0, 0.3, False),
             (8, 125000, 32, None, 11, -0.2, True), (8, 500000, 12, 0.0, 0, 0.45, False),
             (9, 125000, 32, -10.0, 0, 0.0, False), (9, 125000, 32, -15.0, 0, 0.0, False),
             (10, 125000, 16, None, 5, 0.1, False), (11, 125000, 8, -5.0, 0, 0.0, False),
             (12, 125000, 4, None, 0, -0.35, False), (5, 125000, 8, None, 0, 0.0, False),
             (6, 250000, 8, 3.0, 2, 0.0, True), (3, 125000, 6, None, 0, 0.0, False)]]


@pytest.mark.parametrize("sf,bw,plen,snr,delay,cfo,hann", CASES)
def test_demodulate_paths_bit_exact(oracle, reference, sf, bw, plen, snr, delay, cfo, hann):
    """lora_phy::demodulate + decode and dechirp -> lora_demodulate ->
    lora_decode, every output including the float metrics' bits."""
    rng = np.random.default_rng(sf * 1000 + plen + delay)
    for rep in range(3):
        iq = _frame(oracle, rng, sf, bw, plen, snr, delay, cfo)
        a = oracle.demodulate(iq, sf, bw_hz=bw, hann=hann)
        b = reference.demodulate(iq, sf, bw_hz=bw, hann=hann)
        assert a[0] == b[0] and a[2] == b[2]
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(_bits(a[3][:2]), _bits(b[3][:2]))
        np.testing.assert_array_equal(oracle.decode(a[1])[1], reference.decode(b[1])[1])
        x = oracle.dechirp(iq, sf, bw)
        for scratch in (True, False):
            a = oracle.lora_demodulate(x, sf, hann=hann, scratch=scratch)
            b = reference.lora_demodulate(x, sf, hann=hann, scratch=scratch)
            assert a[0] == b[0] and a[2] == b[2]
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(_bits(a[3][:2]), _bits(b[3][:2]))


def test_noise_frames_large_phase(oracle, reference):
    """Pure noise: bogus CFO estimates drive the rotation angle past 120 rad
    (glibc sincosf's large-argument path)."""
    rng = np.random.default_rng(77)
    for sf in (7, 8):
        for _ in range(4):
            x = _iq(rng, 60 * (1 << sf))
            a = oracle.lora_demodulate(x, sf)
            b = reference.lora_demodulate(x, sf)
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(_bits(a[3][:2]), _bits(b[3][:2]))


def test_encode_decode_roundtrip(oracle, reference):
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 7, 32, 255):
        p = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        np.testing.assert_array_equal(oracle.encode(p), reference.encode(p))
        syms = oracle.encode(p) ^ rng.integers(0, 2, 2 * n, dtype=np.uint16) << rng.integers(0, 8, 2 * n, dtype=np.uint16)
        np.testing.assert_array_equal(oracle.decode(syms)[1], reference.decode(syms)[1])
        assert oracle.decode(syms)[2] == reference.decode(syms)[2]


def _osr_frame(oracle, rng, sf, osr, plen, snr, delay, cfo):
    """A frame modulated at osr samples per chip, delayed by a fraction of a
    symbol, with carrier offset and noise."""
    iq = oracle.modulate(oracle.encode(rng.integers(0, 256, plen, dtype=np.uint8).tobytes()),
                         sf, osr=osr)
    if cfo:
        iq = (iq * np.exp(2j * np.pi * cfo / ((1 << sf) * osr) * np.arange(iq.size))).astype(np.complex64)
    if delay:
        iq = np.concatenate([np.zeros(delay, np.complex64), iq[:-delay]])
    if snr is not None:
        s = np.sqrt(10 ** (-snr / 10) / 2)
        iq = (iq + s * (rng.standard_normal(iq.size) + 1j * rng.standard_normal(iq.size))).astype(np.complex64)
    return iq


def _tie_frame(sf, osr, nsym, amp):
    """Oversampled input whose phases tie on detector power with different
    argmax bins: phase 0 carries an alternating sequence (peak at N/2),
    phase 1 a constant one (peak at 0).  LoRaDemod.cpp:102 breaks the tie
    towards the lower bin, phy.cpp:114 keeps the first phase."""
    N = 1 << sf
    x = np.zeros((nsym, N, osr), np.complex64)
    x[:, :, 0] = amp * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    if osr > 1:
        x[:, :, 1] = amp
    return x.reshape(-1)


OSR_CASES = [  # sf, osr, payload bytes, snr, delay, cfo, hann
    (7, 2, 16, None, 0, 0.0, False), (7, 2, 16, -8.0, 37, 0.2, False),
    (7, 4, 8, None, 301, -0.3, False), (8, 3, 12, 0.0, 5, 0.1, True),
    (9, 2, 8, -12.0, 0, 0.0, False), (5, 8, 8, None, 17, 0.05, False),
    (10, 2, 4, None, 700, 0.0, False), (12, 2, 4, -5.0, 0, 0.0, False),
    (11, 4, 4, None, 33, 0.4, True)]


@pytest.mark.parametrize("sf,osr,plen,snr,delay,cfo,hann", OSR_CASES)
def test_oversampled_paths_bit_exact(oracle, reference, sf, osr, plen, snr, delay, cfo, hann):
    """osr > 1: the estimate picks the best of osr phases by detector power
    (log10f), symbols read every osr-th sample after the time shift."""
    rng = np.random.default_rng(sf * 31 + osr * 7 + delay)
    for rep in range(2):
        iq = _osr_frame(oracle, rng, sf, osr, plen, snr, delay, cfo)
        a = oracle.demodulate(iq, sf, osr=osr, hann=hann)
        b = reference.demodulate(iq, sf, osr=osr, hann=hann)
        assert a[0] == b[0] and a[2] == b[2]
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(_bits(a[3][:2]), _bits(b[3][:2]))
        nsym = iq.size // ((1 << sf) * osr)
        for n in (1, 3, nsym):  # estimate_offsets over n whole symbols
            seg = iq[: n * (1 << sf) * osr]
            np.testing.assert_array_equal(_bits(oracle.estimate_offsets(seg, sf, osr, hann)),
                                          _bits(reference.estimate_offsets(seg, sf, osr, hann)))
        for scratch in (True, False):
            a = oracle.lora_demodulate(iq, sf, osr=osr, hann=hann, scratch=scratch)
            b = reference.lora_demodulate(iq, sf, osr=osr, hann=hann, scratch=scratch)
            assert a[0] == b[0] and a[2] == b[2]
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(_bits(a[3][:2]), _bits(b[3][:2]))


@pytest.mark.parametrize("sf,osr,amp", [(2, 2, 0.5), (7, 2, 0.25), (7, 4, 3.0), (10, 2, 1.0)])
def test_oversampled_power_tie(oracle, reference, sf, osr, amp):
    x = _tie_frame(sf, osr, 6, amp)
    a = oracle.demodulate(x, sf, osr=osr)
    b = reference.demodulate(x, sf, osr=osr)
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(_bits(a[3][:2]), _bits(b[3][:2]))
    a1 = oracle.lora_demodulate(x, sf, osr=osr)
    b1 = reference.lora_demodulate(x, sf, osr=osr)
    np.testing.assert_array_equal(a1[1], b1[1])
    np.testing.assert_array_equal(_bits(a1[3][:2]), _bits(b1[3][:2]))
    # the two tie rules pick different phases here
    assert _bits(a[3][1]) != _bits(a1[3][1])


# Non-finite samples: GCC's std::complex<float> product calls __mulsc3 when
# both result parts are NaN (C99 Annex G recovery of infinities), in the
# dechirp, the rotation and every KISS butterfly.  The oracle restates it.
NONFINITE = [(complex(-np.inf, np.nan)), complex(np.inf, 0.25), complex(np.inf, np.inf),
             complex(np.nan, 3.0), complex(0.5, np.nan), complex(-np.inf, -np.inf),
             complex(3e38, 3e38), complex(np.nan, np.inf)]


def _nan_bits_equal(a, b):
    a = np.asarray(a, np.float32).reshape(-1)
    b = np.asarray(b, np.float32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    np.testing.assert_array_equal(na, nb)
    np.testing.assert_array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _nonfinite_frames(oracle, sf, rng):
    base = _frame(oracle, rng, sf, 125000, 8)
    out = []
    for v in NONFINITE:
        for pos in (3, (1 << sf) + 5, base.size - 7):
            x = base.copy()
            x[pos] = v
            out.append(x)
    return out


@pytest.mark.parametrize("sf", [2, 7, 8])
def test_nonfinite_samples_bit_exact(oracle, reference, sf):
    rng = np.random.default_rng(900 + sf)
    for iq in _nonfinite_frames(oracle, sf, rng):
        a = oracle.demodulate(iq, sf)
        b = reference.demodulate(iq, sf)
        assert a[0] == b[0] and a[2] == b[2]
        np.testing.assert_array_equal(a[1], b[1])
        _nan_bits_equal(a[3][:2], b[3][:2])
        x = oracle.dechirp(iq, sf, 125000)
        _nan_bits_equal(x.view(np.float32), reference.dechirp(iq, sf, 125000).view(np.float32))
        for inp in (x, iq):
            a = oracle.lora_demodulate(inp, sf)
            b = reference.lora_demodulate(inp, sf)
            assert a[0] == b[0] and a[2] == b[2]
            np.testing.assert_array_equal(a[1], b[1])
            _nan_bits_equal(a[3][:2], b[3][:2])
        # FFT bins bit for bit, except that a NaN's sign/payload follows the
        # host's operand order (x86 keeps the first NaN operand); NaN
        # positions must agree
        fa, fb = oracle.fft(iq[: 1 << sf]), reference.fft(iq[: 1 << sf])
        _nan_bits_equal(fa.view(np.float32), fb.view(np.float32))


# ---- estimate_offsets over many symbols (phy.cpp:81-148) ------------------
# Input kinds of the estimate tests, here and in tests/test_gpu_estimate.py:
# a noisy packet, noise (random peak phases: both unwrap loops of
# phy.cpp:129-130 run), a packet with all-zero symbols (no bin beats
# best_p = -1e30, so the symbol adds index 0, phase 0) and small noise.
EST_KINDS = ("packet", "noise", "packet_gap", "packet_gap0", "noise_small")


def _estimate_head(oracle, rng, kind, sf, osr, n):
    """n whole symbols of estimate input of one kind.  packet: random symbols
    with a carrier offset of 0.1-0.45 bin, a delay of 1-5 samples and noise at
    0 dB; packet_gap: the same with symbol n // 2 zeroed, packet_gap0 with
    symbol 0 zeroed too; noise: complex Gaussian, noise_small: scaled by 1e-3."""
    step = (1 << sf) * osr
    count = n * step
    if kind in ("noise", "noise_small"):
        return _iq(rng, count, 1e-3 if kind == "noise_small" else 1.0)
    syms = rng.integers(0, 1 << min(sf, 8), n, dtype=np.uint16)
    x = oracle.modulate(syms, sf, osr=osr).astype(np.complex128)
    cfo = rng.uniform(0.1, 0.45) * rng.choice((-1.0, 1.0))
    x = x * np.exp(2j * np.pi * cfo / step * np.arange(x.size))
    x = np.concatenate([np.zeros(int(rng.integers(1, 6))), x])[:count]
    x = (x + np.sqrt(0.5) * (rng.standard_normal(count) + 1j * rng.standard_normal(count))).astype(np.complex64)
    if kind in ("packet_gap", "packet_gap0"):
        x[(n // 2) * step:(n // 2 + 1) * step] = 0
        if kind == "packet_gap0":
            x[:step] = 0
    else:
        assert kind == "packet"
    return x


def _estimate_nonfinite(oracle, rng, sf, osr, n):
    """Packets with a NaN sample in one symbol, an Inf sample in another
    (the last), and both.  The NaN symbol's bins are all NaN: no valid peak."""
    step = (1 << sf) * osr
    base = _estimate_head(oracle, rng, "packet", sf, osr, n)
    p_nan = (1 if n >= 3 else 0) * step + 5
    p_inf = (n - 1) * step + 11
    out = []
    for nan, inf in ((True, False), (False, True), (True, True)):
        x = base.copy()
        if nan:
            x[p_nan] = complex(np.nan, 3.0)
        if inf:
            x[p_inf] = complex(np.inf, 0.25)
        out.append(x)
    return out


@pytest.mark.parametrize("sf,hann,ns", [(5, False, (1, 2, 9, 33)), (7, False, (1, 2, 9, 33)),
                                        (7, True, (1, 2, 9, 33)), (9, True, (1, 2, 9, 33)),
                                        (12, False, (1, 2, 5))],
                         ids=["sf5", "sf7", "sf7-hann", "sf9-hann", "sf12"])
def test_estimate_offsets_many_symbols_bit_exact(oracle, reference, sf, hann, ns):
    """osr 1 over up to 33 symbols: the float sum of unwrapped phase
    differences in symbol order, symbols without a valid peak, non-finite
    samples.  tests/test_gpu_estimate.py holds the GPU to the oracle here."""
    rng = np.random.default_rng(4100 + sf * 2 + hann)
    for n in ns:
        for kind in EST_KINDS:
            if kind == "packet_gap0" and n < 2:
                continue
            x = _estimate_head(oracle, rng, kind, sf, 1, n)
            a, b = oracle.estimate_offsets(x, sf, 1, hann), reference.estimate_offsets(x, sf, 1, hann)
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"n {n} {kind}")
        for x in _estimate_nonfinite(oracle, rng, sf, 1, n):
            _nan_bits_equal(oracle.estimate_offsets(x, sf, 1, hann), reference.estimate_offsets(x, sf, 1, hann))


# ---- lora_modulate's amplitude (LoRaMod.cpp:18 clamp, std::polar) ----------
AMPLITUDES = [0.5, -0.75, 0.0, 1.0, 1.5, -3.0, float("nan")]


@pytest.mark.parametrize("sf", [7, 10])
def test_modulate_amplitude_bit_exact(oracle, reference, sf):
    """std::max(-1.0f, std::min(1.0f, a)): out-of-range amplitudes clamp, a
    NaN amplitude becomes 1 (std::min keeps its first argument), negative
    ones and 0 keep std::polar's signs (-0.0 included)."""
    rng = np.random.default_rng(70 + sf)
    syms = rng.integers(0, 1 << min(sf, 8), 6, dtype=np.uint16)
    for a in AMPLITUDES:
        _nan_bits_equal(oracle.modulate(syms, sf, ampl=a, sync=0x34).view(np.float32),
                        reference.modulate(syms, sf, ampl=a, sync=0x34).view(np.float32))
    one = reference.modulate(syms, sf, ampl=1.0, sync=0x34)
    np.testing.assert_array_equal(reference.modulate(syms, sf, ampl=float("nan"), sync=0x34).view(np.uint32),
                                  one.view(np.uint32))


COMP_CASES = [  # sf, osr, cfo, time_offset
    (7, 1, 0.37, 95.54), (7, 1, -0.21, -12.4), (8, 1, 0.0, 0.0), (9, 2, 0.45, 300.2),
    (12, 1, -0.5, 1e9), (7, 1, 3.0, -2.6e9), (5, 4, 0.1, float("nan")), (10, 1, 1e-4, 0.49)]


@pytest.mark.parametrize("sf,osr,cfo,toff", COMP_CASES)
def test_compensate_offsets_bit_exact(oracle, reference, sf, osr, cfo, toff):
    """phy.cpp:150-180: rotation by -2 pi cfo n / (N osr), then the integer
    shift by round(time_offset) (no shift when it is out of range or NaN)."""
    rng = np.random.default_rng(sf * 13 + osr)
    x = _iq(rng, 7 * (1 << sf) * osr, scale=2.0)
    x[3] = complex(np.inf, 0.5)  # Annex G product inside the rotation
    _nan_bits_equal(oracle.compensate_offsets(x, sf, cfo, toff, osr).view(np.float32),
                    reference.compensate_offsets(x, sf, cfo, toff, osr).view(np.float32))


# ---- LoRaCodes.hpp helpers: oracle vs the reference header
def test_codes_gray_and_hamming_exhaustive(oracle, reference):
    for v in range(0, 65536, 7):
        for tb in (0, 1):
            assert oracle.gray(v, tb) == reference.gray(v, tb)
    for x in range(256):
        for op in range(8):
            assert oracle.hamming(x, op) == reference.hamming(x, op), (x, op)


@pytest.mark.parametrize("ppm,rdd", [(p, r) for p in (5, 7, 8, 10, 12) for r in (0, 1, 2, 4)])
def test_codes_interleaver(oracle, reference, ppm, rdd):
    rng = np.random.default_rng(ppm * 10 + rdd)
    cw = rng.integers(0, 1 << (4 + rdd), 3 * ppm + 2, dtype=np.uint8)
    a, b = oracle.interleave(cw, ppm, rdd), reference.interleave(cw, ppm, rdd)
    np.testing.assert_array_equal(a, b)
    syms = rng.integers(0, 1 << ppm, 3 * (4 + rdd) + 1, dtype=np.uint16)
    np.testing.assert_array_equal(oracle.deinterleave(syms, ppm, rdd), reference.deinterleave(syms, ppm, rdd))
    # round trip of whole blocks
    np.testing.assert_array_equal(oracle.deinterleave(a, ppm, rdd), cw[: len(a) // (4 + rdd) * ppm])


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_codes_whitening_and_checksums(oracle, reference, kind):
    rng = np.random.default_rng(40 + kind)
    for rdd in (0, 1, 2, 3, 4):
        for bit_ofs in (0, 1, 7, 100):
            buf = rng.integers(0, 256, 255, dtype=np.uint8)
            np.testing.assert_array_equal(oracle.whiten(buf, kind, bit_ofs, rdd),
                                          reference.whiten(buf, kind, bit_ofs, rdd))
    for n in (0, 1, 2, 5, 64, 255):
        buf = rng.integers(0, 256, max(n, 2), dtype=np.uint8)[: max(n, 2)]
        assert oracle.checksum(buf[:n] if kind != 1 else buf, kind) == \
            reference.checksum(buf[:n] if kind != 1 else buf, kind)
    # whitening_test.cpp:30-31 known answer
    w = oracle.whiten(np.frombuffer(bytes.fromhex("DEADBEEF700D"), np.uint8), 2, 0, 4)
    assert w.tobytes() == bytes.fromhex("215290102CF2")


# ---- the parameters tests/test_gpu_codes.py leans on the oracle for beyond the
# SX127x geometries above: every ppm 1..16 (ppm < 4 + rdd, where the diagonal
# wraps more than once, and 13..16 among them) and rdd 0..4, on inputs with
# every bit set at random: codeword bits at and above 4 + rdd and symbol bits
# at and above ppm, which both sides must ignore.
@pytest.mark.parametrize("rdd", range(5))
def test_codes_interleaver_every_geometry_full_width(oracle, reference, rdd):
    rng = np.random.default_rng(900 + rdd)
    nb = 4 + rdd
    for ppm in range(1, 17):
        cw = rng.integers(0, 256, 3 * ppm + (ppm - 1), dtype=np.uint8)
        a, b = oracle.interleave(cw, ppm, rdd), reference.interleave(cw, ppm, rdd)
        assert len(a) == 3 * nb
        np.testing.assert_array_equal(a, b, str(ppm))
        np.testing.assert_array_equal(a, oracle.interleave(cw & ((1 << nb) - 1), ppm, rdd))
        syms = rng.integers(0, 65536, 3 * nb + (nb - 1), dtype=np.uint16)
        c, d = oracle.deinterleave(syms, ppm, rdd), reference.deinterleave(syms, ppm, rdd)
        assert len(c) == 3 * ppm
        np.testing.assert_array_equal(c, d, str(ppm))
        np.testing.assert_array_equal(c, oracle.deinterleave(syms & ((1 << ppm) - 1), ppm, rdd))
        np.testing.assert_array_equal(oracle.deinterleave(a, ppm, rdd), cw[: 3 * ppm] & ((1 << nb) - 1))


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_codes_whitening_across_periods(oracle, reference, kind):
    """Rows of 600 and 1024 full-width bytes from offsets at, around and several
    times past the generators' period of 510 positions, every rdd; and the
    longest row the reference's uint16_t length admits."""
    rng = np.random.default_rng(920 + kind)
    for rdd in range(5):
        for bit_ofs in (0, 1, 3, 100, 503, 504, 509, 510, 511, 1019, 1020, 1021, 5103):
            for n in (600, 1024):
                buf = rng.integers(0, 256, n, dtype=np.uint8)
                a, b = oracle.whiten(buf, kind, bit_ofs, rdd), reference.whiten(buf, kind, bit_ofs, rdd)
                np.testing.assert_array_equal(a, b, str((rdd, bit_ofs, n)))
                if kind:  # only the 4 + rdd codeword bits change
                    assert not ((a ^ buf) & (0xFF ^ (0xFF >> (4 - rdd)))).any()
    buf = rng.integers(0, 256, 65535, dtype=np.uint8)
    np.testing.assert_array_equal(oracle.whiten(buf, kind, 9, 2), reference.whiten(buf, kind, 9, 2))


# ---- lora_phy::decode on the decode case table (tests/decode_cases.py) -----
# rows that do and do not carry a matching checksum, at the byte counts where
# csrc/lphy_final.h branches; tests/test_gpu_decode.py leans on the oracle here
import decode_cases as dc  # noqa: E402


@pytest.mark.parametrize("nb", dc.NB_TABLE)
def test_decode_case_table_bit_exact(oracle, reference, nb):
    for variant in (0, 1, 2):
        for kind in dc.kinds_for(nb):
            syms = dc.row(oracle, nb, kind, variant)
            a, b = oracle.decode(syms), reference.decode(syms)
            assert a[0] == b[0] == nb, (kind, variant)
            np.testing.assert_array_equal(a[1], b[1], err_msg=f"{kind} {variant}")
            assert a[2] == b[2], (kind, variant)
            want = dc.promised(nb, kind)
            assert b[2] == (dc.CORRECTED_VERDICT[nb] if want is None else want), (kind, variant)
