"""Shared by tests/test_detect_cpu.py and tests/test_gpu_detect.py: what
lphy_hip_detect_batch must return, from the CPU oracle alone.

A window's expected record is orc_detect (oracle/lphy_oracle.c, the C
restatement of LoRaDetector.hpp:39-74) on the window's input built here:
the strided slice, [oracle.dechirp on the N-sample slice,] [times the Hann
table of LoRaDemod.cpp:20-22, built with glibc cosf in float32 steps].
test_detect_cpu.py checks this helper itself against the reference build.
"""
from __future__ import annotations

import ctypes as C
import ctypes.util
import functools

import numpy as np

from checkers import _f32p, _p

SFS = (7, 8, 10, 12)  # several windows per wave, one per wave (10), several waves per window (12)
NOISE_WINDOWS = {7: 256, 8: 256, 10: 32, 12: 6}
F32 = np.float32


@functools.lru_cache(maxsize=None)
def hann_table(N: int) -> np.ndarray:
    """w[i] = 0.5f - 0.5f * cosf(2.0f * PI * (float)i / ((float)N - 1.0f)),
    every operation rounded to float32 (LoRaDemod.cpp:20-22)."""
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.cosf.argtypes = [C.c_float]
    libm.cosf.restype = C.c_float
    two_pi = F32(F32(2.0) * F32(3.14159265358979323846))
    den = F32(F32(N) - F32(1.0))
    w = np.zeros(N, F32)
    for i in range(N):
        a = F32(F32(two_pi * F32(i)) / den)
        w[i] = F32(F32(0.5) - F32(F32(0.5) * F32(libm.cosf(float(a)))))
    return w


def window_input(oracle, iq, sf, first, hop, step, w, dechirp, hann) -> np.ndarray:
    """The N samples detect() sees for window w."""
    N = 1 << sf
    start = first + w * hop
    x = np.ascontiguousarray(np.asarray(iq, np.complex64).reshape(-1)[start:start + (N - 1) * step + 1:step])
    assert x.size == N
    if dechirp:
        x = oracle.dechirp(x, sf)
    if hann:  # complex times float: each part times w[i]
        x = (x.view(F32).reshape(N, 2) * hann_table(N)[:, None]).astype(F32).reshape(-1).view(np.complex64)
    return x


def orc_detect(oracle, x):
    """(index, power, power_avg, findex, bins) of orc_detect on N samples."""
    x = np.ascontiguousarray(x, np.complex64).view(F32)
    out = np.zeros_like(x)
    p, pa, fi = (np.zeros(1, F32) for _ in range(3))
    idx = oracle.lib.orc_detect(_p(x, _f32p), _p(out, _f32p), x.size // 2, _p(p, _f32p), _p(pa, _f32p),
                                _p(fi, _f32p))
    return int(idx), p[0], pa[0], fi[0], out.view(np.complex64)


def expected(oracle, lphy, iq, sf, first, hop, step, windows, dechirp, hann) -> np.ndarray:
    """The records of one detect call (lphy.DETECT_DTYPE)."""
    out = np.zeros(windows, lphy.DETECT_DTYPE)
    for w in range(windows):
        idx, p, pa, fi, _ = orc_detect(oracle, window_input(oracle, iq, sf, first, hop, step, w, dechirp, hann))
        out[w] = (p, pa, fi, idx, 0)
    return out


def assert_records_equal(got, want, what=""):
    """Bit for bit; where the oracle gives a NaN, any NaN."""
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(got["index"], want["index"], err_msg=f"{what}: index")
    np.testing.assert_array_equal(got["reserved"], 0, err_msg=f"{what}: reserved")
    for k in ("power", "power_avg", "findex"):
        g, e = got[k], want[k]
        nan = np.isnan(e)
        bad = np.where(nan, ~np.isnan(g), g.view(np.uint32) != e.view(np.uint32))
        assert not bad.any(), (f"{what}: {k} differs in windows {np.flatnonzero(bad)[:8].tolist()}: "
                               f"got {g[bad][:4]!r}, want {e[bad][:4]!r}")


def packets(oracle, sf, noisy: bool, osr: int = 1) -> np.ndarray:
    """The fixture sets, flat: modulated packets (test_gpu_osr._frames) of
    NOISE_WINDOWS[sf] symbols in all, at -8 dB (noise set) or without noise
    (clean-tone set; the same packets: a generator per frame, whose first
    draw is the payload)."""
    from test_gpu_osr import _frames
    nf, plen = {7: (4, 31), 8: (4, 31), 10: (1, 15), 12: (1, 2)}[sf]
    iq = np.concatenate([_frames(oracle, sf, osr, 1, plen, seed=100 + sf + 1000 * f,
                                 snr=-8.0 if noisy else None).reshape(-1) for f in range(nf)])
    assert iq.size == NOISE_WINDOWS[sf] * (1 << sf) * osr
    return iq


def detector_feed(oracle, iq, sf, dechirp: bool) -> np.ndarray:
    """What a call is given so that the detector sees dechirped symbols either
    way: the packets themselves with LPHY_DET_DECHIRP, else dechirped here."""
    return iq if dechirp else oracle.dechirp(iq, sf)


def cancellation(oracle, x) -> float:
    """(total - maxValue) / total of a window's bins, in double (0 for an
    all-zero window): below ~N 2^-50 / 2^-24 no bound on a reordered sum
    separates the float the reference rounds to."""
    bins = orc_detect(oracle, x)[4]
    m2 = (bins.real.astype(F32) * bins.real.astype(F32) + bins.imag.astype(F32) * bins.imag.astype(F32)).astype(F32)
    total = float(np.cumsum(m2.astype(np.float64))[-1])  # in bin order
    return (total - float(m2.max())) / total if total > 0 else 0.0
