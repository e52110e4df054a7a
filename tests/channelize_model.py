"""The channeliser's definition (include/lphy_hip.h, lphy_hip_channelize) in
plain numpy float32, and the design helper's float64 maths written out on its
own.  The tests compare the library with this byte for byte.

channelize(): vectorised over the outputs m, a Python loop over the taps k, so
every product, sum and difference is one float32 numpy operation in the
definition's order (numpy neither fuses nor reassociates element-wise
operations)."""
from fractions import Fraction
from math import gcd

import numpy as np


def outputs(in_samples, first, taps, decim):
    """The largest count of outputs whose taps all lie inside the capture."""
    if taps == 0 or decim == 0 or first + taps > in_samples:
        return 0
    return (in_samples - first - taps) // decim + 1


def channelize(x, taps, rot, decim, first=0, n_out=None, rot_first=0):
    """x: complex64 [n]; taps: complex64 [C, T]; rot: complex64 [C, R].
    Returns complex64 [C, n_out]."""
    x = np.ascontiguousarray(x, np.complex64).reshape(-1)
    taps = np.ascontiguousarray(taps, np.complex64)
    rot = np.ascontiguousarray(rot, np.complex64)
    C, T = taps.shape
    R = rot.shape[1]
    if n_out is None:
        n_out = outputs(x.size, first, T, decim)
    assert n_out == 0 or first + (n_out - 1) * decim + T <= x.size
    xr, xi = x.real.copy(), x.imag.copy()
    base = first + np.arange(n_out, dtype=np.int64) * decim
    ridx = np.array([(rot_first + m) % R for m in range(n_out)], dtype=np.int64)
    out = np.zeros((C, n_out), np.complex64)
    with np.errstate(all="ignore"):
        for c in range(C):
            ar = np.zeros(n_out, np.float32)
            ai = np.zeros(n_out, np.float32)
            for k in range(T):
                re, im = xr[base + k], xi[base + k]
                gr, gi = taps[c, k].real, taps[c, k].imag   # numpy float32 scalars
                pr = re * gr - im * gi
                pi = re * gi + im * gr
                ar = ar + pr
                ai = ai + pi
            rr, rim = rot[c, ridx].real, rot[c, ridx].imag
            out[c].real = ar * rr - ai * rim
            out[c].imag = ar * rim + ai * rr
    return out


def _bessel_i0(v):
    return np.i0(v)


def design(centres, decim, taps, cutoff, beta):
    """(taps complex64 [C, T], rot complex64 [C, R], R, delay): a Kaiser(beta)
    windowed sinc with its edge at `cutoff` cycles per input sample and unit
    gain at DC, times the mixer exp(-2 pi i centre k); rot the mixer's phase
    every `decim` samples over its least common period R."""
    T = taps
    alpha = (T - 1) / 2.0
    n = np.arange(0, T)
    if T == 1:
        win = np.ones(1)
    else:
        win = _bessel_i0(beta * np.sqrt(1 - ((n - alpha) / alpha) ** 2.0)) / _bessel_i0(float(beta))
    arg = 2.0 * cutoff * (np.arange(T, dtype=np.float64) - (T - 1) / 2.0)
    y = np.pi * np.where(arg == 0, 1.0e-20, arg)
    h = 2.0 * cutoff * (np.sin(y) / y) * win
    h = h / h.sum()
    R = 1
    fr = []
    for c in centres:
        c = Fraction(c)
        num, den = c.numerator, c.denominator
        g = den // gcd(num * decim, den)      # the period of centre * decim
        R = R * g // gcd(R, g)
        fr.append((num, den))
    if R > 65536:
        raise ValueError("rotation period too long")
    t = np.empty((len(fr), T), np.complex128)
    r = np.empty((len(fr), R), np.complex128)
    for i, (num, den) in enumerate(fr):
        pt = 2.0 * np.pi * np.array([((num * k) % den) / den for k in range(T)])
        pr = 2.0 * np.pi * np.array([((num * decim * m) % den) / den for m in range(R)])
        t[i] = h * (np.cos(pt) - 1j * np.sin(pt))
        r[i] = np.cos(pr) - 1j * np.sin(pr)
    return t.astype(np.complex64), r.astype(np.complex64), R, alpha
