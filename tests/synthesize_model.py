"""The synthesiser's definition (include/lphy_hip.h, lphy_hip_synthesize) in
plain numpy float32, and the design helper's float64 maths written out on its
own.  The tests compare the library with this byte for byte.

synthesize(): vectorised over the outputs n, Python loops over the channels c
and the taps i of a chain, so every product, sum and difference is one float32
numpy operation in the definition's order (numpy neither fuses nor
reassociates element-wise operations).  An output whose chain has no tap i
keeps its accumulator (np.where selects, it does not compute)."""
from fractions import Fraction
from math import gcd

import numpy as np


def outputs(in_samples, first, taps, interp):
    """The outputs from `first` up to the last one an input sample reaches."""
    if taps == 0 or interp == 0 or in_samples == 0:
        return 0
    return max(0, (in_samples - 1) * interp + taps - first)


def synthesize(x, taps, rot, interp, first=0, n_out=None, rot_first=0):
    """x: complex64 [C, in_samples]; taps: complex64 [C, T]; rot: complex64
    [C, R].  Returns complex64 [n_out]."""
    x = np.ascontiguousarray(x, np.complex64)
    taps = np.ascontiguousarray(taps, np.complex64)
    rot = np.ascontiguousarray(rot, np.complex64)
    C, T = taps.shape
    R = rot.shape[1]
    U = int(interp)
    n_in = x.shape[1]
    assert x.shape[0] == C and rot.shape[0] == C
    if n_out is None:
        n_out = outputs(n_in, first, T, U)
    w = first + np.arange(n_out, dtype=np.int64)
    q, p = w // U, w % U
    zero = np.zeros(n_out, np.float32)
    yr, yi = zero.copy(), zero.copy()
    with np.errstate(all="ignore"):
        for c in range(C):
            ar, ai = zero.copy(), zero.copy()
            sr, si = x[c].real, x[c].imag
            for i in range((T - 1) // U + 1 if T else 0):
                k = i * U + p
                tap = k < T
                j = q - i
                have = (j >= 0) & (j < n_in)
                jc = np.where(have, j, 0)
                if n_in:
                    ridx = (rot_first % R + jc % R) % R
                    re, im = sr[jc], si[jc]
                    rr, rim = rot[c, ridx].real, rot[c, ridx].imag
                    xr = np.where(have, re * rr - im * rim, zero)
                    xi = np.where(have, re * rim + im * rr, zero)
                else:
                    xr, xi = zero, zero
                g = taps[c, np.where(tap, k, 0)]
                gr, gi = g.real, g.imag
                pr = xr * gr - xi * gi
                pi = xr * gi + xi * gr
                ar = np.where(tap, ar + pr, ar)
                ai = np.where(tap, ai + pi, ai)
            yr = yr + ar
            yi = yi + ai
    out = np.empty(n_out, np.complex64)
    out.real, out.imag = yr, yi
    return out


def design(centres, interp, taps, cutoff, beta):
    """(taps complex64 [C, T], rot complex64 [C, R], R, delay): `interp` times
    a Kaiser(beta) windowed sinc with its edge at `cutoff` cycles per wideband
    sample and unit gain at DC, times the mixer exp(+2 pi i centre k); rot the
    mixer's phase every `interp` samples over its least common period R."""
    T = taps
    alpha = (T - 1) / 2.0
    n = np.arange(0, T)
    if T == 1:
        win = np.ones(1)
    else:
        win = np.i0(beta * np.sqrt(1 - ((n - alpha) / alpha) ** 2.0)) / np.i0(float(beta))
    arg = 2.0 * cutoff * (np.arange(T, dtype=np.float64) - (T - 1) / 2.0)
    y = np.pi * np.where(arg == 0, 1.0e-20, arg)
    h = 2.0 * cutoff * (np.sin(y) / y) * win
    h = h / h.sum() * float(interp)
    R = 1
    fr = []
    for c in centres:
        c = Fraction(c)
        num, den = c.numerator, c.denominator
        g = den // gcd(num * interp, den)      # the period of centre * interp
        R = R * g // gcd(R, g)
        fr.append((num, den))
    if R > 65536:
        raise ValueError("rotation period too long")
    t = np.empty((len(fr), T), np.complex128)
    r = np.empty((len(fr), R), np.complex128)
    for i, (num, den) in enumerate(fr):
        pt = 2.0 * np.pi * np.array([((num * k) % den) / den for k in range(T)])
        pr = 2.0 * np.pi * np.array([((num * interp * m) % den) / den for m in range(R)])
        t[i] = h * (np.cos(pt) + 1j * np.sin(pt))
        r[i] = np.cos(pr) + 1j * np.sin(pr)
    return t.astype(np.complex64), r.astype(np.complex64), R, alpha
