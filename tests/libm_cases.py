"""Input sets of the libm parity tests (pure numpy, deterministic).

csrc/libm_exact.h restates glibc's sincosf / atan2f / cabsf / logf / log10f;
tests/test_gpu_libm.py runs what hipcc makes of it for the device over these
sets (lphy_hip_test_libm, csrc/lphy_testing.h) and tests/test_libm_cases_cpu.py
runs the host build over the same sets, both against glibc through the oracle
(Oracle.libm).  The sets are built from bit patterns so that every branch of
the header is entered and every threshold is met from both sides
(test_libm_cases_cpu.py asserts that on the sets themselves); a set holds at
most 2^22 elements.

cases(op) -> {set name: (a, b)}, float32 arrays; b is None for the ops with
one argument.
"""
from __future__ import annotations

import functools

import numpy as np

# lphy_test_libm_op (csrc/lphy_testing.h), lphy.LIBM_*
OPS = {"sincos_exact": 0, "sincos_split": 1, "sincos_large": 2, "atan2": 3, "cabs": 4, "logf": 5, "log10f": 6,
       "sqrtf": 7, "detector_power": 8}
ONE_ARG = ("sincos_exact", "sincos_split", "sincos_large", "logf", "log10f", "sqrtf")
MAX_SET = 1 << 22

SIGN = np.uint32(0x80000000)
SUB_MIN, SUB_MAX, FLT_MIN, FLT_MAX, INF = 0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000
ONE, TWO25 = 0x3f800000, 0x4c000000
# quiet NaNs (mantissa bit 22 set) and signalling ones, several payloads
NANS = (0x7fc00000, 0x7fc00001, 0x7fd55555, 0x7fffffff, 0x7f800001, 0x7fa00000, 0x7f855555, 0x7fbfffff)
# the one-argument functions' thresholds: sincosf_needs_large (120.0f),
# glibc's tiny-argument shortcut 2^-12, 1.0f (logf's early return, log10f's
# k < 0 split) and logf's OFF
EDGE_CENTRES = (0x42f00000, 0x39800000, ONE, 0x3f330000)
EDGE_SPAN = 1 << 16
PIO4_K = range(1, 161)   # k pi/4: the quadrant rounding of sincosf_fast up to 40 pi > 120
PIO4_SPAN = 512
# phy.cpp's compensation angle rate * i, rate = -2 pi cfo / N in float32
WORK_CFO = (0.5, -0.5, 0.37, 1e-4, 3.0, -40.0)
WORK_N = (128, 4096)
WORK_I = 1 << 16
# atanf's argument reduction thresholds (s_atanf.c) as quotients |y / x|
ATAN_T = {"2^-29": 0x31000000, "7/16": 0x3ee00000, "11/16": 0x3f300000, "19/16": 0x3f980000, "39/16": 0x401c0000,
          "2^25": TWO25}
ATAN_SPAN = 1024
EXPDIFF_K = range(-70, 71)
BIN_N = (128, 4096)
# detector_power's power_scale: the context's for SF 7 and SF 12
# ((float)(20 log10 N), lphy_hip_ctx_create), none, and a negative one
POWER_SCALES = (float(np.float32(20.0 * np.log10(128.0))), float(np.float32(20.0 * np.log10(4096.0))), 0.0, -3.5)


def f32(bits) -> np.ndarray:
    """uint32 bit patterns -> float32 (no conversion: signalling NaNs stay)."""
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def both_signs(u) -> np.ndarray:
    u = np.ascontiguousarray(u, np.uint32).reshape(-1)
    return np.concatenate([u, u | SIGN])


# ---- one argument ------------------------------------------------------------
@functools.lru_cache(None)
def exponent_grid() -> np.ndarray:
    """Both signs x every biased exponent 0..254 x 4096 mantissas: the 1024
    lowest, the 1024 highest, 2048 random ones per exponent."""
    rng = np.random.default_rng(0x6c70_6879)
    man = np.empty((255, 4096), np.uint32)
    man[:, :1024] = np.arange(1024, dtype=np.uint32)
    man[:, 1024:2048] = np.arange((1 << 23) - 1024, 1 << 23, dtype=np.uint32)
    man[:, 2048:] = rng.integers(0, 1 << 23, (255, 2048), dtype=np.uint32)
    u = (np.arange(255, dtype=np.uint32)[:, None] << np.uint32(23)) | man
    return f32(both_signs(u))


@functools.lru_cache(None)
def edges() -> np.ndarray:
    """Every bit pattern within 2^16 of each threshold and the 512 patterns
    either side of the float nearest k pi/4, k = 1..160; both signs."""
    span = np.arange(-EDGE_SPAN, EDGE_SPAN + 1, dtype=np.int64)
    parts = [(c + span).astype(np.uint32) for c in EDGE_CENTRES]
    near = np.arange(-PIO4_SPAN, PIO4_SPAN + 1, dtype=np.int64)
    for k in PIO4_K:
        c = int(bits(np.float32(k * np.pi / 4))[0])
        parts.append((c + near).astype(np.uint32))
    return f32(both_signs(np.concatenate(parts)))


@functools.lru_cache(None)
def specials() -> np.ndarray:
    u = [0, SUB_MIN, SUB_MAX, FLT_MIN, FLT_MAX, INF, ONE, ONE - 1, ONE + 1, 0x42f00000, 0x42efffff, *NANS]
    return f32(both_signs(np.array(u, np.uint32)))


@functools.lru_cache(None)
def workload() -> np.ndarray:
    """np.float32(rate) * np.float32(i), the compensation's angles: the two
    largest |cfo| take i * rate far past 120 rad."""
    i = np.arange(WORK_I, dtype=np.float32)
    out = []
    for cfo in WORK_CFO:
        for n in WORK_N:
            rate = np.float32(-2.0) * np.float32(np.pi) * np.float32(cfo) / np.float32(n)
            out.append(rate * i)
    return np.concatenate(out).astype(np.float32)


def one_arg_sets() -> dict:
    return {"grid": exponent_grid(), "edges": edges(), "specials": specials(), "workload": workload()}


# ---- atan2f --------------------------------------------------------------------
def special_list(finite_only: bool = False) -> np.ndarray:
    u = [0, SUB_MIN, SUB_MAX, FLT_MIN, ONE - 1, ONE, ONE + 1, TWO25 - 1, TWO25, TWO25 + 1, FLT_MAX,
         0x3f000000, 0x40400000]   # (0.5 and 3: ordinary partners of the special values)
    if not finite_only:
        u += [INF, *NANS]
    return f32(both_signs(np.array(u, np.uint32)))


def cross(v: np.ndarray):
    y, x = np.meshgrid(v, v, indexing="ij")
    return np.ascontiguousarray(y.reshape(-1)), np.ascontiguousarray(x.reshape(-1))


def _quadrants(y, x):
    """(y, x) of non-negative arrays in all four sign quadrants."""
    ys = np.concatenate([y, -y, y, -y])
    xs = np.concatenate([x, x, -x, -x])
    return ys.astype(np.float32), xs.astype(np.float32)


@functools.lru_cache(None)
def atan2_expdiff():
    """For every k = (iy - ix) >> 23 in -70..70 (across atan2f's +-60 and
    atanf's 2^+-25): 256 random mantissa pairs, x at the bottom, in the middle
    and at the top of the exponent range, four quadrants.  Then operands whose
    quotient is subnormal or underflows to zero: y subnormal or barely normal
    under x of every exponent from 2^-24 up."""
    rng = np.random.default_rng(0x6174_616e)
    ys, xs = [], []
    for k in EXPDIFF_K:
        lo, hi = max(1, 1 - k), min(254, 254 - k)   # x's exponent field, y's = that + k, both normal
        for ex in (lo, (lo + hi) // 2, hi):
            n = 256 if ex == (lo + hi) // 2 else 64
            mx = rng.integers(0, 1 << 23, n, dtype=np.uint32)
            my = rng.integers(0, 1 << 23, n, dtype=np.uint32)
            xs.append(np.uint32(ex << 23) | mx)
            ys.append(np.uint32((ex + k) << 23) | my)
    for ex in range(103, 255):
        n = 32
        xs.append(np.uint32(ex << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint32))
        # subnormals of every size, FLT_MIN's neighbourhood
        ys.append(np.where(np.arange(n) % 4 == 3, np.uint32(FLT_MIN) + rng.integers(0, 1 << 24, n, dtype=np.uint32),
                           rng.integers(1, 1 << 23, n, dtype=np.uint32) >> rng.integers(0, 23, n).astype(np.uint32))
                  .astype(np.uint32))
    return _quadrants(f32(np.concatenate(ys)), f32(np.concatenate(xs)))


@functools.lru_cache(None)
def atan2_edges():
    """x random in [2^-3, 2^12), y = x * t with t the 1024 bit patterns either
    side of each of atanf's thresholds: the quotients y / x fall on both sides
    of every one of them.  The same t as y under x == 1.0f, atan2f's shortcut
    to atanf(y)."""
    rng = np.random.default_rng(0x6564_6765)
    ys, xs = [], []
    span = np.arange(-ATAN_SPAN, ATAN_SPAN + 1, dtype=np.int64)
    for thr in ATAN_T.values():
        t = f32((thr + span).astype(np.uint32))
        for _ in range(8):
            x = f32(rng.integers(124 << 23, 139 << 23, t.size, dtype=np.uint32))
            xs.append(x)
            ys.append(x * t)
        # and under x == 1.0f, atan2f's shortcut to atanf(y)
        xs.append(np.ones(t.size, np.float32))
        ys.append(t)
    return _quadrants(np.concatenate(ys), np.concatenate(xs))


def _bins(rng, count):
    """FFT-bin-like pairs: normal, sigma = N for N = 128 and 4096."""
    sig = np.repeat(np.array(BIN_N, np.float32), count // 2)
    return ((rng.standard_normal(count).astype(np.float32) * sig).astype(np.float32),
            (rng.standard_normal(count).astype(np.float32) * sig).astype(np.float32))


def _log_uniform(rng, count, lo_exp, hi_exp):
    """Random signs and mantissas, exponent fields uniform in [lo_exp, hi_exp]."""
    def one():
        u = (rng.integers(lo_exp, hi_exp + 1, count, dtype=np.uint32) << np.uint32(23)) \
            | rng.integers(0, 1 << 23, count, dtype=np.uint32) \
            | (rng.integers(0, 2, count, dtype=np.uint32) << np.uint32(31))
        return f32(u)
    return one(), one()


@functools.lru_cache(None)
def atan2_bins():
    rng = np.random.default_rng(0x6269_6e73)
    y0, x0 = _bins(rng, 1 << 20)
    y1, x1 = _log_uniform(rng, 1 << 18, 64, 190)   # 2^-63 .. 2^63: every k of atan2f, mostly |k| <= 60
    return np.concatenate([y0, y1]), np.concatenate([x0, x1])


# ---- cabsf (finite inputs: the header's contract) ---------------------------------
@functools.lru_cache(None)
def cabs_loguniform():
    """Exponent fields over the whole range, 0 (subnormals) to 254: results
    that overflow to inf, subnormal results, operands that vanish beside the
    other."""
    rng = np.random.default_rng(0x6162_7321)
    a0, b0 = _log_uniform(rng, 1 << 19, 0, 254)
    # equal exponents (both operands count), with the extremes over-weighted
    e = np.concatenate([rng.integers(0, 255, 1 << 18, dtype=np.uint32), rng.integers(0, 3, 1 << 16, dtype=np.uint32),
                        rng.integers(252, 255, 1 << 16, dtype=np.uint32)])
    def one():
        return f32((e << np.uint32(23)) | rng.integers(0, 1 << 23, e.size, dtype=np.uint32)
                   | (rng.integers(0, 2, e.size, dtype=np.uint32) << np.uint32(31)))
    return np.concatenate([a0, one()]), np.concatenate([b0, one()])


@functools.lru_cache(None)
def cabs_bins():
    return _bins(np.random.default_rng(0x6361_6273), 1 << 20)


# ---- detector_power ------------------------------------------------------------------
def detector_sets() -> dict:
    """max_value: the one-argument sets' non-negative members (and their
    sign-clear NaNs), each under every power_scale."""
    out = {}
    for name, a in one_arg_sets().items():
        v = a[(bits(a) < SIGN) | (a == 0)]
        out[name] = (np.tile(v, len(POWER_SCALES)), np.repeat(np.array(POWER_SCALES, np.float32), v.size))
    return out


def cases(op: str) -> dict:
    if op in ONE_ARG:
        return {k: (a, None) for k, a in one_arg_sets().items()}
    if op == "atan2":
        return {"specials": cross(special_list()), "expdiff": atan2_expdiff(), "edges": atan2_edges(),
                "bins": atan2_bins()}
    if op == "cabs":
        return {"specials": cross(special_list(finite_only=True)), "loguniform": cabs_loguniform(),
                "bins": cabs_bins()}
    if op == "detector_power":
        return detector_sets()
    raise KeyError(op)


def needs_large(a) -> np.ndarray:
    """sincosf_needs_large: |y| >= 120, Inf, NaN."""
    return ((bits(a) >> np.uint32(20)) & np.uint32(0x7ff)) >= 0x42f


def reference(op: str, a, b, oracle, host):
    """What the probe must return, bit for bit: glibc's value (Oracle.libm).
    One op has a second reference.  sincosf_large is glibc's Payne-Hanek
    path, which glibc itself enters only for |y| >= 120, Inf and NaN; below
    120 glibc's sincosf reduces with x - n pi/2 in double instead, whose
    rounding differs from the exact reduction at a few arguments next to a
    multiple of pi/2 (0x418a3ada = 17.278736 is one), and below 2 the
    exponent bits (xi >> 26) & 15 select the window of y 2^128.  So for
    sincos_large glibc is the reference where glibc runs that path, and the
    host build of the same header text (checkers.HostLibm) everywhere else:
    no input is left out."""
    want = oracle.libm(OPS[op], a, b)
    if op != "sincos_large":
        return want
    own = host.libm(OPS[op], a, b)
    big = needs_large(a)
    return tuple(np.where(big, w, o) for w, o in zip(want, own))


def mismatches(got, want) -> np.ndarray:
    """Indices where two results differ: bit for bit, NaNs as NaN-ness
    (the rule of _nan_bits_equal, tests/test_oracle_vs_reference.py)."""
    bad = np.zeros(np.asarray(got[0]).size, bool)
    for g, w in zip(got, want):
        if w is None:
            assert g is None
            continue
        ng, nw = np.isnan(g), np.isnan(w)
        bad |= (ng != nw) | (~ng & (bits(g) != bits(w)))
    return np.flatnonzero(bad)


def report(op, a, b, idx, **results) -> str:
    """The first few differing inputs as hex with each party's value."""
    lines = []
    for j in idx[:8]:
        arg = f"a={int(bits(a)[j]):#010x}" + ("" if b is None else f" b={int(bits(b)[j]):#010x}")
        vals = " ".join(f"{k}=" + "/".join(f"{int(bits(r)[j]):#010x}" for r in v if r is not None)
                        for k, v in results.items())
        lines.append(f"{op}: {arg} {vals}")
    return "\n".join(lines)


SET_NAMES = {op: (("grid", "edges", "specials", "workload") if op in ONE_ARG or op == "detector_power" else
                  ("specials", "expdiff", "edges", "bins") if op == "atan2" else ("specials", "loguniform", "bins"))
             for op in OPS}
CASES = [(op, s) for op in OPS for s in SET_NAMES[op]]
