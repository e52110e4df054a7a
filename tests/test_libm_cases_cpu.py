"""The input sets of the libm parity tests (tests/libm_cases.py), without a GPU.

* Coverage: the sets are classified by bit pattern the way csrc/libm_exact.h
  branches, and every branch, both sides of every threshold and every early
  return must be entered by some input.  A condition on the inputs, not a
  measurement: tests/test_gpu_libm.py then runs the device's compile of the
  header over exactly these inputs.
* Host agreement: the host build of the header (tests/cpp/libm_exact_capi.cpp)
  over the same sets equals glibc through the oracle, bit for bit, with no
  input left out.  A device failure then points at the device compile and not
  at a drift of glibc.
"""
import numpy as np
import pytest

import libm_cases as lc

INF = np.uint32(lc.INF)
ABS = np.uint32(0x7fffffff)
SIGN_BIT = np.uint32(0x80000000)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    from checkers import HostLibm
    return HostLibm(tmp_path_factory.mktemp("libm_capi"))


@pytest.fixture(scope="module")
def one_arg():
    """Every input of the one-argument sets."""
    return np.concatenate(list(lc.one_arg_sets().values()))


def has(mask, what):
    assert np.any(mask), f"no input with {what}"
    return True


# ---- sizes ---------------------------------------------------------------------
def test_sets_are_bounded_and_deterministic():
    for op, name in lc.CASES:
        a, b = lc.cases(op)[name]
        assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size <= lc.MAX_SET, (op, name, a.size)
        assert b is None or (b.dtype == np.float32 and b.shape == a.shape)
    lc.exponent_grid.cache_clear()
    again = lc.exponent_grid()
    assert np.array_equal(lc.bits(again), lc.bits(lc.one_arg_sets()["grid"]))
    assert set(lc.SET_NAMES[op] for op in lc.OPS) and all(set(lc.cases(op)) == set(lc.SET_NAMES[op]) for op in lc.OPS)


# ---- sincosf -------------------------------------------------------------------
def payne_hanek(u):
    """sincosf_large's integer reduction on bit patterns -> (n, sign)."""
    table = np.array([0xa2, 0xa2f9, 0xa2f983, 0xa2f9836e, 0xf9836e4e, 0x836e4e44, 0x6e4e4415, 0x4e441529,
                      0x441529fc, 0x1529fc27, 0x29fc2757, 0xfc2757d1, 0x2757d1f5, 0x57d1f534, 0xd1f534dd,
                      0xf534ddc0, 0x34ddc0db, 0xddc0db62, 0xc0db6295, 0xdb629599, 0x6295993c, 0x95993c43,
                      0x993c4390, 0x3c439041], np.uint64)
    u = u.astype(np.uint64)
    idx = (u >> np.uint64(26)) & np.uint64(15)
    shift = (u >> np.uint64(23)) & np.uint64(7)
    m = (((u & np.uint64(0xffffff)) | np.uint64(0x800000)) << shift) & np.uint64(0xffffffff)
    res0 = (m * table[idx]) & np.uint64(0xffffffff)
    res1 = m * table[idx + np.uint64(4)]
    res2 = m * table[idx + np.uint64(8)]
    res0 = (res2 >> np.uint64(32)) | (res0 << np.uint64(32))
    with np.errstate(over="ignore"):
        res0 = res0 + res1
        n = (res0 + (np.uint64(1) << np.uint64(61))) >> np.uint64(62)
    return n.astype(np.int64), (u >> np.uint64(31)).astype(np.int64)


def test_sincos_coverage(one_arg):
    u = lc.bits(one_arg)
    au = u & ABS
    large = lc.needs_large(one_arg)
    # Inf / NaN: the early return of sincosf_large, both signs, quiet and signalling
    for sign in (0, 1):
        s = (u >> np.uint32(31)) == sign
        has(s & (au == INF), f"inf, sign {sign}")
        has(s & (au > INF) & ((au & np.uint32(0x00400000)) != 0), f"quiet NaN, sign {sign}")
        has(s & (au > INF) & ((au & np.uint32(0x00400000)) == 0), f"signalling NaN, sign {sign}")
    # the Payne-Hanek path: every (idx, shift) a finite |y| >= 120 can have.
    # idx = (e >> 3) & 15 and shift = e & 7 of the biased exponent e, which is
    # 133 (120 = 1.875 * 2^6) .. 254: all 16 idx, all 8 shifts, and every pair
    # of them but idx 0 with shift < 5 (|y| < 64) and idx 15 with shift 7 (Inf)
    fin = large & (au < INF)
    e = (au[fin] >> np.uint32(23)).astype(np.int64)
    pairs = set(zip(((e >> 3) & 15).tolist(), (e & 7).tolist()))
    want = {((x >> 3) & 15, x & 7) for x in range(133, 255)}
    assert pairs == want and len(want) == 122
    assert {p[0] for p in pairs} == set(range(16)) and {p[1] for p in pairs} == set(range(8))
    # hence every window i = idx, idx + 4, idx + 8 of the device's
    # inv_pio4_shift: its three k and both r == 0 and r != 0
    win = {i + d for i, _ in pairs for d in (0, 4, 8)}
    assert win == set(range(24))
    assert {(8 * (23 - i)) >> 6 for i in win} == {0, 1, 2} and {(8 * (23 - i)) & 63 == 0 for i in win} == {True, False}
    # its quadrants: (n + sign) & 3 and n & 1, for both signs of y
    n, sign = payne_hanek(u[fin])
    assert {(int(q), int(s)) for q, s in zip(((n + sign) & 3).tolist(), sign.tolist())} == \
        {(q, s) for q in range(4) for s in (0, 1)}
    assert set((n & 1).tolist()) == {0, 1}
    # both sides of the threshold 120.0f, both signs
    for sgn in (0, SIGN_BIT):
        has(u == np.uint32(0x42f00000 | sgn), "120.0f")
        has(u == np.uint32(0x42efffff | sgn), "the float below 120.0f")
    # the fast path: every quadrant n & 3 for both signs; n == 0 (|y| < pi/4)
    small = one_arg[~large].astype(np.float64)
    n = ((small * float.fromhex("0x1.45F306DC9C883p+23")).astype(np.int32) + np.int32(0x800000)) >> np.int32(24)
    for neg in (False, True):
        assert set((n[(small < 0) == neg] & 3).tolist()) == {0, 1, 2, 3}
    us, aus = u[~large], au[~large]
    has((n == 0) & (aus >= np.uint32(0x39800000)), "n == 0 above 2^-12")
    has((aus < np.uint32(0x39800000)) & (aus >= np.uint32(lc.FLT_MIN)), "|y| < 2^-12, normal")
    has((aus < np.uint32(lc.FLT_MIN)) & (aus > 0), "subnormal y")
    has(us == 0, "+0")
    has(us == SIGN_BIT, "-0 (the sign the y == 0 select restores)")
    has(aus == np.uint32(0x39800000), "2^-12")
    has(aus == np.uint32(0x397fffff), "the float below 2^-12")
    # the quadrant rounding ((int32_t)r + 0x800000) >> 24: on both sides of
    # every odd multiple of pi/4 below 120 some neighbour of it lands
    near = np.arange(-lc.PIO4_SPAN, lc.PIO4_SPAN + 1, dtype=np.int64)
    present = set(aus.tolist())
    for k in lc.PIO4_K:
        if k % 2 == 0 or k * np.pi / 4 >= 120:
            continue
        c = int(lc.bits(np.float32(k * np.pi / 4))[0])
        pat = (c + near).astype(np.uint32)
        assert present.issuperset(pat.tolist())
        x = lc.f32(pat).astype(np.float64)
        nk = ((x * float.fromhex("0x1.45F306DC9C883p+23")).astype(np.int32) + np.int32(0x800000)) >> np.int32(24)
        assert set(nk.tolist()) == {(k - 1) // 2, (k + 1) // 2}, k
    # the workload's own angles reach the large path
    w = lc.workload()
    has(lc.needs_large(w) & (w > 0), "compensation angle >= 120") and has(lc.needs_large(w) & (w < 0), "<= -120")


# ---- logf / log10f ---------------------------------------------------------------
def test_log_coverage(one_arg):
    with np.errstate(all="ignore"):
        u = lc.bits(one_arg)
        # logf_exact_t's early returns
        has(u == np.uint32(lc.ONE), "1.0f")
        has(u == 0, "+0") and has(u == SIGN_BIT, "-0")
        has(u == INF, "+inf")
        has((u & SIGN_BIT != 0) & (u != SIGN_BIT) & ((u & ABS) <= INF), "negative")
        has((u & ABS) > INF, "NaN")
        sub = (u > 0) & (u < np.uint32(lc.FLT_MIN))
        has(sub, "subnormal (x * 0x1p23f)")
        has(u == 1, "the smallest subnormal") and has(u == np.uint32(lc.SUB_MAX), "the largest subnormal")
        # logf_eval: the 16 table intervals, k < 0 / == 0 / > 0, both sides of OFF
        pos = (u >= np.uint32(lc.FLT_MIN)) & (u < INF)
        ix = np.concatenate([u[pos], lc.bits(one_arg[sub] * np.float32(2.0 ** 23)) - np.uint32(23 << 23)])
        tmp = ix - np.uint32(0x3f330000)
        assert set(((tmp >> np.uint32(19)) % 16).tolist()) == set(range(16))
        k = tmp.view(np.int32) >> 23
        has(k < 0, "logf k < 0") and has(k == 0, "logf k == 0") and has(k > 0, "logf k > 0")
        assert k.min() == -149 and k.max() == 128    # the smallest subnormal 2^-149 .. FLT_MAX (z < 1 there)
        has(u == np.uint32(0x3f330000), "OFF") and has(u == np.uint32(0x3f32ffff), "the float below OFF")
        # log10f_exact_t: zero, negative, subnormal (x *= two25), Inf / NaN, and
        # the k < 0 split at 1.0f from both sides; log10f hands logf_exact only
        # [0.5, 2), so its intervals are those of the grid's two binades
        has(u == np.uint32(0x3f7fffff), "the float below 1.0f (k = -1)")
        has(u == np.uint32(0x3f800001), "the float above 1.0f")
        for e in (126, 127):
            m = ((u >> np.uint32(23)) == e)
            t = u[m] - np.uint32(0x3f330000)
            assert len(set(((t >> np.uint32(19)) % 16).tolist())) >= 8, e


# ---- atan2f ----------------------------------------------------------------------
def atan2_all():
    ys, xs = zip(*lc.cases("atan2").values())
    return np.concatenate(ys), np.concatenate(xs)


def test_atan2_coverage():
    y, x = atan2_all()
    uy, ux = lc.bits(y), lc.bits(x)
    iy, ix = uy & ABS, ux & ABS
    ny, nx = uy >> np.uint32(31), ux >> np.uint32(31)
    m = (ny | (nx << np.uint32(1))).astype(np.int64)
    k = (iy.astype(np.int64) - ix.astype(np.int64)) >> 23
    label = np.full(y.size, -1)
    todo = np.ones(y.size, bool)

    def take(mask, name):
        nonlocal todo
        sel = todo & mask
        label[sel] = name
        todo = todo & ~mask
        return sel

    nan = take((ix > INF) | (iy > INF), 0)
    one = take(ux == np.uint32(lc.ONE), 1)
    y0 = take(iy == 0, 2)
    x0 = take(ix == 0, 3)
    ii = take((ix == INF) & (iy == INF), 4)
    xi = take(ix == INF, 5)
    yi = take(iy == INF, 6)
    hi = take(k > 60, 7)
    lo = take((nx == 1) & (k < -60), 8)
    div = take(np.ones(y.size, bool), 9)
    has(nan & (ix > INF) & (iy <= INF), "NaN x only") and has(nan & (iy > INF) & (ix <= INF), "NaN y only")
    for sel, what, ms in ((y0, "y == 0", range(4)), (ii, "inf, inf", range(4)), (xi, "x inf", range(4)),
                          (hi, "k > 60", range(4)), (lo, "x < 0, k < -60", (2, 3)), (div, "y / x", range(4))):
        assert set(m[sel].tolist()) == set(ms), what
    for sel, what in ((x0, "x == 0"), (yi, "y inf")):
        assert set(ny[sel].tolist()) == {0, 1}, what
    # the thresholds on k from both sides, and k < -60 with x > 0 (which divides)
    for kk in (60, 61):
        has((hi | div) & (k == kk), f"k == {kk}")
    for kk in (-60, -61):
        has((lo | div) & (k == kk) & (nx == 1), f"k == {kk}, x < 0") and has(div & (k == kk) & (nx == 0), f"k == {kk}, x > 0")
    assert set(k[div | hi | lo].tolist()) >= set(lc.EXPDIFF_K)
    # atanf_exact's argument: y itself after the x == 1.0f shortcut (either
    # sign), |y / x| otherwise
    with np.errstate(all="ignore"):
        q = lc.bits(y[div] / x[div]) & ABS
    a1 = iy[one]
    for arg, what, signs in ((q, "y / x", None), (a1, "x == 1", ny[one])):
        has(arg >= np.uint32(lc.TWO25), f"{what}: |arg| >= 2^25")
        has(arg < np.uint32(0x31000000), f"{what}: |arg| < 2^-29")
        edges = [0x31000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, lc.TWO25]
        for a, b in zip(edges[:-1], edges[1:]):
            sel = (arg >= np.uint32(a)) & (arg < np.uint32(b))
            has(sel, f"{what}: arg in [{a:#x}, {b:#x})")
            if signs is not None and a >= 0x3ee00000:
                assert set(signs[sel].tolist()) == {0, 1}, f"{what}: both signs in [{a:#x}, {b:#x})"
    has((a1 == INF), "atanf(inf) through x == 1") and has(one & (iy == 0), "atanf(0) through x == 1")
    # both sides of each threshold by one bit pattern
    for name, thr in lc.ATAN_T.items():
        has(q == np.uint32(thr), f"quotient {name}") and has(q == np.uint32(thr - 1), f"quotient just below {name}")
    # subnormal operands and quotients, quotients that underflow to zero
    has(q == 0, "a quotient that underflows to zero (y != 0)")
    has((q > 0) & (q < np.uint32(lc.FLT_MIN)), "a subnormal quotient")
    has(div & (iy < np.uint32(lc.FLT_MIN)), "subnormal y") and has(div & (ix < np.uint32(lc.FLT_MIN)), "subnormal x")
    has(div & (ix < np.uint32(lc.FLT_MIN)) & (iy < np.uint32(lc.FLT_MIN)), "both subnormal")
    # z below 2^-29 returned as it is, in every quadrant's final expression
    qfull = np.zeros(y.size, np.uint32)
    qfull[div] = q
    assert set(m[div & (qfull < np.uint32(0x31000000))].tolist()) == {0, 1, 2, 3}


# ---- cabsf / detector_power ---------------------------------------------------------
def test_cabs_and_detector_coverage():
    for name, (a, b) in lc.cases("cabs").items():
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), name   # the header's contract
    a, b = (np.concatenate(v) for v in zip(*lc.cases("cabs").values()))
    r = np.sqrt(a.astype(np.float64) ** 2 + b.astype(np.float64) ** 2)
    flt_max, flt_min = float(lc.f32([lc.FLT_MAX])[0]), float(lc.f32([lc.FLT_MIN])[0])
    has(r > flt_max * (1 + 2.0 ** -24), "a result that overflows to inf")
    has((r > flt_max * (1 - 2.0 ** -20)) & (r <= flt_max), "a result just below FLT_MAX")
    has((r > 0) & (r < flt_min), "a subnormal result")
    has(r == 0, "0, 0")
    ua, ub = lc.bits(a) & ABS, lc.bits(b) & ABS
    has((ua < np.uint32(lc.FLT_MIN)) & (ua > 0) & (ub >= np.uint32(lc.FLT_MIN)), "one subnormal operand")
    has((ua >> np.uint32(23)) == (ub >> np.uint32(23)), "equal exponents")
    for name, (v, s) in lc.cases("detector_power").items():
        assert not np.any(v < 0), name
        assert set(np.unique(s).tolist()) == set(np.float32(lc.POWER_SCALES).tolist())
    v = np.concatenate([c[0] for c in lc.cases("detector_power").values()])
    uv = lc.bits(v)
    has(uv == 0, "max_value 0") and has(uv == INF, "inf") and has((uv > 0) & (uv < np.uint32(lc.FLT_MIN)), "subnormal")
    assert np.float32(20.0 * np.log10(128.0)) in np.float32(lc.POWER_SCALES)
    assert np.float32(20.0 * np.log10(4096.0)) in np.float32(lc.POWER_SCALES)


# ---- the host build of the header against glibc --------------------------------------
@pytest.mark.parametrize("op,name", lc.CASES, ids=[f"{o}-{s}" for o, s in lc.CASES])
def test_host_header_equals_glibc(oracle, host, op, name):
    a, b = lc.cases(op)[name]
    got = host.libm(lc.OPS[op], a, b)
    glibc = oracle.libm(lc.OPS[op], a, b)
    want = lc.reference(op, a, b, oracle, host)
    bad = lc.mismatches(got, want)
    assert bad.size == 0, f"{bad.size} of {a.size} differ\n" + lc.report(op, a, b, bad, header=got, glibc=glibc)
    if op == "sincos_large":
        # where glibc itself takes this path the reference is glibc alone
        big = lc.needs_large(a)
        assert big.any() or name == "specials"
        assert lc.mismatches([g[big] for g in got], [g[big] for g in glibc]).size == 0


def test_sincos_large_below_120_is_a_sine(host):
    """Below 120 sincosf_large is no longer glibc's sincosf bit for bit (a few
    arguments next to a multiple of pi/2 round the other way, lc.reference),
    but from 2 up it is the sine and cosine all the same: within 1 ulp of the
    float result (glibc documents 0.56 ulp for the polynomial this path
    shares), against numpy's double precision."""
    a = np.concatenate(list(lc.one_arg_sets().values()))
    a = a[(np.abs(a) >= 2) & ~lc.needs_large(a)]
    assert a.size > 100000
    sn, cs = host.libm(lc.OPS["sincos_large"], a)
    x = a.astype(np.float64)
    for got, want in ((sn, np.sin(x)), (cs, np.cos(x))):
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.max(np.abs(got.astype(np.float64) - want) / ulp) < 1.0
