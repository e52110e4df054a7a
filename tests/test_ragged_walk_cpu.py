"""The host-side contract of the ragged descriptor table without a device:
csrc/lphy_ragged_layout.h's one walk over a caller's table, as each *_host
form calls it (demod, detect, estimate, tx), and the ragged entry points'
argument checks, compiled into a host-only test library
(tests/cpp/ragged_walk_check.cpp) and compared with a model written here from
the rules include/lphy_hip.h states, not from the header's code:

* a frame of `total` whole symbols yields total - 2 output symbols, none below
  two in mode 0 and `total` below two in modes 1 and 2;
* per frame, in this order: samples >= 2^31 (-ERANGE), unit_offset not the
  running prefix (-EINVAL), iq_offset or sym_offset above 2^48 (-ERANGE), 2^32
  whole symbols reached (-ERANGE); after the frames, record [frames] not the
  total (-EINVAL).  A call makes only the checks of the fields it reads;
* tx: any of the above in any frame first, then -EINVAL for a frame that is not
  whole symbols, has fewer than two or an odd count.

The checks take "every required pointer is there" as one flag; which pointers
an entry point requires is its own conjunction, and each of those pointers is
nulled in turn by the GPU tests of the calls (test_argument_checks of
test_gpu_ragged, test_gpu_tx_ragged and test_gpu_detect_ragged, the argument
tests of test_gpu_estimate_ragged and test_gpu_compensate_batch).

The same source as a stand-alone program runs under ASan + UBSan."""
import ctypes as C
import errno
import itertools

import numpy as np
import pytest

import hostcc

IQ, SAMPLES, SYM, UNIT = range(4)  # lphy_ragged_desc's fields
DEMOD, DETECT, ESTIMATE, TX, COMPENSATE = range(5)  # ragged_walk_check.cpp's callers (TX: modulate and tx)
EINVAL, ERANGE, ENOTSUP = -errno.EINVAL, -errno.ERANGE, -errno.ENOTSUP
UNTOUCHED = 0xABABABABABABABAB


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = hostcc.shared_lib("ragged_walk_check.cpp", tmp_path_factory.mktemp("ragged_walk"))
    L.rw_walk.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.rw_args.argtypes = [C.c_int, C.c_void_p]
    return L


# ------------------------------------------------------------------ the model
def out_syms(total, mode):
    return np.where(total >= 2, total - np.minimum(total, 2), 0 if mode == 0 else total)


def model(who, step, desc, mode):
    """(rc, outputs) of caller `who` for a table of frames + 1 rows of four integers."""
    d = np.asarray(desc, np.uint64).reshape(-1, 4).astype(object)  # Python integers: nothing wraps
    body, frames = d[:-1], d.shape[0] - 1
    reads_sym, reads_unit = who in (DEMOD, TX), who != ESTIMATE
    mode = 1 if who == TX else 0 if who in (DETECT, ESTIMATE) else mode
    total = body[:, SAMPLES] // step
    before = np.concatenate([[0], np.cumsum(total)])  # whole symbols before frame f; [frames]: all
    # each frame's first failing check, in the order of the checks
    checks = [(body[:, SAMPLES] >= 1 << 31, ERANGE),
              ((body[:, UNIT] != before[:-1]) & reads_unit, EINVAL),
              ((body[:, IQ] > 1 << 48) | ((body[:, SYM] > 1 << 48) & reads_sym), ERANGE),
              ((before[1:] >= 1 << 32) & reads_unit, ERANGE)]
    code = np.zeros(frames, np.int64)
    for bad, rc in reversed(checks):
        code[bad.astype(bool)] = rc
    if code.any():
        return int(code[np.flatnonzero(code)[0]]), None
    if reads_unit and d[-1, UNIT] != before[-1]:
        return EINVAL, None
    per = out_syms(total.astype(np.int64), mode)
    iq = int(max(body[:, IQ] + body[:, SAMPLES], default=0))
    syms = int(max(body[:, SYM] + per, default=0))
    if who == DEMOD:
        return 0, [iq, syms]
    if who == DETECT:
        return 0, [iq, int(before[-1])]
    if who == ESTIMATE:
        return 0, [iq]
    if any((body[:, SAMPLES] % step != 0) | (total < 2) | (total % 2 == 1)):
        return EINVAL, None
    need = int(max(body[:, SYM] // 2 + (total - 2) // 2, default=0))
    return 0, [iq, syms, need, int(sum(body[:, SAMPLES]) != iq), int(sum(total - 2) != syms)]


def call(lib, who, step, desc, mode):
    d = np.ascontiguousarray(desc, np.uint64).reshape(-1, 4)
    out = np.full(5, UNTOUCHED, np.uint64)
    rc = lib.rw_walk(who, step, d.ctypes.data, d.shape[0] - 1, mode, out.ctypes.data)
    if rc:
        assert (out == UNTOUCHED).all()  # a refused table writes nothing
        return rc, None
    n = {DEMOD: 2, DETECT: 2, ESTIMATE: 1, TX: 5}[who]
    assert (out[n:] == UNTOUCHED).all()
    return 0, [int(v) for v in out[:n]]


def agree(lib, step, desc, modes=(0, 1, 2)):
    """Every caller's code and outputs equal the model's; returns the codes (demod: mode modes[0])."""
    codes = []
    for who in (DEMOD, DETECT, ESTIMATE, TX):
        for mode in (modes if who == DEMOD else modes[:1]):
            got, want = call(lib, who, step, desc, mode), model(who, step, desc, mode)
            assert got == want, (who, mode)
            if mode == modes[0]:
                codes.append(got[0])
    return codes


def packed(step, lengths, mode):
    """ragged_layout's table (laid out here: the library's refuses 2^32 whole symbols)."""
    rows, iq, sym, unit = [], 0, 0, 0
    for n in lengths:
        rows.append((iq, n, sym, unit))
        per = int(out_syms(np.int64(n // step), mode))
        iq, sym, unit = iq + n, sym + per + (per & 1), unit + n // step
    return np.array(rows + [(iq, 0, sym, unit)], np.uint64)


# --------------------------------------------------------------- sound tables
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("sf,osr", itertools.product([7, 9, 12], [1, 2]))
def test_packed_tables(lib, sf, osr, mode):
    s = (1 << sf) * osr
    # 0 samples, less than a symbol, exactly 1, 2 and 3 symbols, an odd count, a partial last symbol
    lengths = [0, s - 1, s, 2 * s, 3 * s, 7 * s, 6 * s + 37, 2 * s + 1, 66 * s]
    for ln in [[], lengths, lengths[::-1], [4 * s, 2 * s, 10 * s]] + [[n] for n in lengths]:
        desc = packed(s, ln, mode)
        assert agree(lib, s, desc, (mode,))[:3] == [0, 0, 0]
    # whole frames with even counts: tx accepts the table and sees no gap
    assert call(lib, TX, s, packed(s, [4 * s, 2 * s, 10 * s], 1), 1) == (0, [16 * s, 10, 5, 0, 0])


def test_callers_tables(lib):
    s = 128
    # gaps in the IQ and in the outputs, frames out of address order
    gaps = [(5000, 4 * s, 100, 0), (0, 3 * s + 37, 10, 4), (9000, s, 0, 7), (0, 0, 0, 8)]
    assert agree(lib, s, gaps) == [0, 0, 0, EINVAL]
    assert call(lib, DEMOD, s, gaps, 1) == (0, [9000 + s, 102])
    assert call(lib, DETECT, s, gaps, 0) == (0, [9000 + s, 8])
    # overlapping symbol slots and IQ: the walk measures extents, it does not look for overlaps
    over = [(0, 6 * s, 0, 0), (s, 4 * s, 2, 6), (0, 2 * s, 2, 10), (0, 0, 0, 12)]
    assert agree(lib, s, over) == [0, 0, 0, 0]
    assert call(lib, TX, s, over, 1) == (0, [6 * s, 4, 2, 1, 1])
    # out of order with whole frames: tx's bytes follow sym_offset, the sums see no gap
    swap = [(4 * s, 6 * s, 2, 0), (0, 4 * s, 0, 6), (0, 0, 0, 10)]
    assert call(lib, TX, s, swap, 1) == (0, [10 * s, 6, 3, 0, 0])
    # the fields a call does not read may hold anything
    junk = [(5, 100, 1 << 60, 77), (300, 0, 1 << 63, 7), (0, 0, 0, 99)]
    assert agree(lib, s, junk)[2] == 0 and call(lib, ESTIMATE, s, junk, 0) == (0, [300])
    unread = [(0, 3 * s, 1 << 60, 0), (7, s, (1 << 48) + 1, 3), (0, 0, 5, 4)]
    assert agree(lib, s, unread) == [ERANGE, 0, 0, ERANGE]
    # the limits themselves are allowed
    edge = [(1 << 48, (1 << 31) - 1, 1 << 48, 0), (0, 0, 0, ((1 << 31) - 1) // s)]
    assert agree(lib, s, edge)[:3] == [0, 0, 0]


# -------------------------------------------------------------- forged tables
FAULTS = ["samples", "prefix", "iq", "sym", "units"]
BIG = 257  # frames of 2^24 - 1 symbols (step 128) that reach 2^32 in the last of them


def forged(step, lengths, faults, mode=1):
    """`lengths` packed, then each (fault, frame) applied; 'units' puts BIG frames before `frame`."""
    lengths = list(lengths)
    at = {k: f for k, f in faults}
    if "units" in at:
        assert step == 128
        f = at["units"]
        lengths[f:f] = [(1 << 31) - step] * BIG
        at = {k: (g + BIG if g >= f and k != "units" else g) for k, g in at.items()}
    d = packed(step, lengths, mode)
    for k, f in at.items():
        if k == "samples":
            d[f, SAMPLES] = 1 << 31
        elif k == "prefix":
            d[f, UNIT] += 1
        elif k == "iq":
            d[f, IQ] = (1 << 48) + 1
        elif k == "sym":
            d[f, SYM] = (1 << 48) + 1
    return d


def base(s):
    return [4 * s, 0, 2 * s, 6 * s + 5, 37, 66 * s, 3 * s, s, 2 * s]


# what one fault costs (demod, detect, estimate, tx); tx with nothing else wrong: its own -EINVAL
ALONE = {"samples": [ERANGE] * 4, "prefix": [EINVAL, EINVAL, 0, EINVAL], "iq": [ERANGE] * 4,
         "sym": [ERANGE, 0, 0, ERANGE], "units": [ERANGE, ERANGE, 0, ERANGE]}


# (2^32 whole symbols in frames below 2^31 samples: step 128 alone keeps that table small)
@pytest.mark.parametrize("step,fault", [(s, k) for s in (128, 1024) for k in FAULTS if s == 128 or k != "units"])
def test_one_fault(lib, step, fault):
    n = len(base(step))
    # [n]: record [frames] / the last frames
    for f in [0, n // 2, n - 1] + ([n] if fault in ("prefix", "units") else []):
        if fault == "units" and f == n - 1:
            continue
        desc = forged(step, base(step), [(fault, f)])
        assert agree(lib, step, desc) == ALONE[fault], f


def test_two_faults(lib):
    """Two different faults in two different frames, in both orders: the earlier frame's code,
    for the calls that read both fields."""
    s, n = 128, len(base(128))
    for a, b in itertools.permutations(FAULTS, 2):
        for f, g in ((0, n - 1), (1, n // 2), (n // 2, n - 1)):
            if a == "units":
                f += 1  # (the frame where the count reaches 2^32 is frame f + BIG - 1)
            desc = forged(s, base(s), [(a, f), (b, g)])
            codes = agree(lib, s, desc)
            for who in range(4):
                first, second = ALONE[a][who], ALONE[b][who]
                assert codes[who] == (first or second or (EINVAL if who == TX else 0)), (a, b, f, g, who)


def test_units_fault_sits_where_the_count_reaches_the_limit(lib):
    s = 128
    full = forged(s, base(s), [("units", len(base(s)))])
    assert agree(lib, s, full)[:2] == [ERANGE, ERANGE]
    short = np.concatenate([full[:-2], full[-2:-1]])  # one frame fewer, its record as the total
    short[-1, SAMPLES] = 0
    assert agree(lib, s, short)[:3] == [0, 0, 0]


@pytest.mark.parametrize("kind", ["partial", "one", "odd"])
@pytest.mark.parametrize("fault", ["samples", "iq", "sym", "units"])
def test_tx_own_fault_beside_a_range_fault(lib, kind, fault):
    """tx's own -EINVAL in an earlier or a later frame never hides a fault of the common walk."""
    s = 128
    whole = [4 * s, 2 * s, 6 * s, 2 * s, 10 * s, 4 * s, 8 * s, 2 * s, 4 * s]
    assert agree(lib, s, packed(s, whole, 1))[3] == 0
    n = len(whole)
    for own, f in ((1, n - 2), (n - 2, 1)):
        ln = list(whole)
        ln[own] = {"partial": 4 * s + 1, "one": s, "odd": 3 * s}[kind]
        assert agree(lib, s, packed(s, ln, 1))[3] == EINVAL
        assert agree(lib, s, forged(s, ln, [(fault, f)]))[3] == ERANGE, (own, f)


# ------------------------------------------------------------ argument checks
# A bad argument of every kind, as rw_args takes them: (index, bad value).  The good call:
# ctx, SF 7, osr 1, 3 frames, pointers there, mode 1, LPHY_F_DECODE (detect: LPHY_DET_DECHIRP), phase 0, bytes there.
GOOD = [1, 7, 1, 3, 1, 1, 1, 0, 1]
BAD = {"ctx": (0, 0), "sf6": (1, 6), "osr2": (2, 2), "none": (3, 0), "many": (3, 1 << 31), "ptr": (4, 0),
       "mode": (5, 3), "flag": (6, 0x101), "phase": (7, 1), "bytes": (8, 0)}


def documented(who, a):
    """include/lphy_hip.h's order for entry point `who`."""
    ctx, sf, osr, frames, ptrs, mode, flags, phase, have_bytes = a
    if who == DEMOD:  # pointers, mode, flags, osr and SF, decode without bytes, then frames
        if not ctx or not ptrs or not 0 <= mode <= 2:
            return EINVAL
        if flags & ~0x3 or osr != 1 or sf < 7:  # LPHY_F_DECODE | LPHY_F_NO_SCRATCH
            return ENOTSUP
        if flags & 1 and not have_bytes:
            return EINVAL
        return 0 if frames == 0 else ERANGE if frames >= 1 << 31 else 0
    if not ctx:
        return EINVAL
    if frames == 0:
        return 0
    if not ptrs or (who == DETECT and (flags & ~1 or phase >= osr)):
        return EINVAL
    if frames >= 1 << 31:
        return ERANGE
    return ENOTSUP if sf < 7 and who != COMPENSATE else 0


@pytest.mark.parametrize("who", [DEMOD, DETECT, ESTIMATE, TX, COMPENSATE])
def test_argument_checks(lib, who):
    def rc(bad):
        a = list(GOOD)
        for k in bad:
            a[BAD[k][0]] = BAD[k][1]
        arr = np.array(a, np.uint64)
        got = lib.rw_args(who, arr.ctypes.data)
        assert got == documented(who, a), bad
        return got

    assert lib.rw_args.argtypes and C.sizeof(C.c_size_t) == 8  # frames = 2^31 needs a 64-bit size_t
    assert rc([]) == 0
    for k in BAD:
        rc([k])
    for pair in itertools.combinations(BAD, 2):
        if BAD[pair[0]][0] != BAD[pair[1]][0]:  # ("none" and "many" are one argument)
            rc(pair)
    # a few of the documented orders, spelt out
    assert rc(["ctx", "none"]) == EINVAL
    if who == DEMOD:
        assert rc(["none", "flag"]) == ENOTSUP and rc(["none", "bytes"]) == EINVAL
        assert rc(["osr2"]) == ENOTSUP and rc(["mode", "flag"]) == EINVAL and rc(["many", "sf6"]) == ENOTSUP
    else:
        assert rc(["none", "ptr"]) == 0 and rc(["ptr", "many"]) == EINVAL
        assert rc(["many", "sf6"]) == ERANGE and rc(["osr2"]) == 0
        assert rc(["sf6"]) == (0 if who == COMPENSATE else ENOTSUP)
        assert rc(["flag", "many"]) == (EINVAL if who == DETECT else ERANGE)
        assert rc(["phase"]) == (EINVAL if who == DETECT else 0)


def test_walk_and_checks_under_the_host_sanitizers(tmp_path):
    """The same source as a stand-alone program (-DRAGGED_WALK_MAIN) under ASan + UBSan, on heap
    tables of exactly frames + 1 records."""
    out = hostcc.run_check("ragged_walk_check.cpp", tmp_path, define="RAGGED_WALK_MAIN")
    assert out.strip() == "ragged_walk_check: ok", out
