"""lphy_hip_detect_ragged_host without a device: its staging plan
(csrc/lphy_stage_plan.h detect_ragged_plan), the reservation that has to cover
it, and the check of the caller's table (csrc/lphy_ragged_layout.h
detect_ragged_extent), compiled into a host-only test library
(tests/cpp/detect_ragged_plan_check.cpp) as tests/test_stage_plan_cpu.py does
for the other plans."""
import ctypes as C
import errno
import itertools

import numpy as np
import pytest

import hostcc
from test_estimate_ragged_cpu import _mod_scratch


IN, OUT = 1, 2
REC, DESC, IQ = 16, 32, 8


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = hostcc.shared_lib("detect_ragged_plan_check.cpp", tmp_path_factory.mktemp("detect_ragged_plan"))
    L.detect_ragged_plan_check.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.detect_ragged_reserve_check.argtypes = [C.c_uint64] * 5
    L.detect_ragged_reserve_check.restype = C.c_uint64
    L.detect_ragged_extent_check.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    L.demod_ragged_extent_check.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64]
    return L


def _plan(lib, iq_samples, frames, units):
    out = np.zeros(7 + 3 * 5, np.uint64)
    k = lib.detect_ragged_plan_check(iq_samples, frames, units, out.ctypes.data)
    assert k == 7 + 3 * int(out[0])
    n, end, copied_end, ub, ue, db, de = (int(v) for v in out[:7])
    slices = [tuple(int(v) for v in out[7 + 3 * i: 10 + 3 * i]) for i in range(n)]  # (off, size, role)
    return dict(end=end, copied_end=copied_end, up=(ub, ue), down=(db, de), slices=slices)


def _a(x):  # a slice's room: align_up(max(1, x))
    return (max(1, x) + 255) & ~255


# (iq samples, frames, units): empty slices, one byte past the alignment, ordinary calls
SHAPES = [(0, 1, 0), (0, 3, 0), (1, 1, 0), (128, 1, 1), (33, 8, 0), (17 * 128, 8, 17), (8 * 128 + 7, 3, 8),
          (40 * 9000, 40, 40 * 70), (66 * 4096 * 5, 5, 330)]


@pytest.mark.parametrize("iq,frames,units", SHAPES)
def test_plan_slices(lib, iq, frames, units):
    """iq (in) | frames + 1 records (in) | one record per unit (out):
    disjoint, aligned, back to back; the first two go up, the last comes down."""
    p = _plan(lib, iq, frames, units)
    want = [(iq * IQ, IN), ((frames + 1) * DESC, IN), (units * REC, OUT)]
    off, prev_end = 0, 0
    for (o, size, role), (wsize, wrole) in zip(p["slices"], want):
        assert (o, size, role) == (off, wsize, wrole)
        assert o % 256 == 0 and o >= prev_end
        prev_end = o + max(size, 1)
        off += _a(wsize)
    assert len(p["slices"]) == 3 and p["end"] == off == p["copied_end"]
    desc_off, rec_off = p["slices"][1][0], p["slices"][2][0]
    assert p["up"] == ((0 if iq else desc_off), rec_off)
    assert p["down"] == ((rec_off, p["end"]) if units else (0, 0))


@pytest.mark.parametrize("sf,osr,frames", list(itertools.product([7, 9, 12], [1, 2, 4], [1, 3, 40, 1000])))
def test_reservation_covers_the_plan(lib, sf, osr, frames):
    """lphy_hip_ctx_reserve(frames, frame_samples): `frames` frames of up to
    frame_samples each, so an IQ extent of up to frames * frame_samples and at
    most that over N * osr whole symbols (frames of fewer samples, however
    they are cut, hold no more)."""
    N = 1 << sf
    step = N * osr
    for fs in (0, 1, step - 1, step, 2 * step + 5, 66 * step + 3, 67 * step - 1):
        n = frames * fs
        got = lib.detect_ragged_reserve_check(N, osr, frames, fs, _mod_scratch(N, osr, fs // step))
        assert got >= _plan(lib, n, frames, n // step)["end"], (fs,)
        assert got >= _plan(lib, n, frames, frames * (fs // step))["end"], (fs,)


def _extent(lib, step, rows):
    desc = np.array(rows, np.uint64).reshape(-1, 4)
    out = np.zeros(2, np.uint64)
    rc = lib.detect_ragged_extent_check(step, desc.ctypes.data, desc.shape[0] - 1, out.ctypes.data)
    return rc, int(out[0]), int(out[1])


def test_table_check(lib):
    """iq_offset, samples and unit_offset are checked, with the ragged
    demodulator's limits and its answer for a wrong prefix (the step of this
    call is N * osr); sym_offset holds anything."""
    junk = 0xDEADBEEF
    step = 256   # N = 128, osr = 2
    ok = [(900, 3 * step + 5, junk, 0), (0, 0, junk, 3), (100, step, junk, 3), (5000, step - 1, 1 << 60, 4),
          (0, 0, junk, 4)]
    assert _extent(lib, step, ok) == (0, 5000 + step - 1, 4)
    assert _extent(lib, 128, [(0, 0, 0, 0)]) == (0, 0, 0)                       # frames == 0
    assert _extent(lib, 128, [(0, (1 << 31) - 1, 0, 0), (0, 0, 0, (1 << 24) - 1)]) == (0, (1 << 31) - 1, (1 << 24) - 1)
    assert _extent(lib, 128, [(0, 128, 0, 0), (0, 1 << 31, 0, 1), (0, 0, 0, 1)])[0] == -errno.ERANGE
    assert _extent(lib, 128, [((1 << 48) + 1, 0, 0, 0), (0, 0, 0, 0)])[0] == -errno.ERANGE
    assert _extent(lib, 128, [(1 << 48, 4, 0, 0), (0, 0, 0, 0)]) == (0, (1 << 48) + 4, 0)
    # a wrong prefix: in a frame's record, in the totals, and one right at osr 1 only
    for bad in ([(0, 256, 0, 0), (256, 256, 0, 2), (0, 0, 0, 2)],
                [(0, 256, 0, 0), (256, 256, 0, 1), (0, 0, 0, 3)],
                [(0, 256, 0, 1), (0, 0, 0, 2)]):
        rc = _extent(lib, step, bad)[0]
        assert rc == -errno.EINVAL
        d = np.array(bad, np.uint64)
        assert rc == lib.demod_ragged_extent_check(step, d.ctypes.data, len(bad) - 1)
    right_at_osr1 = [(0, 256, 0, 0), (256, 256, 0, 2), (0, 0, 0, 4)]
    assert _extent(lib, 128, right_at_osr1) == (0, 512, 4)
    assert _extent(lib, step, right_at_osr1)[0] == -errno.EINVAL
    # 2^32 whole symbols in the call
    many = [(0, (1 << 31) - 128, 0, k * ((1 << 24) - 1)) for k in range(257)] + [(0, 0, 0, 257 * ((1 << 24) - 1))]
    assert _extent(lib, 128, many)[0] == -errno.ERANGE
