"""The host arithmetic of the ragged transmit path without a device:
lphy_hip_tx_layout's table (csrc/lphy_ragged_layout.h: tx_layout), the table
checks of lphy_hip_tx_ragged_host (tx_extent) and its staging plan
(csrc/lphy_stage_plan.h: tx_plan), compiled into a host-only test library
(tests/cpp/tx_layout_check.cpp) and called through ctypes:

* tx_layout equals ragged_layout in mode 1 on (2 len + 2) * step samples, and
  every sym_offset / 2 is the exclusive prefix of len;
* -ERANGE where (2 len + 2) * step reaches 2^31, -EINVAL on null pointers;
* tx_extent: the extents, the bytes the frames read, gaps or none, and -EINVAL
  for a partial symbol, a frame below two symbols and an odd symbol count;
* tx_plan: four distinct, ordered slices within kMaxSlices, whose spans cover
  exactly the slices that go in and come out;
* the reservation covers tx_plan at the reserved shape."""
import ctypes as C

import numpy as np
import pytest

import hostcc

DESC = np.dtype([("iq_offset", "<u8"), ("samples", "<u8"), ("sym_offset", "<u8"), ("unit_offset", "<u8")])
EINVAL, ERANGE = -22, -34
IN, OUT, INOUT = 1, 2, 3


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = hostcc.shared_lib("tx_layout_check.cpp", tmp_path_factory.mktemp("tx_layout"))
    L.tx_layout_check.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p]
    L.tx_ragged_layout_check.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p]
    L.tx_extent_check.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p]
    L.tx_plan_check.argtypes = [C.c_void_p, C.c_void_p]
    L.tx_reserve_check.argtypes = [C.c_uint64] * 5
    L.tx_reserve_check.restype = C.c_uint64
    return L


def _tx_layout(lib, sf, osr, lens):
    n = np.ascontiguousarray(lens, np.uint64)
    desc = np.full(n.size + 1, 0xAB, np.uint8).repeat(32).view(DESC)
    rc = lib.tx_layout_check(sf, osr, n.ctypes.data if n.size else None, n.size, desc.ctypes.data)
    return rc, desc


@pytest.mark.parametrize("sf,osr", [(7, 1), (7, 2), (9, 1), (12, 4)])
def test_equals_ragged_layout_on_the_sample_counts(lib, sf, osr):
    step = (1 << sf) * osr
    lens = [0, 1, 2, 3, 5, 9, 16, 33, 0, 64, 1]
    rc, desc = _tx_layout(lib, sf, osr, lens)
    assert rc == 0
    samples = np.array([(2 * n + 2) * step for n in lens], np.uint64)
    want = np.zeros(len(lens) + 1, DESC)
    assert lib.tx_ragged_layout_check(sf, osr, samples.ctypes.data, samples.size, want.ctypes.data) == 0
    np.testing.assert_array_equal(desc, want)
    # bytes of frame f at sym_offset / 2: the exclusive prefix of len
    prefix = np.concatenate([[0], np.cumsum(lens)])
    assert not np.any(desc["sym_offset"] & 1)
    np.testing.assert_array_equal(desc["sym_offset"] // 2, prefix)
    np.testing.assert_array_equal(desc["unit_offset"], np.concatenate([[0], np.cumsum([2 * n + 2 for n in lens])]))
    np.testing.assert_array_equal(desc["samples"][:-1], samples)
    assert desc["samples"][-1] == 0 and desc["iq_offset"][-1] == samples.sum()


def test_no_frames(lib):
    rc, desc = _tx_layout(lib, 8, 1, [])
    assert rc == 0 and desc[0].tolist() == (0, 0, 0, 0)


def test_limits_and_null_pointers(lib):
    # SF 7: (2 len + 2) * 128 < 2^31  <=>  len <= 2^23 - 2
    top = (1 << 23) - 2
    assert _tx_layout(lib, 7, 1, [3, top])[0] == 0
    assert _tx_layout(lib, 7, 1, [3, top + 1])[0] == ERANGE      # the product is 2^31
    assert _tx_layout(lib, 7, 2, [(1 << 22) - 2])[0] == 0         # osr 2: (2 len + 2) * 256
    assert _tx_layout(lib, 7, 2, [(1 << 22) - 1])[0] == ERANGE
    assert _tx_layout(lib, 12, 1, [(1 << 18) - 2])[0] == 0
    assert _tx_layout(lib, 12, 1, [(1 << 18) - 1])[0] == ERANGE
    assert _tx_layout(lib, 7, 1, [1 << 40])[0] == ERANGE
    assert _tx_layout(lib, 7, 1, [(1 << 64) - 1])[0] == ERANGE   # 2 len + 2 would wrap
    n = np.array([4], np.uint64)
    d = np.zeros(2, DESC)
    assert lib.tx_layout_check(7, 1, n.ctypes.data, 1, None) == EINVAL
    assert lib.tx_layout_check(7, 1, None, 1, d.ctypes.data) == EINVAL
    assert lib.tx_layout_check(7, 1, None, 0, d.ctypes.data) == 0


def _extent(lib, sf, osr, desc):
    out = np.zeros(5, np.uint64)
    rc = lib.tx_extent_check(sf, osr, desc.ctypes.data, desc.size - 1, out.ctypes.data)
    return rc, [int(v) for v in out]


def test_extent_of_a_packed_and_of_a_callers_table(lib):
    N = 128
    rc, desc = _tx_layout(lib, 7, 1, [0, 3, 1])
    assert _extent(lib, 7, 1, desc) == (0, [(2 + 8 + 4) * N, 8, 4, 0, 0])
    # gaps in the IQ and in the symbols, frames against their address order
    d = np.array([(9000, 4 * N, 100, 0), (1, 2 * N, 10, 4), (3000, 6 * N, 20, 6), (0, 0, 0, 12)], DESC)
    assert _extent(lib, 7, 1, d) == (0, [9000 + 4 * N, 102, 51, 1, 1])
    for bad_samples in (4 * N + 3, N, 0, 5 * N):   # partial symbol, below two symbols, odd data symbols
        bad = d.copy()
        bad["samples"][0] = bad_samples
        bad["unit_offset"][1:] = np.cumsum(bad["samples"][:3] // N)
        assert _extent(lib, 7, 1, bad)[0] == EINVAL, bad_samples
    bad = d.copy()
    bad["unit_offset"][2] = 5
    assert _extent(lib, 7, 1, bad)[0] == EINVAL
    bad = d.copy()
    bad["samples"][0] = 1 << 31
    assert _extent(lib, 7, 1, bad)[0] == ERANGE
    # osr 2: the unit is N * osr samples
    d2 = np.array([(0, 4 * N * 2, 0, 0), (0, 0, 2, 4)], DESC)
    assert _extent(lib, 7, 2, d2) == (0, [8 * N, 2, 1, 0, 0])
    assert _extent(lib, 7, 1, d2)[0] == EINVAL     # the prefix counts units of N * osr


def _plan(lib, *args):
    a = np.array(args, np.uint64)
    out = np.zeros(7 + 3 * lib.tx_max_slices(), np.uint64)
    k = lib.tx_plan_check(a.ctypes.data, out.ctypes.data)
    n, end, copied_end, ub, ue, db, de = (int(v) for v in out[:7])
    assert k == 7 + 3 * n
    slices = [tuple(int(v) for v in out[7 + 3 * i: 10 + 3 * i]) for i in range(n)]
    return dict(end=end, copied_end=copied_end, up=(ub, ue), down=(db, de), slices=slices)


def _a(x):
    return (max(1, x) + 255) & ~255


@pytest.mark.parametrize("iq_gaps,sym_gaps", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("shape", [(70, 5, 14 * 128, 140), (1, 1, 4 * 128, 2), (0, 2, 4 * 128, 0), (257, 3, 999, 0)])
def test_plan_slices_and_spans(lib, shape, iq_gaps, sym_gaps):
    nbytes, frames, iq, syms = shape
    p = _plan(lib, nbytes, frames, iq, syms, iq_gaps, sym_gaps)
    assert lib.tx_max_slices() >= 4
    want = [(nbytes, IN), ((frames + 1) * 32, IN), (iq * 8, INOUT if iq_gaps else OUT),
            (syms * 2, INOUT if sym_gaps else OUT)]
    off = 0
    for (o, size, role), (wsize, wrole) in zip(p["slices"], want):
        assert (o, size, role) == (off, wsize, wrole)     # distinct, ordered, 256-byte aligned
        off += _a(wsize)
    assert len(p["slices"]) == 4 and p["end"] == off == p["copied_end"]
    # the spans: from the first to the last non-empty slice that goes in / comes out
    ins = [(o, o + _a(s)) for o, s, r in p["slices"] if s and r & IN]
    outs = [(o, o + _a(s)) for o, s, r in p["slices"] if s and r & OUT]
    assert p["up"] == (ins[0][0], ins[-1][1])
    assert p["down"] == (outs[0][0], outs[-1][1])
    # without gaps nothing of the outputs is uploaded: the upload ends where the IQ begins
    if not iq_gaps and not (sym_gaps and syms):
        assert p["up"][1] == p["slices"][2][0]


@pytest.mark.parametrize("sf,osr,frames,nbytes", [(7, 1, 1, 0), (7, 1, 70, 33), (7, 2, 9, 16), (12, 1, 3, 3),
                                                  (9, 4, 5, 64)])
def test_reservation_covers_the_plan(lib, sf, osr, frames, nbytes):
    N = 1 << sf
    fs = (2 * nbytes + 2) * N * osr
    got = lib.tx_reserve_check(N, osr, frames, fs, 0)
    for gaps in (0, 1):
        assert got >= _plan(lib, frames * nbytes, frames, frames * fs, frames * 2 * nbytes, gaps, gaps)["end"]
