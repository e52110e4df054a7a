"""lphy_hip_ragged_layout without a device.  The product library's entry
point needs a context, and a context needs a HIP device, so the function's
own translation unit (csrc/lphy_ragged_layout.h, which lphy_hip.hip calls with
the context's N * osr) is compiled into a host-only test library
(tests/cpp/ragged_layout_check.cpp) and called through ctypes:

* the prefix sums of modes 0, 1 and 2 over frames of 0, 1, 2 and more whole
  symbols, with and without a trailing partial symbol;
* every sym_offset even (frame f's bytes start at sym_offset / 2);
* the sentinel record [frames] with the totals and samples = 0;
* -ERANGE at samples = 2^31 and at 2^32 whole symbols, -EINVAL for a bad
  mode or a null pointer;
* the extent check of a caller's table (the host form's)."""
import ctypes as C

import numpy as np
import pytest

import hostcc

DESC = np.dtype([("iq_offset", "<u8"), ("samples", "<u8"), ("sym_offset", "<u8"), ("unit_offset", "<u8")])


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = hostcc.shared_lib("ragged_layout_check.cpp", tmp_path_factory.mktemp("ragged_layout"))
    L.ragged_layout_check.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ragged_extent_check.argtypes = [C.c_uint, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.ragged_desc_size.restype = C.c_size_t
    return L


def _layout(lib, sf, lengths, mode, osr=1):
    n = np.ascontiguousarray(lengths, np.uint64)
    desc = np.full(n.size + 1, 0xAB, np.uint8).repeat(32).view(DESC)
    rc = lib.ragged_layout_check(sf, osr, n.ctypes.data if n.size else None, n.size, mode, desc.ctypes.data)
    return rc, desc


def _expected(sf, lengths, mode, osr=1):
    step = (1 << sf) * osr
    rows, iq, sym, unit = [], 0, 0, 0
    for n in lengths:
        total = n // step
        per = (total - 2 if total >= 2 else 0) if mode == 0 else (total - 2 if total >= 2 else total)
        rows.append((iq, n, sym, unit))
        iq += n
        sym += per + (per & 1)
        unit += total
    rows.append((iq, 0, sym, unit))
    return np.array(rows, DESC)


def test_descriptor_is_32_bytes(lib):
    assert lib.ragged_desc_size() == 32 == DESC.itemsize


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("sf", [7, 12])
def test_prefix_sums(lib, sf, mode):
    N = 1 << sf
    lengths = [0, N, 2 * N, 3 * N, 4 * N, 5 * N, 10 * N, 34 * N, 66 * N, 2 * N, 66 * N, 3 * N,
               37, N + 37, 2 * N + 37, 7 * N + N - 1]
    rc, desc = _layout(lib, sf, lengths, mode)
    assert rc == 0
    np.testing.assert_array_equal(desc, _expected(sf, lengths, mode))
    assert not np.any(desc["sym_offset"] & 1)
    # frames of 0 / 1 / 2 whole symbols: 0 / 1 / 0 output symbols in modes 1, 2; none in mode 0
    step = np.diff(desc["sym_offset"].astype(np.int64))[:3]
    assert list(step) == ([0, 0, 0] if mode == 0 else [0, 2, 0])
    # the sentinel record
    last = desc[-1]
    assert last["samples"] == 0
    assert last["iq_offset"] == sum(lengths)
    assert last["unit_offset"] == sum(n // N for n in lengths)


def test_oversampled_step(lib):
    rc, desc = _layout(lib, 7, [128 * 4 * 5, 128 * 4 * 3 + 1], 1, osr=4)
    assert rc == 0
    np.testing.assert_array_equal(desc, _expected(7, [128 * 4 * 5, 128 * 4 * 3 + 1], 1, osr=4))
    assert list(desc["unit_offset"]) == [0, 5, 8]


def test_no_frames(lib):
    rc, desc = _layout(lib, 8, [], 2)
    assert rc == 0
    assert desc[0].tolist() == (0, 0, 0, 0)


def test_limits_and_arguments(lib):
    N = 128
    assert _layout(lib, 7, [4 * N, (1 << 31) - 1], 1)[0] == 0
    assert _layout(lib, 7, [4 * N, 1 << 31], 1)[0] == -34          # -ERANGE: samples = 2^31
    assert _layout(lib, 7, [4 * N, 1 << 40], 0)[0] == -34
    # 2^32 whole symbols in the call: 2^10 frames of 2^22 symbols (SF 7: 2^29 samples)
    big = [1 << 29] * (1 << 10)
    assert _layout(lib, 7, big, 1)[0] == -34
    assert _layout(lib, 7, big[:-1], 1)[0] == 0
    assert _layout(lib, 7, [N], 3)[0] == -22                       # -EINVAL: mode
    assert _layout(lib, 7, [N], -1)[0] == -22
    n = np.array([N], np.uint64)
    assert lib.ragged_layout_check(7, 1, n.ctypes.data, 1, 1, None) == -22
    d = np.zeros(2, DESC)
    assert lib.ragged_layout_check(7, 1, None, 1, 1, d.ctypes.data) == -22


def test_extent_of_a_callers_table(lib):
    N = 128
    # gaps in the IQ and in the outputs, frames out of address order
    d = np.array([(5000, 4 * N, 100, 0), (0, 3 * N + 37, 10, 4), (9000, N, 0, 7), (0, 0, 0, 8)], DESC)
    iq, out = C.c_uint64(), C.c_uint64()
    assert lib.ragged_extent_check(7, d.ctypes.data, 3, 1, C.byref(iq), C.byref(out)) == 0
    assert (iq.value, out.value) == (9000 + N, 102)
    assert lib.ragged_extent_check(7, d.ctypes.data, 3, 0, C.byref(iq), C.byref(out)) == 0
    assert out.value == 102
    bad = d.copy()
    bad["unit_offset"][1] = 5                                      # not the prefix of whole symbols
    assert lib.ragged_extent_check(7, bad.ctypes.data, 3, 1, C.byref(iq), C.byref(out)) == -22
    bad = d.copy()
    bad["samples"][0] = 1 << 31
    assert lib.ragged_extent_check(7, bad.ctypes.data, 3, 1, C.byref(iq), C.byref(out)) == -34
