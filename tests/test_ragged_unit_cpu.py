"""csrc/lphy_ragged_unit.h without a device: ragged_unit<false>, the one
resolver of "unit u of a ragged table" that k_rg_demod, the ragged detector
and k_tx_samples call, compiled into a host-only test library
(tests/cpp/ragged_unit_check.cpp) and compared, for every u in [0, units + 2),
with a linear scan written here: the last record whose unit_offset is <= u.
For forged tables the property the kernels rely on: a live unit's record has
unit_offset <= u and its frame is below `frames`; a unit past the table's
total is not live and read record 0."""
import ctypes as C
import itertools

import numpy as np
import pytest

import hostcc

STEP = 128  # N = 128, osr = 1
IQ, SAMPLES, SYM, UNIT = range(4)  # lphy_ragged_desc's fields


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = hostcc.shared_lib("ragged_unit_check.cpp", tmp_path_factory.mktemp("ragged_unit"))
    L.ru_layout_check.argtypes = [C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p]
    L.ru_units_check.argtypes = [C.c_void_p, C.c_uint, C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p]
    L.ru_units_check.restype = None
    return L


def _layout(lib, symbols):
    """ragged_layout's table for frames of `symbols` whole symbols (and a partial one)."""
    samples = np.array([n * STEP + (f % 3) for f, n in enumerate(symbols)], np.uint64)
    desc = np.zeros((len(symbols) + 1, 4), np.uint64)
    assert lib.ru_layout_check(STEP, samples.ctypes.data, len(symbols), desc.ctypes.data) == 0
    assert int(desc[-1, UNIT]) == sum(symbols)
    return desc


def _resolve(lib, desc):
    """(frame, s, live, read) of every u in [0, units + 2); units is record [frames]'s."""
    frames, units = desc.shape[0] - 1, int(desc[-1, UNIT])
    out = np.zeros((units + 2, 4), np.uint64)
    lib.ru_units_check(desc.ctypes.data, frames, units, 0, units + 2, out.ctypes.data)
    return out[:, 0].astype(np.int64), out[:, 1], out[:, 2].astype(bool), out[:, 3].astype(bool)


def _scan(desc, u):
    """The last record of the frames' whose unit_offset is <= u."""
    want = 0
    for f in range(desc.shape[0] - 1):
        if int(desc[f, UNIT]) <= u:
            want = f
    return want


# one frame of 0, 1 and 5 symbols; 2 and 3 frames with every placement of a
# zero-symbol frame (first, middle, last, all); [0, 0, 0, 1, 2, 3, 4, 5] to 601 frames
ZEROS = [[0 if z else n for z, n in zip(zs, (2, 3, 4))] for k in (2, 3) for zs in itertools.product((0, 1), repeat=k)]
TABLES = [[0], [1], [5]] + ZEROS + [([0, 0, 0, 1, 2, 3, 4, 5] * 76)[:601]]


@pytest.mark.parametrize("symbols", TABLES, ids=lambda s: f"{len(s)}f-" + "".join(map(str, s[:8])))
def test_sound_tables_equal_the_linear_scan(lib, symbols):
    desc = _layout(lib, symbols)
    units = sum(symbols)
    frame, s, live, read = _resolve(lib, desc)
    assert read.all()
    for u in range(units + 2):
        if u < units:
            want = _scan(desc, u)
            assert (frame[u], int(s[u]), live[u]) == (want, u - int(desc[want, UNIT]), True), u
            assert int(s[u]) < symbols[want]  # inside the frame's own count
        else:
            assert not live[u] and frame[u] == 0, u


def _forged(lib):
    base = _layout(lib, [3, 0, 2, 4, 1])
    a = base.copy()
    a[2, UNIT] = base[-1, UNIT] + 7    # a non-monotone unit_offset
    b = base.copy()
    b[1, UNIT], b[3, UNIT] = 6, 1      # ... and one that goes down again
    c = base.copy()
    c[0, UNIT] = 3                     # a first record with unit_offset > 0
    d = base.copy()
    d[-1, UNIT] = base[-1, UNIT] + 9   # a total larger than the true sum
    many = _layout(lib, ([0, 0, 0, 1, 2, 3, 4, 5] * 76)[:601])
    e = many.copy()
    e[300, UNIT] = 0
    e[-1, UNIT] += 5
    return dict(up=a, down=b, first=c, total=d, many=e)


@pytest.mark.parametrize("which", ["up", "down", "first", "total", "many"])
def test_forged_tables_stay_inside(lib, which):
    desc = _forged(lib)[which]
    frames, units = desc.shape[0] - 1, int(desc[-1, UNIT])
    frame, s, live, read = _resolve(lib, desc)
    assert read.all() and (frame >= 0).all() and (frame < frames).all()
    for u in range(units + 2):
        if live[u]:
            assert u < units and int(desc[frame[u], UNIT]) <= u and int(s[u]) == u - int(desc[frame[u], UNIT]), u
        if u >= units:
            assert not live[u] and frame[u] == 0, u
    if which == "first":  # the units below the first record's offset belong to no frame
        assert not live[:3].any() and live[3:units].all()


def test_resolver_under_the_host_sanitizers(tmp_path):
    """The same source as a stand-alone program (-DRAGGED_UNIT_MAIN) under
    ASan + UBSan, on heap tables of exactly frames + 1 records."""
    out = hostcc.run_check("ragged_unit_check.cpp", tmp_path, define="RAGGED_UNIT_MAIN")
    assert out.strip() == "ragged_unit_check: ok", out
