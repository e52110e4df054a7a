"""lphy_hip_estimate_ragged_host without a device: its staging plan
(csrc/lphy_stage_plan.h estimate_ragged_plan), the reservation that has to
cover it, and the check of the caller's table (csrc/lphy_ragged_layout.h
estimate_ragged_extent), compiled into a host-only test library
(tests/cpp/estimate_ragged_plan_check.cpp) as tests/test_stage_plan_cpu.py
does for the other plans; and the binding's argument checks."""
import ctypes as C
import errno
import itertools

import numpy as np
import pytest
import torch

import hostcc

IN, INOUT = 1, 3
META, DESC, IQ = 32, 32, 8


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = hostcc.shared_lib("estimate_ragged_plan_check.cpp", tmp_path_factory.mktemp("estimate_ragged_plan"))
    L.estimate_ragged_plan_check.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    L.estimate_ragged_reserve_check.argtypes = [C.c_uint64] * 5
    L.estimate_ragged_reserve_check.restype = C.c_uint64
    L.estimate_ragged_extent_check.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def _plan(lib, iq_samples, frames):
    out = np.zeros(7 + 3 * 5, np.uint64)
    k = lib.estimate_ragged_plan_check(iq_samples, frames, out.ctypes.data)
    assert k == 7 + 3 * int(out[0])
    n, end, copied_end, ub, ue, db, de = (int(v) for v in out[:7])
    slices = [tuple(int(v) for v in out[7 + 3 * i: 10 + 3 * i]) for i in range(n)]  # (off, size, role)
    return dict(end=end, copied_end=copied_end, up=(ub, ue), down=(db, de), slices=slices)


def _a(x):  # a slice's room: align_up(max(1, x))
    return (max(1, x) + 255) & ~255


# a zero-sized slice, a one-byte-past-alignment slice and ordinary calls
SHAPES = [(0, 1), (0, 3), (1, 1), (33, 8), (32, 8), (8 * 128 + 7, 3), (40 * 9000, 40), (66 * 4096 * 5, 5)]


@pytest.mark.parametrize("iq,frames", SHAPES)
def test_plan_slices(lib, iq, frames):
    """iq (in) | the frames' records (in) | meta (in and out): disjoint,
    aligned, back to back; everything goes up, the records' slice comes down."""
    p = _plan(lib, iq, frames)
    want = [(iq * IQ, IN), (frames * DESC, IN), (frames * META, INOUT)]
    off, prev_end = 0, 0
    for (o, size, role), (wsize, wrole) in zip(p["slices"], want):
        assert (o, size, role) == (off, wsize, wrole)
        assert o % 256 == 0 and o >= prev_end
        prev_end = o + max(size, 1)
        off += _a(wsize)
    assert len(p["slices"]) == 3 and p["end"] == off == p["copied_end"]
    meta_off = p["slices"][2][0]
    assert p["down"] == (meta_off, p["end"])
    assert p["up"] == ((0 if iq else p["slices"][1][0]), p["end"])


def _mod_scratch(N, osr, nsyms):
    """mod_scratch_bytes for one frame (lphy_hip.hip) at the smaller of k_mod_fast's LDS limits."""
    nph, step = nsyms + 2, N * osr
    form = 0 if nph >= 4096 or nph > 256 else (1 if nph * ((step + 4) * 4 + 64) <= 64 << 10 else 2)
    al = lambda x: (x + 255) & ~255
    return al(nph * 4) + (al(nph * step * 4) if nph < 4096 else 0) + ((al(2056) + al(256 * 64)) if form == 2 else 0)


@pytest.mark.parametrize("sf,osr,frames", list(itertools.product([7, 9, 12], [1, 4], [1, 3, 40])))
def test_reservation_covers_the_plan(lib, sf, osr, frames):
    """lphy_hip_ctx_reserve(frames, frame_samples): `frames` frames of up to
    frame_samples each, so an IQ extent of up to frames * frame_samples."""
    N = 1 << sf
    step = N * osr
    for fs in (0, 1, step - 1, step, 2 * step + 5, 66 * step + 3):
        got = lib.estimate_ragged_reserve_check(N, osr, frames, fs, _mod_scratch(N, osr, fs // step))
        assert got >= _plan(lib, frames * fs, frames)["end"], (fs,)


def _extent(lib, rows):
    desc = np.array(rows, np.uint64).reshape(-1, 4)
    out = np.zeros(1, np.uint64)
    rc = lib.estimate_ragged_extent_check(desc.ctypes.data, desc.shape[0], out.ctypes.data)
    return rc, int(out[0])


def test_table_check(lib):
    """The limits of lphy_hip_demod_ragged_host on the two fields the call
    reads; no prefix is required (unit_offset and sym_offset hold anything)."""
    junk = 0xDEADBEEF
    assert _extent(lib, [(5, 100, junk, junk), (300, 0, 1, 7), (120, 50, junk, 0)]) == (0, 300)
    assert _extent(lib, [(0, (1 << 31) - 1, 0, junk)]) == (0, (1 << 31) - 1)
    assert _extent(lib, [(0, 10, 0, 0), (0, 1 << 31, 0, 0)])[0] == -errno.ERANGE
    assert _extent(lib, [((1 << 48) + 1, 0, 0, 0)])[0] == -errno.ERANGE
    assert _extent(lib, [(1 << 48, 4, 0, 0)]) == (0, (1 << 48) + 4)
    assert _extent(lib, [(7, 7, 0, 0)] * 0) == (0, 0)


def test_binding_refuses_host_buffers(lphy):
    """Demodulator.estimate_ragged checks its tensors (lphy._dev_buf) before
    the library is called: no context is needed to see that."""
    class Ctx:  # the attributes estimate_ragged reads before its first library call
        device, ctx, lib = 0, None, None
    iq, desc, meta = torch.zeros(64), torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="cpu"):
        lphy.Demodulator.estimate_ragged(Ctx(), iq, desc, 2, 0, meta, iq_samples=8)
    with pytest.raises(ValueError, match="device tensor"):
        lphy.Demodulator.estimate_ragged(Ctx(), np.zeros(64, np.float32), desc, 2, 0, meta, iq_samples=8)
    with pytest.raises(ValueError, match="device tensor"):
        lphy.Demodulator.estimate_ragged(Ctx(), None, desc, 2, 0, meta)
    assert "lphy_hip_estimate_ragged" in lphy.EXPORTS and "lphy_hip_estimate_ragged_host" in lphy.EXPORTS
