"""The staging plans of the *_host entry points without a device.
csrc/lphy_stage_plan.h (which csrc/lphy_host.h builds every host call on, and
lphy_hip_ctx_reserve sizes the staging from) is compiled into a host-only
test library (tests/cpp/stage_plan_check.cpp) and called through ctypes:

* the slice offsets of each of the eight plans equal the layout formulas the
  entry points computed by hand before they shared the plan, restated below
  (a slice of 0 bytes occupies one 256-byte unit: the old `max(1, ...)`, now
  for every slice - the old demod layout gave its IQ and record slices no
  unit at 0 frames, where nothing is copied or launched);
* slices disjoint and aligned, copied_end <= end, scratch last;
* the upload / download spans of the three calls that go through the pinned
  mirror equal the single copies those calls made;
* the reservation covers every plan at the reserved shape and never falls
  below the old formula."""
import ctypes as C
import itertools

import numpy as np
import pytest

import hostcc

IN, OUT, INOUT, ZERO_OUT, SCRATCH = 1, 2, 3, 6, 8
DEMOD, RAGGED, DETECT, DECODE, ESTIMATE, COMPENSATE, COMPENSATE_BATCH, MODULATE = range(8)
META, DESC, REC, SPEC, IQ = 32, 32, 16, 16, 8


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = hostcc.shared_lib("stage_plan_check.cpp", tmp_path_factory.mktemp("stage_plan"))
    L.stage_plan_check.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.stage_reserve_check.argtypes = [C.c_uint64] * 5
    L.stage_reserve_check.restype = C.c_uint64
    return L


def _plan(lib, which, *args):
    a = np.array(list(args) + [0, 0, 0], np.uint64)
    out = np.zeros(7 + 3 * lib.stage_max_slices(), np.uint64)
    k = lib.stage_plan_check(which, a.ctypes.data, out.ctypes.data)
    assert k >= 7 and k == 7 + 3 * int(out[0])
    n, end, copied_end, ub, ue, db, de = (int(v) for v in out[:7])
    slices = [tuple(int(v) for v in out[7 + 3 * i: 10 + 3 * i]) for i in range(n)]  # (off, size, role)
    return dict(end=end, copied_end=copied_end, up=(ub, ue), down=(db, de), slices=slices)


def _a(x):  # a slice's room: align_up(max(1, x))
    return (max(1, x) + 255) & ~255


def _offsets(sizes):
    """Back-to-back offsets of slices of `sizes` bytes, and their end."""
    off, o = [], 0
    for s in sizes:
        off.append(o)
        o += _a(s)
    return off, o


def _sizes(which, *a):
    """(size, role) per slice as the entry points laid them out by hand."""
    if which == DEMOD:  # demod_layout: iq | syms | bytes | meta | spec
        frames, fs, per = a
        return [(frames * fs * IQ, IN), (frames * per * 2, OUT), (frames * (per // 2), OUT),
                (frames * META, ZERO_OUT), (frames * SPEC, SCRATCH)]
    if which == RAGGED:  # o_desc, o_syms, o_bytes, o_meta
        iq, frames, syms = a
        return [(iq * IQ, IN), ((frames + 1) * DESC, IN), (syms * 2, INOUT), ((syms + 1) // 2, INOUT),
                (frames * META, ZERO_OUT)]
    if which == DETECT:  # o_out
        span, windows = a
        return [(span * IQ, IN), (windows * REC, OUT)]
    if which == DECODE:  # sym_b, byte_b, meta_b
        return [(a[0] * 2, IN), (a[0] // 2, OUT), (META, ZERO_OUT)]
    if which == ESTIMATE:  # iq_b, meta_b
        return [(a[0] * IQ, IN), (META, INOUT)]
    if which == COMPENSATE:  # 2 * iq_b
        return [(a[0] * IQ, INOUT), (a[0] * IQ, SCRATCH)]
    if which == COMPENSATE_BATCH:  # o_meta
        return [(a[0] * a[1] * IQ, INOUT), (a[0] * META, IN)]
    step, nsyms, scratch = a  # sym_b, iq_b, mod_scratch_bytes
    return [(nsyms * 2, IN), ((nsyms + 2) * step * IQ, OUT), (scratch, SCRATCH)]


# a zero-sized slice, a one-byte slice, one byte past an alignment boundary, and an ordinary call
CASES = [
    (DEMOD, 3, 4 * 128, 2), (DEMOD, 0, 512, 2), (DEMOD, 3, 128, 0), (DEMOD, 1, 512, 2), (DEMOD, 1, 66 * 128, 514),
    (DEMOD, 2, 6 * 2048, 4),
    (RAGGED, 0, 3, 0), (RAGGED, 8 * 128 + 7, 3, 2), (RAGGED, 33, 8, 513), (RAGGED, 1, 1, 1),
    (DETECT, 128, 1), (DETECT, 128 + 2 * 64, 3), (DETECT, 33, 17),
    (DECODE, 0), (DECODE, 2), (DECODE, 8), (DECODE, 514), (DECODE, 130),
    (ESTIMATE, 0), (ESTIMATE, 1), (ESTIMATE, 33), (ESTIMATE, 256),
    (COMPENSATE, 1), (COMPENSATE, 32), (COMPENSATE, 33), (COMPENSATE, 256),
    (COMPENSATE_BATCH, 1, 1), (COMPENSATE_BATCH, 3, 512), (COMPENSATE_BATCH, 9, 33),
    (MODULATE, 128, 0, 2304), (MODULATE, 128, 2, 0), (MODULATE, 128, 129, 1), (MODULATE, 4 * 4096, 66, 257),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_offsets_equal_the_hand_computed_layouts(lib, case):
    p = _plan(lib, *case)
    want = _sizes(*case)
    off, end = _offsets([s for s, _ in want])
    assert [(o, s, r) for o, (s, r) in zip(off, want)] == p["slices"]
    assert p["end"] == end


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_slices_are_disjoint_aligned_and_scratch_is_last(lib, case):
    p = _plan(lib, *case)
    prev_end, seen_scratch, copied = 0, False, 0
    for off, size, role in p["slices"]:
        assert off % 256 == 0 and off >= prev_end and (off > 0 or prev_end == 0)
        prev_end = off + max(size, 1)
        assert not (seen_scratch and role != SCRATCH)
        seen_scratch |= role == SCRATCH
        if role != SCRATCH:
            copied = off + _a(size)
    assert prev_end <= p["end"]
    assert p["copied_end"] == copied <= p["end"]
    for b, e in (p["up"], p["down"]):
        assert b % 256 == 0 and e % 256 == 0 and b <= e <= p["copied_end"]


def test_spans_equal_the_mirrored_copies(lib):
    # demod: H2D [0, L.spec), D2H [L.syms, L.spec)
    p = _plan(lib, DEMOD, 3, 512, 2)
    (syms, _, _), (spec, _, _) = p["slices"][1], p["slices"][4]
    assert p["up"] == (0, spec) and p["down"] == (syms, spec) and p["copied_end"] == spec
    # decode: H2D [0, end), D2H [sym_b, end)
    p = _plan(lib, DECODE, 8)
    assert p["up"] == (0, p["end"]) and p["down"] == (p["slices"][1][0], p["end"]) and p["copied_end"] == p["end"]
    # modulate: the symbols in (rounded up to the slice), the samples out; the mirror holds sym_b + iq_b
    p = _plan(lib, MODULATE, 128, 2, 2304)
    iq, scratch = p["slices"][1][0], p["slices"][2][0]
    assert p["up"] == (0, iq) and p["down"] == (iq, scratch) and p["copied_end"] == scratch
    assert iq == _a(2 * 2) and scratch - iq == 4 * 128 * IQ
    # nothing to move: no copy at all (modulate of 0 symbols uploads nothing; decode of 0 symbols has no bytes)
    assert _plan(lib, MODULATE, 128, 0, 2304)["up"] == (0, 0)
    p = _plan(lib, DECODE, 0)
    assert p["down"] == (p["slices"][2][0], p["end"])
    # slice-by-slice calls: in / inout / zero up, out / inout down
    p = _plan(lib, RAGGED, 1024, 3, 6)
    assert p["up"] == (0, p["end"]) and p["down"] == (p["slices"][2][0], p["end"])


def _mod_scratch(N, osr, nsyms, lds_limit):
    """mod_scratch_bytes for one frame (lphy_hip.hip), with k_mod_fast's LDS limit of the device."""
    nph, step = nsyms + 2, N * osr
    form = 0 if nph >= 4096 or nph > 256 else (1 if nph * ((step + 4) * 4 + 64) <= lds_limit else 2)
    al = lambda x: (x + 255) & ~255
    return al(nph * 4) + (al(nph * step * 4) if nph < 4096 else 0) + ((al(2056) + al(256 * 64)) if form == 2 else 0)


def _old_reserve(N, osr, frames, fs, scratch):
    """host_stage_bytes before it was derived from the plans."""
    al = lambda x: (x + 255) & ~255
    step, n = N * osr, frames * fs
    syms = fs // step + 2

    def demod_end(mode):
        total = fs // step
        per = (total - 2 if total >= 2 else 0) if mode == 0 else (total - 2 if total >= 2 else total)
        return (al(n * IQ) + al(max(1, frames * per) * 2) + al(max(1, frames * (per // 2))) + al(frames * META)
                + al(frames * SPEC))
    return max(demod_end(2), demod_end(0), 2 * al(n * IQ), al(syms * 2) + al(n * IQ) + scratch,
               3 * al(max(1, frames * syms) * 2))


def _reserved_plans(lib, N, osr, frames, fs, scratch):
    """Every entry point's plan at the shape lphy_hip_ctx_reserve(frames, fs) is for."""
    step, n, total = N * osr, frames * fs, fs // (N * osr)
    per = total - 2 if total >= 2 else total
    plans = [_plan(lib, DEMOD, frames, fs, per), _plan(lib, DEMOD, frames, fs, max(total, 2) - 2),
             _plan(lib, RAGGED, n, frames, frames * (per + (per & 1))), _plan(lib, DETECT, n, n // N),
             _plan(lib, DECODE, frames * (total + 2)), _plan(lib, ESTIMATE, n), _plan(lib, COMPENSATE, n),
             _plan(lib, COMPENSATE_BATCH, frames, fs), _plan(lib, MODULATE, step, total, scratch)]
    return max(p["end"] for p in plans)


@pytest.mark.parametrize("sf,osr,frames,nsyms", list(itertools.product([7, 12], [1, 4], [1, 3], [2, 66])))
@pytest.mark.parametrize("lds_limit", [64 << 10, 144 << 10])
def test_reservation_covers_every_plan_and_never_shrinks(lib, sf, osr, frames, nsyms, lds_limit):
    N = 1 << sf
    fs = nsyms * N * osr
    scratch = _mod_scratch(N, osr, fs // (N * osr), lds_limit)
    got = lib.stage_reserve_check(N, osr, frames, fs, scratch)
    assert got == _reserved_plans(lib, N, osr, frames, fs, scratch)
    assert got >= _old_reserve(N, osr, frames, fs, scratch)


def test_reservation_never_shrinks_on_odd_shapes(lib):
    """The same over every SF, frames shorter than a symbol, a trailing
    partial symbol, and many frames (the old modulate term counted the whole
    buffer's samples; the plans count one frame's symbols, and the
    compensation's two buffers cover the rest)."""
    for sf, osr, frames in itertools.product(range(1, 13), [1, 4], [1, 2, 5, 64]):
        N = 1 << sf
        step = N * osr
        for fs in (0, 1, step - 1, step, 2 * step + 1, 4 * step, 66 * step + 3, 300 * step):
            for lds_limit in (64 << 10, 144 << 10):
                scratch = _mod_scratch(N, osr, fs // step, lds_limit)
                got = lib.stage_reserve_check(N, osr, frames, fs, scratch)
                assert got >= _old_reserve(N, osr, frames, fs, scratch), (sf, osr, frames, fs, lds_limit)
