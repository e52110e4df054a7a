"""lphy_hip_compensate_batch / _ragged / _batch_host (compensate_offsets,
phy.cpp:150-180, for every frame of a batch with the frame's own offsets read
on the device) against the oracle's restatement applied frame by frame, which
test_oracle_vs_reference.py::test_compensate_offsets_bit_exact pins to the
reference build.  Bit for bit, NaN results as NaN.

k_comp_batch (csrc/lphy_mod.h) works in tiles of 1024 samples cut where the
destination is 16-byte aligned; out of place every tile is independent, in
place one workgroup walks a frame's tiles in memmove order.  Frames of an odd
length put every other frame half a 16-byte pair off, and the buffers here
are also started one sample (8 bytes) into a 16-byte line.

Every device buffer has guard samples in front and behind, and the out-of-
place destination is filled with the same sentinel, so a sample left
unwritten, or one written outside a frame, shows."""
import errno

import numpy as np
import pytest
import torch

from test_oracle_vs_reference import COMP_CASES, _nan_bits_equal

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5  # as float32: -2.9e-16, no value a test expects
GUARD = 4          # samples (32 bytes: keeps the 16-byte phase of what follows)
TILE = 1024        # kCompTile

PAIRS = [(c[2], c[3]) for c in COMP_CASES] + [(0.0, 0.0), (0.3, 0.49), (0.3, -0.49)]


def _iq(rng, shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 2.0).astype(np.complex64)


def _buffer(payload, skew, dev, fill_payload=True):
    """Device float32 tensor: GUARD + skew sentinel samples, the payload (or
    sentinels of its size), GUARD sentinel samples.  Returns (whole, view of
    the payload's place)."""
    n = payload.size
    a = 2 * (GUARD + skew)
    host = np.full(a + 2 * n + 2 * GUARD, SENT, np.uint32)
    if fill_payload:
        host[a: a + 2 * n] = np.ascontiguousarray(payload).reshape(-1).view(np.uint32)
    whole = torch.from_numpy(host.view(np.float32)).to(dev)
    return whole, whole[a: a + 2 * n]


def _read(whole, n, skew):
    """The payload's float32 values after checking the guards."""
    got = whole.cpu().numpy().view(np.uint32)
    a = 2 * (GUARD + skew)
    assert (got[:a] == SENT).all(), "written in front of the buffer"
    assert (got[a + 2 * n:] == SENT).all(), "written behind the buffer"
    return got[a: a + 2 * n].view(np.float32)


def _meta(lphy, pairs):
    """Records with cfo and time_offset set; the fields the call must not use
    (rate is -2 pi cfo / N without osr, t_off may be unset) hold other values."""
    m = np.zeros(len(pairs), lphy.META_DTYPE)
    m["cfo"] = [p[0] for p in pairs]
    m["time_offset"] = [p[1] for p in pairs]
    m["rate"], m["t_off"], m["scale"], m["status"] = 123.0, 77, -3.0, -5
    return m


def _meta_dev(m, dev):
    return torch.from_numpy(m.view(np.uint8).copy()).to(dev)


def _want(oracle, x, sf, osr, pairs):
    return [oracle.compensate_offsets(x[f], sf, float(pairs[f][0]), float(pairs[f][1]), osr)
            for f in range(len(pairs))]


def _run_uniform(lphy, d, x, pairs, in_place, in_skew=0, out_skew=0, stream=None):
    """compensate_batch on the frames of x ([frames, fs]); returns the output
    as float32 [frames * fs * 2]."""
    frames, fs = x.shape
    dev = torch.device("cuda", d.device)
    m = _meta(lphy, pairs)
    t_meta = _meta_dev(m, dev)
    w_in, v_in = _buffer(x, in_skew, dev)
    if in_place:
        w_out, v_out, out_skew = w_in, v_in, in_skew
    else:
        w_out, v_out = _buffer(x, out_skew, dev, fill_payload=False)
    torch.cuda.synchronize()
    d.compensate_batch(v_in, v_out, frames, fs, t_meta, stream=stream)
    torch.cuda.synchronize()
    assert (t_meta.cpu().numpy() == m.view(np.uint8)).all(), "d_meta written"
    if not in_place:  # the source is read only
        np.testing.assert_array_equal(_read(w_in, x.size, in_skew).view(np.uint32),
                                      np.ascontiguousarray(x).reshape(-1).view(np.uint32))
    return _read(w_out, x.size, out_skew)


def _check_frames(got, want, fs):
    for f, w in enumerate(want):
        try:
            _nan_bits_equal(got[2 * f * fs: 2 * (f + 1) * fs], w.view(np.float32))
        except AssertionError as e:
            raise AssertionError(f"frame {f}: {e}") from None


_UNIFORM = {}


def _uniform_case(oracle, sf, osr, frames, fs):
    """The shape's batches (frames, per-frame offsets, expectation), PAIRS in
    chunks of `frames` (the last one wraps); computed once per shape."""
    key = (sf, osr, frames, fs)
    if key not in _UNIFORM:
        rng = np.random.default_rng(1000 * sf + fs)
        batches = []
        for i in range(0, len(PAIRS), frames):
            pairs = [PAIRS[(i + j) % len(PAIRS)] for j in range(frames)]
            x = _iq(rng, (frames, fs))
            x[0, 3] = complex(np.inf, 0.5)  # the Annex G product inside the rotation
            x[1, fs // 2] = complex(np.nan, 1.0)
            want = _want(oracle, x, sf, osr, pairs)
            x.setflags(write=False)
            batches.append((x, pairs, want))
        _UNIFORM[key] = batches
    return _UNIFORM[key]


UNIFORM = [(7, 1, 6, 389), (9, 2, 3, 4101)]  # 389: no multiple of N, of a wave or of 4


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("sf,osr,frames,fs", UNIFORM)
def test_compensate_batch_uniform(oracle, lphy, sf, osr, frames, fs, in_place):
    d = lphy.Demodulator(sf, osr=osr)
    skews = [(0, 0), (1, 1)] if in_place else [(0, 0), (1, 0), (0, 1)]
    for x, pairs, want in _uniform_case(oracle, sf, osr, frames, fs):
        for in_skew, out_skew in skews:
            got = _run_uniform(lphy, d, x, pairs, in_place, in_skew, out_skew)
            _check_frames(got, want, fs)


EDGE_K = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4100, 4101, 4102]
assert TILE in EDGE_K and TILE - 1 in EDGE_K and TILE + 1 in EDGE_K
_EDGES = {}


def _edge_case(oracle):
    if not _EDGES:
        sf, fs = 9, 4101
        pairs = [(0.3, float(s * k)) for k in EDGE_K for s in (1, -1)]
        x = _iq(np.random.default_rng(77), (len(pairs), fs))
        want = _want(oracle, x, sf, 1, pairs)
        x.setflags(write=False)
        _EDGES["case"] = (sf, fs, x, pairs, want)
    return _EDGES["case"]


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_compensate_batch_shift_edges(oracle, lphy, in_place):
    """+-k around the wave, workgroup and tile sizes and around the frame
    length (4100 shifts all but one sample out, 4101 and 4102 do not shift),
    all in one call: where the in-place tile walk could go wrong."""
    sf, fs, x, pairs, want = _edge_case(oracle)
    got = _run_uniform(lphy, lphy.Demodulator(sf), x, pairs, in_place)
    _check_frames(got, want, fs)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_compensate_batch_no_shift_conversions(oracle, lphy, in_place):
    """time_offset values whose (int)round() is INT_MIN or at least the frame
    length: rotation only.  cfo = NaN and 3e7: sincosf's large-argument path."""
    sf, fs = 7, 389
    nan, inf = float("nan"), float("inf")
    pairs = [(0.3, nan), (0.3, inf), (0.3, -inf), (0.3, 1e9), (0.3, -2.6e9), (0.3, 2147483648.0),
             (nan, 5.0), (3e7, 5.0), (3e7, -2147483904.0)]
    x = _iq(np.random.default_rng(5), (len(pairs), fs))
    want = _want(oracle, x, sf, 1, pairs)
    for f in range(6):  # the oracle's own answer for these is the rotation alone
        _nan_bits_equal(want[f].view(np.float32),
                        oracle.compensate_offsets(x[f], sf, 0.3, 0.0, 1).view(np.float32))
    got = _run_uniform(lphy, lphy.Demodulator(sf), x, pairs, in_place)
    _check_frames(got, want, fs)


RAGGED_LEN = [0, 1, 255, 256, 700, 0, 2049]
RAGGED_PAIRS = [(0.37, 3.0), (0.2, 0.6), (-0.21, -17.3), (0.45, 255.0), (0.37, 95.54), (0.1, -2.0),
                (0.05, -1030.2)]
RAGGED_ORDER = [6, 2, 4, 1, 3, 0, 5]  # the frames' order in memory
RAGGED_GAPS = [3, 1, 2, 5, 1, 4, 2]   # samples left free after each of them


def _ragged_desc(lphy):
    desc = np.zeros(len(RAGGED_LEN), lphy.RAGGED_DESC_DTYPE)  # (no record [frames]: it is not read)
    pos = 5
    for f, gap in zip(RAGGED_ORDER, RAGGED_GAPS):
        desc["iq_offset"][f] = pos
        pos += RAGGED_LEN[f] + gap
    desc["samples"] = RAGGED_LEN
    desc["sym_offset"], desc["unit_offset"] = 0xDEADBEEF, 0xFEEDFACE  # not read
    return desc, pos


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_compensate_ragged(oracle, lphy, in_place):
    """Frames of 0 .. 2049 samples in non-monotonic address order with gaps:
    each frame as the oracle gives it alone, gaps and zero-length frames
    untouched in the destination."""
    sf = 8
    d = lphy.Demodulator(sf)
    dev = torch.device("cuda", d.device)
    desc, extent = _ragged_desc(lphy)
    rng = np.random.default_rng(88)
    frames = [_iq(rng, n) for n in RAGGED_LEN]
    want = [oracle.compensate_offsets(x, sf, cfo, toff, 1) if x.size else x
            for x, (cfo, toff) in zip(frames, RAGGED_PAIRS)]
    owned = np.zeros(extent, bool)
    src = _iq(rng, extent)  # the gaps of the source hold samples no frame owns
    for f, x in enumerate(frames):
        o = int(desc["iq_offset"][f])
        assert not owned[o: o + x.size].any()
        owned[o: o + x.size] = True
        src[o: o + x.size] = x
    if in_place:
        src.view(np.uint32).reshape(-1, 2)[~owned] = SENT
    m = _meta(lphy, RAGGED_PAIRS)
    t_meta = _meta_dev(m, dev)
    t_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    w_in, v_in = _buffer(src, 0, dev)
    w_out, v_out = (w_in, v_in) if in_place else _buffer(src, 0, dev, fill_payload=False)
    torch.cuda.synchronize()
    d.compensate_ragged(v_in, v_out, t_desc, len(RAGGED_LEN), t_meta, iq_samples=extent,
                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (t_meta.cpu().numpy() == m.view(np.uint8)).all(), "d_meta written"
    assert (t_desc.cpu().numpy() == desc.view(np.uint8)).all(), "d_desc written"
    got = _read(w_out, extent, 0)
    assert (got.view(np.uint32).reshape(-1, 2)[~owned] == SENT).all(), "a gap sample was written"
    for f, w in enumerate(want):
        o = int(desc["iq_offset"][f])
        try:
            _nan_bits_equal(got[2 * o: 2 * (o + w.size)], w.view(np.float32))
        except AssertionError as e:
            raise AssertionError(f"frame {f}: {e}") from None


def test_estimate_then_compensate_on_one_stream(oracle, lphy):
    """The chain the batch form exists for: estimate_batch leaves cfo and
    time_offset in d_meta, compensate_batch reads them there, both queued on
    one non-default stream with no synchronisation and no host copy between."""
    sf, frames, nsyms = 7, 4, 10
    N = 1 << sf
    fs = (nsyms + 2) * N
    d = lphy.Demodulator(sf)
    dev = torch.device("cuda", d.device)
    rng = np.random.default_rng(31)
    syms = rng.integers(0, N, (frames, nsyms)).astype(np.uint16)
    t_syms = torch.from_numpy(syms.view(np.int16).reshape(-1).copy()).to(dev)
    t_mod = torch.zeros(frames * fs * 2, dtype=torch.float32, device=dev)
    d.modulate_batch(t_syms, frames, nsyms, t_mod, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x = t_mod.cpu().numpy().view(np.complex64).reshape(frames, fs).copy()
    n = np.arange(fs)
    for f in range(frames):  # a time offset of f samples and a small CFO of its own
        cfo = 0.02 * (f + 1)
        x[f] = (np.roll(x[f], f) * np.exp(2j * np.pi * cfo * n / N)).astype(np.complex64)
    want = [oracle.compensate_offsets(x[f], sf, *(float(v) for v in oracle.estimate_offsets(x[f][:2 * N], sf)))
            for f in range(frames)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t_iq = torch.from_numpy(x.view(np.float32).reshape(-1).copy()).to(dev)
        t_meta = torch.full((frames * 32,), 0xA5, dtype=torch.uint8, device=dev)
        d.estimate_batch(t_iq, frames, fs, 2 * N, t_meta, stream=s.cuda_stream)
        before = t_meta.clone()  # (a device copy in stream order: not a synchronisation)
        d.compensate_batch(t_iq, t_iq, frames, fs, t_meta, stream=s.cuda_stream)
        s.synchronize()
    assert torch.equal(before, t_meta), "compensate_batch wrote d_meta"
    _check_frames(t_iq.cpu().numpy(), want, fs)


def test_compensate_batch_host(oracle, lphy):
    sf, osr, frames, fs = UNIFORM[0]
    d = lphy.Demodulator(sf, osr=osr)
    for x, pairs, want in _uniform_case(oracle, sf, osr, frames, fs):
        got = d.compensate_batch_host(x, frames, fs, _meta(lphy, pairs))
        assert got is not x
        _check_frames(np.asarray(got, np.complex64).view(np.float32), want, fs)


def test_compensate_batch_argument_errors(lphy):
    sf, frames, fs = 7, 2, 389
    d = lphy.Demodulator(sf)
    dev = torch.device("cuda", d.device)
    t = torch.full((frames * fs * 2 + 2,), 1.5, dtype=torch.float32, device=dev)
    t_meta = torch.zeros(frames * 32, dtype=torch.uint8, device=dev)
    cur = torch.cuda.current_stream().cuda_stream
    with pytest.raises(lphy.LphyError) as e:  # d_out = d_in + 8 bytes: neither in place nor disjoint
        d.compensate_batch(t[: frames * fs * 2], t[2:], frames, fs, t_meta, stream=cur)
    assert e.value.rc == -errno.EINVAL
    with pytest.raises(lphy.LphyError) as e:
        d.compensate_batch(t[2:], t[: frames * fs * 2], frames, fs, t_meta, stream=cur)
    assert e.value.rc == -errno.EINVAL
    d.compensate_batch(t, t, 0, fs, t_meta, stream=cur)  # frames == 0: returns 0
    d.compensate_batch(t, t, frames, 0, t_meta, stream=cur)  # no samples: returns 0
    lib, p = d.lib, t.data_ptr()
    assert lib.lphy_hip_compensate_batch(d.ctx, None, p, frames, fs, t_meta.data_ptr(), cur) == -errno.EINVAL
    assert lib.lphy_hip_compensate_batch(d.ctx, p, None, frames, fs, t_meta.data_ptr(), cur) == -errno.EINVAL
    assert lib.lphy_hip_compensate_batch(d.ctx, p, p, frames, fs, None, cur) == -errno.EINVAL
    assert lib.lphy_hip_compensate_batch(d.ctx, p, p, 1 << 31, 1, t_meta.data_ptr(), cur) == -errno.ERANGE
    assert lib.lphy_hip_compensate_ragged(d.ctx, p, p, None, frames, t_meta.data_ptr(), cur) == -errno.EINVAL
    assert lib.lphy_hip_compensate_ragged(d.ctx, p, p, t_meta.data_ptr(), 0, None, cur) == 0
    assert lib.lphy_hip_compensate_ragged(d.ctx, p, p, t_meta.data_ptr(), 1 << 31, t_meta.data_ptr(),
                                          cur) == -errno.ERANGE
    torch.cuda.synchronize()
    assert (t == 1.5).all() and (t_meta == 0).all()  # nothing was launched
