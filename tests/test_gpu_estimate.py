"""lphy_hip_estimate_batch (lora_phy::estimate_offsets, phy.cpp:81-148) on
device buffers against the oracle's restatement, which
test_oracle_vs_reference.py pins to the reference build at osr 1 over many
symbols (test_estimate_offsets_many_symbols_bit_exact) and at osr > 1
(test_oversampled_paths_bit_exact): cfo and time_offset bit for bit, t_off
and rate recomputed from them.

k_estimate (csrc/lphy_demod.h) transforms units (symbol, osr phase), T =
Geo<SF>::T per 256-thread tile.  A frame of U = n*osr <= T units shares its
workgroup with FPT = T/U - 1 others (thread tid folds frame fbase + tid);
U > T loops one frame's units in chunks of T with the fold state carried
across chunks.  Each case below states the path it reaches and the test
checks that statement against the geometry before it runs.

Every frame has its own content, and whatever the call may not use (the
partial symbol at the end of est_samples and the rest of the frame) is NaN:
reading any of it, or another frame's samples, changes the result."""
import errno
import math

import numpy as np
import pytest
import torch

from test_oracle_vs_reference import EST_KINDS, _estimate_head, _estimate_nonfinite, _nan_bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _tile_units(sf):
    """Geo<SF>::T (csrc/lphy_fft.h): symbol slots per 256-thread tile."""
    N = 1 << sf
    return 256 // (N // min(N, 16))


def _path(sf, osr, n, frames):
    """(packed, FPT or chunk count, frames in the last workgroup, units in the
    last chunk) as k_estimate / launch_estimate_sf derive them."""
    U, T = n * osr, _tile_units(sf)
    if U <= T:
        fpt = T // U
        return True, fpt, frames - (frames - 1) // fpt * fpt, U
    chunks = -(-U // T)
    return False, chunks, 1, U - (chunks - 1) * T


# sf, osr, n symbols, frames, hann, then what the shape reaches:
# packed, FPT (packed) or chunks (unpacked), frames in the last workgroup,
# units in the last chunk
CASES = [
    (5, 1, 3, 45, False, True, 42, 3, 3),     # second workgroup holds 3 frames
    (7, 1, 5, 13, False, True, 6, 1, 5),      # slots 30, 31 idle; last workgroup holds 1 frame
    (7, 1, 32, 3, True, True, 1, 1, 32),      # U == T
    (8, 2, 3, 7, False, True, 2, 1, 6),       # U = 6 of T = 16
    (9, 1, 8, 2, False, True, 1, 1, 8),       # U == T
    (2, 1, 5, 4, False, True, 51, 4, 5),      # T = 256
    (7, 1, 33, 3, False, False, 2, 1, 1),     # last chunk holds one unit
    (7, 1, 70, 2, True, False, 3, 1, 6),      # three chunks
    (7, 3, 11, 2, False, False, 2, 1, 1),     # U = 33: the chunk edge splits symbol 10's phases
    (9, 1, 20, 3, False, False, 3, 1, 4),
    (9, 4, 5, 2, True, False, 3, 1, 4),
    (10, 1, 9, 2, False, False, 3, 1, 1),
    (11, 1, 5, 2, False, False, 3, 1, 1),
    (12, 1, 4, 3, False, False, 4, 1, 1),
    (12, 2, 3, 2, False, False, 6, 1, 1),
    (3, 1, 300, 2, False, False, 2, 1, 44),   # U = 300 > T = 256 at N = 8
]
SHAPES = [c[:5] for c in CASES]
WHOLE = [(7, 1, 5, 13, False), (9, 1, 20, 3, False)]  # again with est_samples == frame_samples == n*step


@pytest.mark.parametrize("sf,osr,n,frames,hann,packed,count,last,tail", CASES)
def test_case_reaches_its_path(sf, osr, n, frames, hann, packed, count, last, tail):
    """The table's claims, from the kernel's geometry (no device work)."""
    assert _path(sf, osr, n, frames) == (packed, count, last, tail)
    if (sf, osr, n) == (7, 3, 11):  # a chunk edge inside a symbol's osr phases
        assert _tile_units(sf) % osr != 0


_HEADS = {}


def _heads(oracle, sf, osr, n, frames, hann):
    """The frames' heads (n whole symbols each, kinds cycled from a start that
    differs per shape) and the oracle's (cfo, time_offset) for each; computed
    once per shape and shared by the tests that use it."""
    key = (sf, osr, n, frames, hann)
    if key not in _HEADS:
        rng = np.random.default_rng(9000 + 97 * sf + 13 * osr + n)
        kinds = [k for k in EST_KINDS if k != "packet_gap0"]
        start, gaps, heads = SHAPES.index(key), 0, []
        for f in range(frames):
            kind = kinds[(f + start) % 4]
            if kind == "packet_gap":
                gaps += 1
                if gaps == 2 and n >= 2:  # the second frame of this kind: symbol 0 zeroed too
                    kind = "packet_gap0"
            heads.append(_estimate_head(oracle, rng, kind, sf, osr, n))
        heads = np.stack(heads)
        want = np.stack([oracle.estimate_offsets(h, sf, osr, hann) for h in heads])
        heads.setflags(write=False)
        want.setflags(write=False)
        _HEADS[key] = (heads, want)
    return _HEADS[key]


def _layout(heads, frame_samples):
    """Frames of frame_samples samples: the head, then NaN."""
    x = np.full((heads.shape[0], frame_samples), complex(np.nan, np.nan), np.complex64)
    x[:, : heads.shape[1]] = heads
    return x


def _run(d, iq, est_samples, stream=None, fill=SENTINEL):
    """estimate_batch on the frames of `iq` ([frames, frame_samples]) with a
    sentinel-filled meta; returns (META_DTYPE records, raw bytes)."""
    import lphy
    frames, fs = iq.shape
    dev = torch.device("cuda", d.device)
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        t = torch.from_numpy(np.ascontiguousarray(iq).view(np.float32).reshape(-1).copy()).to(dev)
        meta = torch.full((max(frames, 1) * 32,), fill, dtype=torch.uint8, device=dev)
        d.estimate_batch(t, frames, fs, est_samples, meta, stream=s.cuda_stream)
        s.synchronize()
        raw = meta.cpu().numpy()
    return raw[: frames * 32].view(lphy.META_DTYPE), raw


def _round_to_int(x):
    """(int)std::round(x) of the x86-64 reference: INT_MIN for NaN / out of range."""
    x = float(x)
    if not math.isfinite(x):
        return -(1 << 31)
    r = math.copysign(math.floor(abs(x) + 0.5), x)
    return int(r) if -2147483648.0 <= r < 2147483648.0 else -(1 << 31)


def _check(meta, want, N, nonfinite=False):
    two_pi = np.float32(-2.0) * np.float32(np.pi)
    for f in range(len(want)):
        cfo, toff = np.float32(want[f][0]), np.float32(want[f][1])
        if nonfinite:
            _nan_bits_equal([meta["cfo"][f], meta["time_offset"][f]], [cfo, toff])
        else:
            assert _bits(meta["cfo"][f]) == _bits(cfo), f"frame {f}: cfo {meta['cfo'][f]!r} != {cfo!r}"
            assert _bits(meta["time_offset"][f]) == _bits(toff), \
                f"frame {f}: time_offset {meta['time_offset'][f]!r} != {toff!r}"
        assert meta["t_off"][f] == _round_to_int(toff), f"frame {f}: t_off"
        with np.errstate(invalid="ignore"):
            rate = np.float32(np.float32(two_pi * cfo) / np.float32(N))
        if nonfinite:
            _nan_bits_equal(meta["rate"][f], rate)
        else:
            assert _bits(meta["rate"][f]) == _bits(rate), f"frame {f}: rate {meta['rate'][f]!r} != {rate!r}"


def _demod(lphy, sf, osr, hann):
    return lphy.Demodulator(sf, 125000, osr, lphy.WINDOW_HANN if hann else lphy.WINDOW_NONE)


@pytest.mark.parametrize("sf,osr,n,frames,hann", SHAPES)
def test_estimate_batch_vs_oracle(oracle, lphy, sf, osr, n, frames, hann):
    """est_samples ends inside symbol n (step - 1 samples of it, NaN), the
    frame two symbols and three samples later (NaN)."""
    step = (1 << sf) * osr
    heads, want = _heads(oracle, sf, osr, n, frames, hann)
    iq = _layout(heads, (n + 2) * step + 3)
    assert np.isnan(iq[:, n * step:].view(np.float32)).all() and iq.shape[1] - n * step == 2 * step + 3
    meta, _ = _run(_demod(lphy, sf, osr, hann), iq, n * step + step - 1)
    _check(meta, want, 1 << sf)


@pytest.mark.parametrize("sf,osr,n,frames,hann", WHOLE)
def test_estimate_batch_whole_frames(oracle, lphy, sf, osr, n, frames, hann):
    """est_samples == frame_samples == n*step, as lphy_hip_estimate_host calls it."""
    heads, want = _heads(oracle, sf, osr, n, frames, hann)
    meta, _ = _run(_demod(lphy, sf, osr, hann), np.asarray(heads), n * (1 << sf) * osr)
    _check(meta, want, 1 << sf)


def test_estimate_batch_on_stream(oracle, lphy):
    sf, osr, n, frames, hann = WHOLE[0]
    step = (1 << sf) * osr
    heads, want = _heads(oracle, sf, osr, n, frames, hann)
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    meta, _ = _run(_demod(lphy, sf, osr, hann), _layout(heads, (n + 2) * step + 3), n * step + step - 1, stream=s)
    _check(meta, want, 1 << sf)


@pytest.mark.parametrize("sf,n", [(7, 5), (9, 20)])
def test_estimate_batch_nonfinite(oracle, lphy, sf, n):
    """A NaN sample in one symbol (all its bins NaN: no valid peak), an Inf
    sample in another, and both; NaN results compare as NaN."""
    step = 1 << sf
    heads = np.stack(_estimate_nonfinite(oracle, np.random.default_rng(600 + sf), sf, 1, n))
    want = np.stack([oracle.estimate_offsets(h, sf, 1, False) for h in heads])
    assert np.isfinite(want[0]).all()  # the NaN-only frame still estimates
    meta, _ = _run(_demod(lphy, sf, 1, False), _layout(heads, (n + 2) * step + 3), n * step + step - 1)
    _check(meta, want, step, nonfinite=True)


@pytest.mark.parametrize("sf,ns", [(7, (1, 2, 33)), (10, (1, 9))], ids=["sf7", "sf10"])
@pytest.mark.parametrize("hann", [False, True])
def test_estimate_host_vs_oracle(oracle, lphy, sf, ns, hann):
    """lphy_hip_estimate_host at osr 1 (the context's staging), every input kind."""
    rng = np.random.default_rng(300 + sf + hann)
    d = _demod(lphy, sf, 1, hann)
    for n in ns:
        for kind in EST_KINDS:
            if kind == "packet_gap0" and n < 2:
                continue
            x = _estimate_head(oracle, rng, kind, sf, 1, n)
            m = d.estimate_host(x)
            _check(np.array([m]), [oracle.estimate_offsets(x, sf, 1, hann)], 1 << sf)


def test_estimate_batch_writes_nothing(oracle, lphy):
    """est_samples shorter than one symbol, or no frames: 0, meta untouched."""
    sf, n, frames = 7, 3, 3
    step = 1 << sf
    heads, _ = _heads(oracle, 7, 1, 5, 13, False)
    iq = np.ascontiguousarray(heads[:frames, : n * step])
    d =_demod(lphy, sf, 1, False)
    for est in (step - 1, 0):
        _, raw = _run(d, iq, est)
        assert (raw == SENTINEL).all()
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(iq.view(np.float32).reshape(-1).copy()).to(dev)
    meta = torch.full((frames * 32,), SENTINEL, dtype=torch.uint8, device=dev)
    d.estimate_batch(t, 0, n * step, n * step, meta, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (meta.cpu().numpy() == SENTINEL).all()


@pytest.mark.parametrize("sf,n,frames,extra,have_sync", [(7, 3, 3, 2, 1), (7, 33, 2, 0, 1), (7, 1, 2, 0, 0),
                                                          (9, 1, 2, 1, 1)])
@pytest.mark.parametrize("fill", [SENTINEL, 0xFF])
def test_estimate_batch_rewrites_whole_record(oracle, lphy, sf, n, frames, extra, have_sync, fill):
    """include/lphy_hip.h: the call rewrites the whole record, status 0,
    scale 1, have_sync = (frame_samples / step >= 2), the other fields 0,
    whatever the record held (packed and unpacked path)."""
    step = 1 << sf
    rng = np.random.default_rng(sf + n)
    heads = np.stack([_estimate_head(oracle, rng, "packet", sf, 1, n) for _ in range(frames)])
    fs = (n + extra) * step
    assert (fs // step >= 2) == bool(have_sync)
    meta, _ = _run(_demod(lphy, sf, 1, False), _layout(heads, fs), n * step, fill=fill)
    _check(meta, [oracle.estimate_offsets(h, sf, 1, False) for h in heads], step)
    assert (meta["status"] == 0).all() and (_bits(meta["scale"]) == _bits(1.0)).all()
    assert (meta["have_sync"] == have_sync).all()
    for name in ("sw0", "sw1", "sync_word", "crc_ok", "normalised"):
        assert (meta[name] == 0).all(), name


@pytest.mark.parametrize("fs_syms,over", [(3, 1), (3, 128), (0, 1)])
def test_estimate_batch_rejects_est_beyond_frame(oracle, lphy, fs_syms, over):
    """est_samples > frame_samples: -EINVAL, nothing launched (meta untouched).
    The buffer holds one frame more than the call names, so that a library
    without the check would read the caller's memory only."""
    sf, frames = 7, 2
    step = 1 << sf
    fs = fs_syms * step + 5
    d = _demod(lphy, sf, 1, False)
    dev = torch.device("cuda", 0)
    t = torch.zeros((frames + 1) * (fs + over) * 2, dtype=torch.float32, device=dev)
    meta = torch.full((frames * 32,), SENTINEL, dtype=torch.uint8, device=dev)
    with pytest.raises(lphy.LphyError) as e:
        d.estimate_batch(t, frames, fs, fs + over, meta, stream=torch.cuda.current_stream().cuda_stream)
    assert e.value.rc == -errno.EINVAL
    torch.cuda.synchronize()
    assert (meta.cpu().numpy() == SENTINEL).all()
