"""lphy_hip_demod_ragged: frames of different lengths in one call, bit for
bit against the CPU oracle run on each frame alone (symbols, sync_word, the
float bits of cfo / time_offset, status, have_sync, normalised, scale,
crc_ok, bytes).

* mixed lengths at SF 7, 8, 10 and 12 in all three modes, with and without
  the Hann window, with LPHY_F_DECODE: frames of 0, 1, 2, 3 ... 66 whole
  symbols (no sync below two, an odd data-symbol count gives the decode's
  -EINVAL), noise at -8 dB, a fractional CFO on every other frame; mode 1
  also with a trailing partial symbol (samples = k N + 37), which mode 0 and
  mode 2 answer with status -EINVAL and untouched output slots;
* neighbour isolation: a delayed frame A (t_off > 0, its last symbol takes
  the end clamp) packed directly in front of a frame B of amplitude 3 and a
  frame C of amplitude 0.5: A and C keep their own normalisation and A's last
  symbol its own window; under LPHY_F_NO_SCRATCH B alone gives -ERANGE;
* hand-written descriptors with gaps in the IQ and in the outputs and frames
  out of address order;
* agreement with lphy_hip_demod_host of the same frame alone (LPHY_F_UNFUSED);
* the test build's device index checks stay at zero;
* the argument checks of the header.

The fixtures' own properties (the oracle recovers the SF 12 payloads; A's
t_off > 0 and its last symbol depends on the clamp) are checked without a GPU
in tests/test_ragged_fixtures_cpu.py."""
import numpy as np
import pytest

from test_gpu_osr import _frames

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ENOTSUP = -22, -34, -95
SENTINEL = 0xA5C3

MIXED = {7: [0, 1, 2, 3, 4, 5, 10, 34, 66, 2, 66, 3],
         8: [0, 1, 2, 3, 4, 5, 10, 34, 66, 2, 66, 3],
         10: [2, 3, 6, 1, 18],
         12: [2, 4, 3]}


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def mixed_frames(oracle, sf, counts, tail=0, seed=0):
    """One frame per whole-symbol count (plus `tail` samples of a partial
    symbol): a modulated packet cut to length, noise at -8 dB, CFO 0.3 bins on
    every other frame (test_gpu_osr._frames)."""
    N = 1 << sf
    out = []
    for k, s in enumerate(counts):
        plen = max(1, (s + 1) // 2)  # 2 plen + 2 >= s + 1 symbols
        x = _frames(oracle, sf, 1, 1, plen, seed=1000 * sf + 31 * k + seed, snr=-8.0, cfo=0.3 if k & 1 else 0.0)[0]
        out.append(np.ascontiguousarray(x[: s * N + tail]))
    return out


def sf12_frames(oracle):
    """The SF 12 fixture without the cut: whole packets of 0, 1 and 1 payload
    bytes ... as mixed_frames(12, [2, 4, 3]) builds them."""
    return mixed_frames(oracle, 12, MIXED[12])


def isolation_frames(oracle, sf=7):
    """A: 6 symbols, amplitude 0.9, CFO -0.45 bins, advanced by 5 samples (the
    estimate then gives t_off > 0 in every mode); B: 8 symbols at amplitude
    3.0; C: 6 symbols at amplitude 0.5.  Raw IQ."""
    N = 1 << sf

    def pkt(nbytes, seed):
        rng = np.random.default_rng(seed)
        return oracle.modulate(oracle.encode(rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()), sf)
    a = pkt(2, 71)
    a = (0.9 * a * np.exp(-2j * np.pi * 0.45 / N * np.arange(a.size))).astype(np.complex64)
    a = np.concatenate([a[5:], np.zeros(5, np.complex64)])
    b = (3.0 * pkt(3, 72)).astype(np.complex64)
    c = (0.5 * pkt(2, 73)).astype(np.complex64)
    return [a, b, c]


def mode_input(oracle, sf, x, mode):
    """What the caller hands to `mode`: mode 1 takes dechirped samples."""
    if mode == 1 and x.size:
        N = 1 << sf
        whole = (x.size // N) * N
        return np.concatenate([oracle.dechirp(x[:whole], sf), x[whole:]]) if whole else x
    return x


def expect(oracle, sf, x, mode, hann, decode=True, scratch=True):
    """The oracle on one frame alone -> dict of expected outputs."""
    N = 1 << sf
    total = x.size // N
    e = {"status": 0, "syms": None}
    if mode == 0:
        r, osyms, osync, omet = oracle.demodulate(x, sf, hann=hann)
        if r < 0:
            return {"status": r, "syms": None}
    else:
        if mode == 2 and x.size % N:
            return {"status": EINVAL, "syms": None}  # the uniform call's answer for this length
        src = oracle.dechirp(x, sf) if mode == 2 and x.size else x
        r, osyms, osync, omet = oracle.lora_demodulate(src, sf, hann=hann, scratch=scratch)
        mx = max(float(np.abs(src.real).max()), float(np.abs(src.imag).max())) if src.size else 0.0
        e["normalised"] = int(mx > 1.0)
        e["scale"] = np.float32(1.0) / np.float32(mx) if mx > 1.0 else np.float32(1.0)
        if r < 0:
            e["status"] = r
            return e
    e.update(syms=osyms, sync=osync, cfo=omet[0], toff=omet[1], have_sync=int(total >= 2))
    if decode:
        if len(osyms) & 1:
            e["status"] = EINVAL  # LoRaDecoder.cpp:10
        else:
            r, pay, crc = oracle.decode(osyms)
            e.update(bytes=pay, crc=crc)
    return e


def check_frame(e, syms, pay, meta, desc, f, what, fill=SENTINEL):
    m = meta[f]
    so = int(desc["sym_offset"][f])
    assert m["status"] == e["status"], what
    if "normalised" in e:
        assert m["normalised"] == e["normalised"], what
        assert _bits(m["scale"]) == _bits(e["scale"]), what
    if e["syms"] is None:
        return 0
    n = len(e["syms"])
    np.testing.assert_array_equal(syms[so: so + n], e["syms"], err_msg=what)
    assert m["sync_word"] == e["sync"], what
    assert _bits(m["cfo"]) == _bits(e["cfo"]), what
    assert _bits(m["time_offset"]) == _bits(e["toff"]), what
    assert m["have_sync"] == e["have_sync"], what
    if "bytes" in e:
        np.testing.assert_array_equal(pay[so // 2: so // 2 + n // 2], e["bytes"], err_msg=what)
        assert m["crc_ok"] == e["crc"], what
    return n


def check_batch(oracle, sf, frames, mode, hann, syms, pay, meta, desc, what, scratch=True):
    """Every frame against the oracle, and every output slot no frame owns
    still holds the sentinel."""
    owned = np.zeros(syms.size, bool)
    for f, x in enumerate(frames):
        e = expect(oracle, sf, x, mode, hann, scratch=scratch)
        n = check_frame(e, syms, pay, meta, desc, f, f"{what} frame {f} ({x.size} samples)")
        so = int(desc["sym_offset"][f])
        owned[so: so + n] = True
    assert np.all(syms[~owned] == SENTINEL), what
    bown = owned[0::2][: pay.size].copy()
    bown[: owned[1::2].size] |= owned[1::2][: bown.size]
    assert np.all(pay[: bown.size][~bown] == (SENTINEL & 0xFF)), what


@pytest.fixture(scope="module")
def mixed(oracle):
    """The mixed-length frames per (sf, tail) and their per-mode inputs, built once."""
    cache = {}

    def get(sf, mode, tail=0):
        key = (sf, mode, tail)
        if key not in cache:
            raw = cache.setdefault((sf, "raw", tail), mixed_frames(oracle, sf, MIXED[sf], tail))
            cache[key] = [mode_input(oracle, sf, x, mode) for x in raw]
        return cache[key]
    return get


@pytest.mark.parametrize("sf", [7, 8, 10, 12])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("hann", [False, True])
def test_mixed_lengths(oracle, lphy, mixed, sf, mode, hann):
    frames = mixed(sf, mode)
    d = lphy.Demodulator(sf, window=lphy.WINDOW_HANN if hann else lphy.WINDOW_NONE)
    flat = np.concatenate(frames)
    syms, pay, meta, desc = d.demod_ragged_host(flat, [x.size for x in frames], mode, lphy.F_DECODE, fill=SENTINEL)
    assert not np.any(desc["sym_offset"] & 1)
    check_batch(oracle, sf, frames, mode, hann, syms, pay, meta, desc, f"SF{sf} mode {mode} hann {hann}")


@pytest.mark.parametrize("sf", [7, 8, 10, 12])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_trailing_partial_symbol(oracle, lphy, mixed, sf, mode):
    """samples = k N + 37: mode 1 scans and demodulates the frame as the
    reference does (the partial symbol counts for the max-abs only); modes 0
    and 2 give -EINVAL per frame and write nothing."""
    frames = mixed(sf, mode, 37)
    d = lphy.Demodulator(sf)
    flat = np.concatenate(frames)
    syms, pay, meta, desc = d.demod_ragged_host(flat, [x.size for x in frames], mode, lphy.F_DECODE, fill=SENTINEL)
    if mode != 1:
        assert np.all(meta["status"] == EINVAL)
        assert np.all(syms == SENTINEL) and np.all(pay == (SENTINEL & 0xFF))
    check_batch(oracle, sf, frames, mode, False, syms, pay, meta, desc, f"SF{sf} mode {mode} tail 37")


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("no_scratch", [False, True])
def test_neighbour_isolation(oracle, lphy, mode, no_scratch):
    sf, N = 7, 128
    raw = isolation_frames(oracle, sf)
    frames = [mode_input(oracle, sf, x, mode) for x in raw]
    d = lphy.Demodulator(sf)
    flags = lphy.F_DECODE | (lphy.F_NO_SCRATCH if no_scratch else 0)
    syms, pay, meta, desc = d.demod_ragged_host(np.concatenate(frames), [x.size for x in frames], mode, flags,
                                                fill=SENTINEL)
    assert meta["t_off"][0] > 0  # A's windows are shifted, its last one clamped
    if mode != 0:
        # B does not normalise its neighbours
        assert list(meta["normalised"]) == [0, 1, 0]
        alone = [expect(oracle, sf, x, mode, False, scratch=True)["scale"] for x in frames]  # stand-alone values
        assert [int(_bits(s)) for s in meta["scale"]] == [int(_bits(s)) for s in alone]
        assert _bits(alone[0]) == _bits(1.0) == _bits(alone[2]) and 0.3 < alone[1] < 0.34
        assert list(meta["status"]) == ([0, ERANGE, 0] if no_scratch else [0, 0, 0])
    check_batch(oracle, sf, frames, mode, False, syms, pay, meta, desc, f"isolation mode {mode}",
                scratch=not no_scratch)
    # A's last symbol is the oracle's for A alone
    e = expect(oracle, sf, frames[0], mode, False)
    assert syms[int(desc["sym_offset"][0]) + len(e["syms"]) - 1] == e["syms"][-1]


@pytest.mark.parametrize("sf,mode", [(7, 1), (7, 2), (8, 0), (10, 1), (12, 2)])
def test_hand_written_descriptors(oracle, lphy, mixed, sf, mode):
    """Gaps in the IQ (filled with loud samples no frame may read) and in the
    outputs, frames listed against their address order."""
    frames = mixed(sf, mode)
    N = 1 << sf
    nf = len(frames)
    order = list(range(nf))[::-1]  # record f sits behind record f + 1 in memory
    desc = np.zeros(nf + 1, lphy.RAGGED_DESC_DTYPE)
    iq_at, sym_at, unit = 3, 6, 0
    chunks = []
    place = {}
    for f in order:
        place[f] = (iq_at, sym_at)
        chunks.append((iq_at, frames[f]))
        iq_at += frames[f].size + 11
        total = frames[f].size // N
        per = total - 2 if total >= 2 else (0 if mode == 0 else total)
        sym_at += per + (per & 1) + 4
    flat = np.full(iq_at, np.complex64(7.0 - 7.0j))
    for at, x in chunks:
        flat[at: at + x.size] = x
    for f in range(nf):
        desc[f] = (place[f][0], frames[f].size, place[f][1], unit)
        unit += frames[f].size // N
    desc[nf] = (iq_at, 0, sym_at, unit)
    d = lphy.Demodulator(sf)
    syms, pay, meta, out = d.demod_ragged_host(flat, desc, mode, lphy.F_DECODE, fill=SENTINEL)
    np.testing.assert_array_equal(out, desc)
    check_batch(oracle, sf, frames, mode, False, syms, pay, meta, desc, f"SF{sf} mode {mode} hand-written")


@pytest.mark.parametrize("sf,mode", [(7, 0), (7, 2), (10, 1), (12, 2)])
def test_agrees_with_uniform_api(lphy, mixed, sf, mode):
    frames = mixed(sf, mode)
    d = lphy.Demodulator(sf)
    syms, pay, meta, desc = d.demod_ragged_host(np.concatenate(frames), [x.size for x in frames], mode, lphy.F_DECODE)
    picked = [f for f, x in enumerate(frames) if x.size >> sf in (2, 4, 6, 34, 18)][:3]
    assert len(picked) == 3 or sf == 12
    for f in picked:
        x = frames[f]
        s1, p1, m1 = d.demod_host(x, 1, x.size, mode, lphy.F_DECODE | lphy.F_UNFUSED)
        so = int(desc["sym_offset"][f])
        np.testing.assert_array_equal(syms[so: so + s1.size], s1[0])
        np.testing.assert_array_equal(pay[so // 2: so // 2 + p1.size], p1[0])
        assert meta[f: f + 1].tobytes() == m1.tobytes()


@pytest.mark.parametrize("sf", [7, 10, 12])
def test_bounds_checked_build(lphy, mixed, sf):
    t = lphy.Demodulator(sf, test_build=True)
    p = lphy.Demodulator(sf, lib_path=lphy.HIP_SO)
    t.bounds_violations(reset=True)
    for mode in (0, 1, 2):
        for tail in (0, 37):
            frames = mixed(sf, mode, tail)
            lens = [x.size for x in frames]
            a = t.demod_ragged_host(np.concatenate(frames), lens, mode, lphy.F_DECODE, fill=SENTINEL)
            b = p.demod_ragged_host(np.concatenate(frames), lens, mode, lphy.F_DECODE, fill=SENTINEL)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
    assert t.bounds_violations() == 0


def test_device_pointer_form(oracle, lphy, mixed):
    import torch
    sf, mode = 8, 2
    frames = mixed(sf, mode)
    d = lphy.Demodulator(sf)
    desc = d.ragged_layout([x.size for x in frames], mode)
    n_iq, n_out = d._ragged_extent(desc, mode)
    dev = torch.device("cuda:0")
    t_iq = torch.from_numpy(np.concatenate(frames).view(np.float32).copy()).to(dev)
    t_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    t_syms = torch.full((n_out,), SENTINEL - 65536, dtype=torch.int16, device=dev)
    t_pay = torch.full(((n_out + 1) // 2,), SENTINEL & 0xFF, dtype=torch.uint8, device=dev)
    t_meta = torch.zeros(len(frames) * 32, dtype=torch.uint8, device=dev)
    d.demod_ragged(t_iq, t_desc, len(frames), t_syms, t_meta, mode, lphy.F_DECODE, payload=t_pay,
                   stream=torch.cuda.current_stream().cuda_stream, iq_samples=n_iq, out_syms=n_out)
    torch.cuda.synchronize()
    syms = t_syms.cpu().numpy().view(np.uint16)
    meta = t_meta.cpu().numpy().view(lphy.META_DTYPE)
    check_batch(oracle, sf, frames, mode, False, syms, t_pay.cpu().numpy(), meta, desc, "device form")


def test_argument_checks(lphy):
    N = 128
    iq = np.zeros(4 * N, np.complex64)

    def rc_of(fn):
        with pytest.raises(lphy.LphyError) as e:
            fn()
        return e.value.rc

    assert rc_of(lambda: lphy.Demodulator(7, osr=2).demod_ragged_host(iq, [4 * N], 1)) == ENOTSUP
    assert rc_of(lambda: lphy.Demodulator(6).demod_ragged_host(iq, [4 * 64], 1)) == ENOTSUP
    d = lphy.Demodulator(7)
    for fl in (lphy.F_STAGE_SYMBOLS, lphy.F_STAGE_PROLOGUE | lphy.F_STAGE_SYMBOLS, lphy.F_UNFUSED):
        assert rc_of(lambda: d.demod_ragged_host(iq, [4 * N], 1, fl)) == ENOTSUP
    # frames == 0: nothing to do
    syms, pay, meta, desc = d.demod_ragged_host(np.zeros(0, np.complex64), [], 1, lphy.F_DECODE)
    assert meta.size == 0 and desc.size == 1
    # null d_meta
    desc = d.ragged_layout([4 * N], 1)
    out = np.zeros(8, np.uint16)
    assert d.lib.lphy_hip_demod_ragged_host(d.ctx, iq.ctypes.data, desc.ctypes.data, 1, out.ctypes.data, None, None,
                                            1, 0) == EINVAL
    assert d.lib.lphy_hip_demod_ragged(d.ctx, iq.ctypes.data, desc.ctypes.data, 1, out.ctypes.data, None, None,
                                       1, 0, None) == EINVAL
    # a frame of 2^31 samples never reaches the device
    big = np.array([(0, 1 << 31, 0, 0), (1 << 31, 0, 0, 1 << 24)], lphy.RAGGED_DESC_DTYPE)
    assert rc_of(lambda: d.ragged_layout([1 << 31], 1)) == ERANGE
    meta = np.zeros(1, lphy.META_DTYPE)
    assert d.lib.lphy_hip_demod_ragged_host(d.ctx, iq.ctypes.data, big.ctypes.data, 1, out.ctypes.data, None,
                                            meta.ctypes.data, 1, 0) == ERANGE
