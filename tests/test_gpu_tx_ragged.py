"""lphy_hip_modulate_ragged / lphy_hip_tx_ragged: frames of different lengths
encoded and modulated in one call, compared bit for bit (uint32 views of the
floats, no tolerance) with checker.modulate(checker.encode(payload), sf, osr,
bw_hz, ampl, sync) on each frame alone.  The checker is the CPU oracle and,
where it has been built, the pinned reference build as well.

* mixed lengths: SF 7 x 70 frames (two waves in the walk pass) of 0, 1, 2, 3,
  5, 9, 16, 33 bytes in turn, over osr {1, 2} x bw {125k, 500k} x amplitude
  {1.0, 0.5, 2.0 (clamped)} x sync {0x12, 0x34}; SF 9 x 9 frames and SF 12 x 3
  frames (0, 1, 3 bytes) at osr 1; d_syms_out equals encode() per frame;
* the symbol form on the same batches, with a frame of an odd symbol count;
* hand-written descriptors: frames against their address order, gaps of 1 and
  37 samples (odd iq_offsets: the 8-byte aligned rows), a frame below two
  symbols, a frame with 3 trailing samples, a frame with an odd symbol count
  in the byte form, gaps between the symbol slots; every sample and symbol
  slot no frame owns, and a guard region on both sides of the IQ buffer, keep
  the bits of a NaN-payload sentinel;
* round trip through lphy_hip_demod_ragged on the same table (mode 2, decode);
* agreement with lphy_hip_lora_encode_batch + lphy_hip_modulate_batch;
* the host form equals the device form; the argument checks of the header;
* two calls back to back into one buffer (the parked phases leave no residue).
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ENOTSUP = -22, -34, -95
IQ_SENTINEL = 0x7FC5A5A5   # a quiet NaN with a payload: no modulator output has these bits
SYM_SENTINEL = 0xA5C3
GUARD = 64                 # samples on either side of the IQ buffer
CYCLE = [0, 1, 2, 3, 5, 9, 16, 33]


def _bits(x):
    return np.ascontiguousarray(x).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def checkers(oracle):
    """The oracle and, when it has been built, the reference itself."""
    from checkers import Reference, reference_available
    return [("oracle", oracle)] + ([("reference", Reference())] if reference_available() else [])


@pytest.fixture(scope="module")
def expected():
    """checker.modulate(checker.encode(payload) or symbols, ...) per frame, computed once per argument set."""
    cache = {}

    def get(named, src, sf, osr=1, bw=125000, ampl=1.0, sync=0x12, symbols=False):
        name, chk = named
        key = (name, bytes(src) if not symbols else np.asarray(src, np.uint16).tobytes(), symbols, sf, osr, bw, ampl,
               sync)
        if key not in cache:
            syms = np.asarray(src, np.uint16) if symbols else chk.encode(bytes(src))
            iq = chk.modulate(syms, sf, osr, bw, ampl, sync)
            iq.setflags(write=False)
            cache[key] = (syms, iq)
        return cache[key]
    return get


def payloads_of(lengths, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]


class Run:
    """One device call: the IQ buffer between two guard regions and the symbol
    slots, all pre-filled with sentinels."""

    def __init__(self, lphy, d, desc, n_iq, n_sym):
        import torch
        self.torch, self.lphy, self.d = torch, lphy, d
        self.dev = torch.device("cuda:0")
        self.desc = desc
        self.frames = desc.size - 1
        self.n_iq, self.n_sym = n_iq, n_sym
        self.t_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(self.dev)
        fill = np.full(2 * (n_iq + 2 * GUARD), IQ_SENTINEL, np.uint32).view(np.int32)
        self.t_all = torch.from_numpy(fill.copy()).to(self.dev).view(torch.float32)
        self.t_iq = self.t_all[2 * GUARD: 2 * (GUARD + n_iq)] if n_iq else self.t_all[2 * GUARD: 2 * GUARD + 2]
        self.t_syms = torch.full((max(n_sym, 1),), SYM_SENTINEL - 65536, dtype=torch.int16, device=self.dev)
        self.stream = torch.cuda.current_stream().cuda_stream

    def tx(self, data, ampl=1.0, sync=0x12, want_syms=True):
        t_data = self.torch.from_numpy(np.frombuffer(bytes(data) + b"\0", np.uint8).copy()).to(self.dev)
        self.d.tx_ragged(t_data, self.t_desc, self.frames, self.t_iq, self.t_syms if want_syms else None, ampl, sync,
                         stream=self.stream, iq_samples=self.n_iq, out_syms=self.n_sym)
        return self.fetch()

    def modulate(self, syms, ampl=1.0, sync=0x12):
        a = np.concatenate([np.asarray(syms, np.uint16), np.zeros(1, np.uint16)])
        t_in = self.torch.from_numpy(a.view(np.int16).copy()).to(self.dev)
        self.d.modulate_ragged(t_in, self.t_desc, self.frames, self.t_iq, ampl, sync, stream=self.stream,
                               iq_samples=self.n_iq, out_syms=self.n_sym)
        return self.fetch()

    def fetch(self):
        self.torch.cuda.synchronize()
        whole = self.t_all.cpu().numpy().view(np.uint32)
        assert np.all(whole[: 2 * GUARD] == IQ_SENTINEL), "the guard in front of the IQ buffer was written"
        assert np.all(whole[2 * (GUARD + self.n_iq):] == IQ_SENTINEL), "the guard behind the IQ buffer was written"
        iq = whole[2 * GUARD: 2 * (GUARD + self.n_iq)].view(np.complex64)
        return iq, self.t_syms.cpu().numpy().view(np.uint16)[: self.n_sym]


def check_iq(iq, desc, want, what):
    """want[f]: the frame's expected IQ (possibly shorter than its samples:
    the rest is not modulated).  Everything else keeps the sentinel."""
    owned = np.zeros(iq.size, bool)
    for f, x in enumerate(want):
        at = int(desc["iq_offset"][f])
        assert x.size <= int(desc["samples"][f])
        got = iq[at: at + x.size]
        bad = np.flatnonzero(_bits(got) != _bits(x))
        assert bad.size == 0, f"{what} frame {f}: {bad.size} words differ, first at sample {bad[0] // 2 if bad.size else 0}"
        owned[at: at + x.size] = True
    rest = _bits(iq).reshape(-1, 2)[~owned]
    assert np.all(rest == IQ_SENTINEL), f"{what}: {np.count_nonzero(rest != IQ_SENTINEL)} words no frame owns were written"


def check_syms(syms, desc, want, what):
    owned = np.zeros(syms.size, bool)
    for f, s in enumerate(want):
        at = int(desc["sym_offset"][f])
        np.testing.assert_array_equal(syms[at: at + s.size], s, err_msg=f"{what} frame {f}")
        owned[at: at + s.size] = True
    assert np.all(syms[~owned] == SYM_SENTINEL), what


def extent(d, lphy, desc):
    return d._ragged_extent(desc, lphy.MODE_LORA_DEMODULATE)


SF7_CASES = [(7, 70, osr, bw, ampl, sync) for osr, bw, ampl, sync in
             itertools.product([1, 2], [125000, 500000], [1.0, 0.5, 2.0], [0x12, 0x34])]
MIXED_CASES = SF7_CASES + [(9, 9, 1, 125000, 1.0, 0x12), (12, 3, 1, 125000, 1.0, 0x12)]


def mixed_lengths(sf, frames):
    return [0, 1, 3] if sf == 12 else [CYCLE[f % len(CYCLE)] for f in range(frames)]


@pytest.mark.parametrize("sf,frames,osr,bw,ampl,sync", MIXED_CASES)
def test_mixed_lengths(lphy, checkers, expected, sf, frames, osr, bw, ampl, sync):
    lens = mixed_lengths(sf, frames)
    pl = payloads_of(lens, 100 + sf)
    d = lphy.Demodulator(sf, bw_hz=bw, osr=osr)
    desc = d.tx_layout(lens)
    n_iq, n_sym = extent(d, lphy, desc)
    assert n_iq == sum(2 * n + 2 for n in lens) * (1 << sf) * osr and n_sym == 2 * sum(lens)
    iq, syms = Run(lphy, d, desc, n_iq, n_sym).tx(b"".join(pl), ampl, sync)
    for named in checkers:
        want = [expected(named, p, sf, osr, bw, ampl, sync) for p in pl]
        what = f"SF{sf} osr {osr} bw {bw} ampl {ampl} sync {sync:#x} vs {named[0]}"
        check_iq(iq, desc, [w[1] for w in want], what)
        check_syms(syms, desc, [w[0] for w in want], what)   # d_syms_out equals encode() per frame
    d.close()


@pytest.mark.parametrize("sf,frames,osr,bw,ampl,sync", [SF7_CASES[0], SF7_CASES[-1]] + MIXED_CASES[-2:])
def test_symbol_form(lphy, checkers, expected, sf, frames, osr, bw, ampl, sync):
    """The same batches through lphy_hip_modulate_ragged, plus one frame with
    an odd symbol count, which the byte form cannot express."""
    lens = mixed_lengths(sf, frames)
    pl = payloads_of(lens, 100 + sf)
    d = lphy.Demodulator(sf, bw_hz=bw, osr=osr)
    step = (1 << sf) * osr
    chk = checkers[0]
    frames_syms = [expected(chk, p, sf, osr, bw, ampl, sync)[0] for p in pl]
    frames_syms.insert(2, expected(chk, payloads_of([4], 7)[0], sf, osr, bw, ampl, sync)[0][:7])   # 7 symbols
    desc = d.ragged_layout([(s.size + 2) * step for s in frames_syms], lphy.MODE_LORA_DEMODULATE)
    n_iq, n_sym = extent(d, lphy, desc)
    flat = np.zeros(n_sym, np.uint16)
    for f, s in enumerate(frames_syms):
        at = int(desc["sym_offset"][f])
        flat[at: at + s.size] = s
    iq, _ = Run(lphy, d, desc, n_iq, n_sym).modulate(flat, ampl, sync)
    for named in checkers:
        want = [expected(named, s, sf, osr, bw, ampl, sync, symbols=True)[1] for s in frames_syms]
        assert want[2].size == 9 * step
        check_iq(iq, desc, want, f"symbol form SF{sf} osr {osr} vs {named[0]}")
    d.close()


def hand_written(sf, osr, specs):
    """specs: (payload bytes, whole symbols or None for 2 len + 2, trailing
    samples) per record.  Frames lie in memory against the record order, with
    gaps of 1 and 37 samples in turn and gaps of 4 and 2 symbol slots."""
    step = (1 << sf) * osr
    nf = len(specs)
    desc = np.zeros(nf + 1, [("iq_offset", "<u8"), ("samples", "<u8"), ("sym_offset", "<u8"), ("unit_offset", "<u8")])
    iq_at, sym_at = 5, 6
    place = {}
    for k, f in enumerate(reversed(range(nf))):
        nbytes, total, tail = specs[f]
        total = 2 * nbytes + 2 if total is None else total
        samples = total * step + tail
        place[f] = (iq_at, samples, sym_at)
        iq_at += samples + (1 if k % 2 == 0 else 37)
        sym_at += max(total - 2, 0) + (max(total - 2, 0) & 1) + (4 if k % 2 == 0 else 2)
    unit = 0
    for f in range(nf):
        desc[f] = (place[f][0], place[f][1], place[f][2], unit)
        unit += place[f][1] // step
    desc[nf] = (iq_at, 0, sym_at, unit)
    return desc


HAND_SPECS = [(3, None, 0), (0, None, 0), (5, None, 3), (0, 1, 5), (2, None, 0), (1, 5, 0), (9, None, 0), (4, None, 0),
              (0, 0, 0), (16, None, 0)]


@pytest.mark.parametrize("sf,osr", [(7, 1), (7, 2), (9, 1)])
def test_hand_written_descriptors(lphy, checkers, expected, sf, osr):
    desc = hand_written(sf, osr, HAND_SPECS)
    assert np.count_nonzero(desc["iq_offset"][:-1] & 1) >= 3 and np.count_nonzero(~desc["iq_offset"][:-1] & 1) >= 3
    assert np.all(np.diff(desc["iq_offset"][:-1].astype(np.int64)) < 0)   # reverse address order
    d = lphy.Demodulator(sf, osr=osr)
    lp = d._ragged_extent(desc, lphy.MODE_LORA_DEMODULATE)
    n_iq = int((desc["iq_offset"][:-1] + desc["samples"][:-1]).max())
    n_sym = int(desc["sym_offset"][-1])
    assert lp[0] == n_iq and lp[1] <= n_sym
    pl = payloads_of([s[0] for s in HAND_SPECS], 40 + sf)
    data = np.full(n_sym // 2 + 1, 0xEE, np.uint8)
    for f, p in enumerate(pl):
        at = int(desc["sym_offset"][f]) // 2
        data[at: at + len(p)] = np.frombuffer(p, np.uint8)
    iq, syms = Run(lphy, d, desc, n_iq, n_sym).tx(data.tobytes(), 0.75, 0x34)
    empty = np.zeros(0, np.complex64)
    for named in checkers:
        want = [expected(named, p, sf, osr, 125000, 0.75, 0x34) for p in pl]
        # records 3 and 8 have fewer than two symbols: nothing written, no symbols
        want_iq = [empty if f in (3, 8) else w[1] for f, w in enumerate(want)]
        want_sy = [np.zeros(0, np.uint16) if f in (3, 8) else w[0] for f, w in enumerate(want)]
        check_iq(iq, desc, want_iq, f"hand-written SF{sf} osr {osr} vs {named[0]}")
        check_syms(syms, desc, want_sy, f"hand-written SF{sf} osr {osr} vs {named[0]}")
    d.close()


@pytest.mark.parametrize("sf,lens", [(7, [1, 2, 3, 5, 9, 16, 0, 4]), (10, [1, 3, 0, 4])])
def test_round_trip_through_demod_ragged(lphy, oracle, sf, lens):
    import torch
    pl = payloads_of(lens, 900 + sf)
    # the precondition: the oracle's own chain returns the payloads
    for p in pl:
        x = oracle.modulate(oracle.encode(p), sf)
        r, osyms, _, _ = oracle.lora_demodulate(oracle.dechirp(x, sf), sf)
        assert r == 2 * len(p)
        r, back = oracle.lora_decode(osyms)
        assert r == len(p) and back.tobytes() == p
    d = lphy.Demodulator(sf)
    desc = d.tx_layout(lens)
    n_iq, n_sym = extent(d, lphy, desc)
    run = Run(lphy, d, desc, n_iq, n_sym)
    run.tx(b"".join(pl))
    t_syms = torch.zeros(max(n_sym, 1), dtype=torch.int16, device=run.dev)
    t_pay = torch.full(((n_sym + 1) // 2 + 1,), 0xEE, dtype=torch.uint8, device=run.dev)
    t_meta = torch.zeros(len(lens) * 32, dtype=torch.uint8, device=run.dev)
    d.demod_ragged(run.t_iq, run.t_desc, len(lens), t_syms, t_meta, lphy.MODE_DECHIRP_LORA_DEMODULATE, lphy.F_DECODE,
                   payload=t_pay, stream=run.stream, iq_samples=n_iq, out_syms=n_sym)
    torch.cuda.synchronize()
    got = t_pay.cpu().numpy()
    meta = t_meta.cpu().numpy().view(lphy.META_DTYPE)
    assert np.all(meta["status"] == 0)
    for f, p in enumerate(pl):
        at = int(desc["sym_offset"][f]) // 2
        assert got[at: at + len(p)].tobytes() == p, f"SF{sf} frame {f}"
    assert got[sum(lens):].tobytes() == b"\xee" * (got.size - sum(lens))
    d.close()


@pytest.mark.parametrize("sf,frames,nbytes", [(7, 5, 6), (7, 300, 6), (8, 3, 2)])
def test_agrees_with_the_uniform_api(lphy, sf, frames, nbytes):
    """Equal lengths: the bits of lora_encode_batch + modulate_batch (its
    few-symbol form and, from 4096 symbols per call, its two-pass batch form)."""
    import torch
    pl = payloads_of([nbytes] * frames, 5 + frames)
    d = lphy.Demodulator(sf)
    desc = d.tx_layout([nbytes] * frames)
    n_iq, n_sym = extent(d, lphy, desc)
    run = Run(lphy, d, desc, n_iq, n_sym)
    iq, syms = run.tx(b"".join(pl), 0.9, 0x12)
    t_data = torch.from_numpy(np.frombuffer(b"".join(pl), np.uint8).copy()).to(run.dev)
    t_sy = torch.zeros(frames * 2 * nbytes, dtype=torch.int16, device=run.dev)
    t_out = torch.zeros(2 * n_iq, dtype=torch.float32, device=run.dev)
    lphy.lora_encode_batch(t_data, frames, nbytes, nbytes, t_sy, 2 * nbytes, stream=run.stream)
    d.modulate_batch(t_sy, frames, 2 * nbytes, t_out, 0.9, 0x12, stream=run.stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(syms, t_sy.cpu().numpy().view(np.uint16))
    np.testing.assert_array_equal(_bits(iq), _bits(t_out.cpu().numpy()))
    d.close()


@pytest.mark.parametrize("table", ["packed", "hand"])
def test_host_form_equals_device_form(lphy, table):
    sf = 7
    d = lphy.Demodulator(sf)
    if table == "packed":
        lens = mixed_lengths(sf, 20)
        desc = d.tx_layout(lens)
        n_sym = 2 * sum(lens)
    else:
        specs = [s for f, s in enumerate(HAND_SPECS) if f not in (2, 3, 5, 8)]   # the host form refuses those
        lens = [s[0] for s in specs]
        desc = hand_written(sf, 1, specs)
        n_sym = int(desc["sym_offset"][-1])
    n_iq = int((desc["iq_offset"][:-1] + desc["samples"][:-1]).max())
    pl = payloads_of(lens, 77)
    data = np.full(n_sym // 2 + 1, 0xEE, np.uint8)
    for f, p in enumerate(pl):
        at = int(desc["sym_offset"][f]) // 2
        data[at: at + len(p)] = np.frombuffer(p, np.uint8)
    iq_d, syms_d = Run(lphy, d, desc, n_iq, n_sym).tx(data.tobytes(), 1.0, 0x12)
    h_iq = np.full(2 * n_iq, IQ_SENTINEL, np.uint32).view(np.complex64)
    h_sy = np.full(max(n_sym, 1), SYM_SENTINEL, np.uint16)
    d.reserve(len(lens), int(desc["samples"].max()))
    out_iq, out_sy, _ = d.tx_ragged_host(data, desc, 1.0, 0x12, iq=h_iq, syms_out=h_sy)
    np.testing.assert_array_equal(_bits(out_iq), _bits(iq_d))
    np.testing.assert_array_equal(out_sy[:n_sym], syms_d)
    # without the symbols, and from a list of payloads
    if table == "packed":
        iq2, none, desc2 = d.tx_ragged_host(pl, want_syms=False)
        assert none is None
        np.testing.assert_array_equal(desc2, desc)
        np.testing.assert_array_equal(_bits(iq2), _bits(iq_d))
    d.close()


def test_argument_checks(lphy):
    import torch
    dev = torch.device("cuda:0")
    sf, N = 7, 128
    d = lphy.Demodulator(sf)
    L = d.lib
    desc = d.tx_layout([1, 2])
    n_iq, n_sym = extent(d, lphy, desc)
    run = Run(lphy, d, desc, n_iq, n_sym)
    t_data = torch.zeros(8, dtype=torch.uint8, device=dev)
    t_sy = torch.zeros(8, dtype=torch.int16, device=dev)
    p_desc, p_iq, p_data, p_sy = run.t_desc.data_ptr(), run.t_iq.data_ptr(), t_data.data_ptr(), t_sy.data_ptr()
    big = 1 << 31

    def mod(ctx, syms, dsc, frames, iq):
        return L.lphy_hip_modulate_ragged(ctx, syms, dsc, frames, iq, 1.0, 0x12, None)

    def tx(ctx, data, dsc, frames, iq, out=None):
        return L.lphy_hip_tx_ragged(ctx, data, dsc, frames, iq, out, 1.0, 0x12, None)

    for fn, src in ((mod, p_sy), (tx, p_data)):
        assert fn(None, src, p_desc, 2, p_iq) == EINVAL
        assert fn(None, src, p_desc, 0, p_iq) == EINVAL          # the null ctx comes first
        assert fn(d.ctx, None, None, 0, None) == 0               # then frames == 0
        assert fn(d.ctx, None, p_desc, 2, p_iq) == EINVAL
        assert fn(d.ctx, src, None, 2, p_iq) == EINVAL
        assert fn(d.ctx, src, p_desc, 2, None) == EINVAL
        assert fn(d.ctx, src, p_desc, big, p_iq) == ERANGE
        assert fn(d.ctx, src, p_desc, big - 1, None) == EINVAL   # a null pointer before the range
    d6 = lphy.Demodulator(6)
    for fn, src in ((mod, p_sy), (tx, p_data)):
        assert fn(d6.ctx, src, p_desc, 2, p_iq) == ENOTSUP
        assert fn(d6.ctx, src, p_desc, big, p_iq) == ERANGE
        assert fn(d6.ctx, None, p_desc, 2, p_iq) == EINVAL
        assert fn(d6.ctx, src, p_desc, 0, p_iq) == 0
    iq, syms = run.fetch()
    assert np.all(_bits(iq) == IQ_SENTINEL) and np.all(syms == SYM_SENTINEL)   # none of it launched anything

    # the host form
    h_iq = np.full(2 * n_iq, IQ_SENTINEL, np.uint32).view(np.complex64)
    h_sy = np.full(n_sym, SYM_SENTINEL, np.uint16)
    data = np.arange(8, dtype=np.uint8)

    def host(ctx, data_p, dsc, frames, iq_p, sy_p):
        return L.lphy_hip_tx_ragged_host(ctx, data_p, dsc, frames, iq_p, sy_p, 1.0, 0x12)
    ok = (data.ctypes.data, desc.ctypes.data, 2, h_iq.ctypes.data, h_sy.ctypes.data)
    assert host(None, *ok) == EINVAL
    assert host(d.ctx, None, None, 0, None, None) == 0
    assert host(d.ctx, None, *ok[1:]) == EINVAL                  # the frames have bytes
    assert host(d.ctx, ok[0], None, *ok[2:]) == EINVAL
    assert host(d.ctx, ok[0], ok[1], 2, None, ok[4]) == EINVAL
    assert host(d.ctx, ok[0], ok[1], big, ok[3], ok[4]) == ERANGE
    assert host(d6.ctx, *ok) == ENOTSUP
    step = N
    for samples in (4 * step + 1, step, 5 * step):               # partial symbol, below two symbols, odd nsyms
        bad = desc.copy()
        bad["samples"][0] = samples
        bad["unit_offset"][1:] = np.cumsum(bad["samples"][:2] // step)
        assert host(d.ctx, ok[0], bad.ctypes.data, *ok[2:]) == EINVAL, samples
    bad = desc.copy()
    bad["unit_offset"][1] += 1                                   # not the prefix
    assert host(d.ctx, ok[0], bad.ctypes.data, *ok[2:]) == EINVAL
    bad = desc.copy()
    bad["samples"][1] = 1 << 31
    assert host(d.ctx, ok[0], bad.ctypes.data, *ok[2:]) == ERANGE
    assert np.all(_bits(h_iq) == IQ_SENTINEL) and np.all(h_sy == SYM_SENTINEL)   # outputs untouched
    # a table of sync symbols alone needs no bytes
    empty = d.tx_layout([0, 0])
    z_iq = np.zeros(4 * N, np.complex64)
    assert host(d.ctx, None, empty.ctypes.data, 2, z_iq.ctypes.data, None) == 0
    assert np.all(np.abs(np.abs(z_iq) - 1.0) < 1e-6)

    with pytest.raises(lphy.LphyError) as e:
        d.tx_layout([3, (1 << 23) - 1])                          # (2 len + 2) * 128 = 2^31
    assert e.value.rc == ERANGE
    assert L.lphy_hip_tx_layout(None, None, 0, desc.ctypes.data) == EINVAL
    assert L.lphy_hip_tx_layout(d.ctx, None, 1, desc.ctypes.data) == EINVAL
    d.close()
    d6.close()


def test_repeat_on_one_stream(lphy, checkers, expected):
    """Two calls back to back into the same buffer: the second finds the
    first's samples, not sentinels, where it parks its phases."""
    sf = 7
    lens = mixed_lengths(sf, 70)
    pl = payloads_of(lens, 100 + sf)
    d = lphy.Demodulator(sf)
    desc = d.tx_layout(lens)
    n_iq, n_sym = extent(d, lphy, desc)
    run = Run(lphy, d, desc, n_iq, n_sym)
    t_data = run.torch.from_numpy(np.frombuffer(b"".join(pl), np.uint8).copy()).to(run.dev)
    for _ in range(2):
        d.tx_ragged(t_data, run.t_desc, run.frames, run.t_iq, run.t_syms, 1.0, 0x12, stream=run.stream,
                    iq_samples=n_iq, out_syms=n_sym)
    twice, _ = run.fetch()
    once, _ = Run(lphy, d, desc, n_iq, n_sym).tx(b"".join(pl))
    np.testing.assert_array_equal(_bits(twice), _bits(once))
    check_iq(twice, desc, [expected(checkers[0], p, sf)[1] for p in pl], "repeat")
    d.close()
