"""lphy_hip_estimate_ragged (lora_phy::estimate_offsets, phy.cpp:81-148, for
every frame of a lphy_ragged_desc table in one launch) against the oracle's
restatement, which test_oracle_vs_reference.py pins to the reference build:
cfo and time_offset bit for bit, t_off and rate recomputed from them, the
rest of the record as include/lphy_hip.h states it.

k_rg_estimate (csrc/lphy_ragged.h) gives a 256-thread workgroup a group of
FPW = max(T / 2, 1) consecutive frames (T = Geo<SF>::T) and walks the group's
concatenated units, U_f = n_f * osr per frame, in passes of T; thread k folds
the units of frame k that lay in the pass and carries the fold across passes.
Each case below states what its shape reaches, and a device-free test checks
that statement against the geometry (_passes) before anything runs.

Every frame has its own content, and whatever the call may not read is NaN:
the partial symbol at the end of the estimate extent, the rest of the frame
and the gaps between frames.  A stray read changes a result."""
import errno

import numpy as np
import pytest
import torch

from test_gpu_estimate import _bits, _check, _tile_units
from test_oracle_vs_reference import EST_KINDS, _estimate_head, _estimate_nonfinite, _nan_bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
NAN = complex(np.nan, np.nan)


def _fpw(sf):
    return max(_tile_units(sf) // 2, 1)


def _nsyms(samples, est, step):
    """n_f of include/lphy_hip.h: whole symbols of min(samples, est_samples), est 0 = the frame."""
    return (min(samples, est) if est else samples) // step


def _passes(sf, osr, ns):
    """The kernel's walk, from the estimate symbol counts `ns` in record order:
    per workgroup the passes, per pass the (frame, first unit in the frame,
    units) runs it holds, in slot order."""
    T, fpw = _tile_units(sf), _fpw(sf)
    groups = []
    for g0 in range(0, len(ns), fpw):
        units = [(f, u) for f in range(g0, min(g0 + fpw, len(ns))) for u in range(ns[f] * osr)]
        passes = []
        for p0 in range(0, len(units), T):
            runs = []
            for f, u in units[p0: p0 + T]:
                if runs and runs[-1][0] == f:
                    runs[-1][2] += 1
                else:
                    runs.append([f, u, 1])
            passes.append([tuple(r) for r in runs])
        groups.append(passes)
    return groups


# ---- the tables -------------------------------------------------------------
# A case: sf, osr, hann, est_samples in samples or ("syms", k, extra) for k * step + extra,
# and per frame (whole symbols, samples of a trailing partial symbol).
def _case1():
    """SF 7, 40 frames: three workgroups of 16, 16 and 8 frames.  The counts
    cycle through 0 samples, half a symbol, 1, 2, 3, 5, 31, 32, 33 and 70
    symbols, so each group holds frames of U < T, U == T and U > T, and a pass
    holds the tail of one frame, whole frames and the head of the next."""
    step = 128
    cyc = [(0, 0), (0, step // 2), (1, 0), (2, 5), (3, 0), (5, 127), (31, 1), (32, 0), (33, 64), (70, 9)]
    return dict(sf=7, osr=1, hann=False, est=0, frames=[cyc[f % 10] for f in range(40)], shuffle=True)


def _mixed(sf, osr, hann, frames, lo, hi, mul):
    """`frames` frames of lo..hi symbols (n = lo + f * mul mod the range), a partial symbol after each."""
    step = (1 << sf) * osr
    return dict(sf=sf, osr=osr, hann=hann, est=0, shuffle=True,
                frames=[(lo + f * mul % (hi - lo + 1), (37 * f + 11) % step) for f in range(frames)])


CASES = {
    "sf7": _case1(),
    # osr > 1, 1..11 symbols, two workgroups each; at SF 7 osr 3 a pass edge splits a symbol's phases (32 % 3)
    "sf7-osr3": _mixed(7, 3, False, 19, 1, 11, 4),
    "sf8-osr2": _mixed(8, 2, False, 11, 1, 11, 3),
    "sf9-osr4-hann": _mixed(9, 4, True, 7, 1, 11, 5),
    # T <= 4: 1..5 symbols, every workgroup walks more than one pass
    "sf10": _mixed(10, 1, False, 5, 1, 5, 3),
    "sf11": _mixed(11, 1, False, 4, 1, 5, 2),
    "sf12": _mixed(12, 1, False, 3, 1, 5, 2),
    "sf12-osr2": _mixed(12, 2, False, 3, 1, 5, 4),
}
BOUNDS = list(CASES)  # cases 1-3 of the issue, once more through the checked build
# est_samples caps on frames of 1, 2 and 9 symbols (SF 7, one workgroup)
CAP_FRAMES = [(1, 17), (2, 0), (9, 3), (9, 0), (2, 100), (1, 0)]
CAPS = {
    "two-symbols": 2 * 128,        # exactly two symbols
    "partial-in-cap": 2 * 128 + 5,  # the five samples past them lie inside the cap and are not read
}

_TABLES = {}


def _table(oracle, lphy, key, case=None, heads=None):
    """The IQ buffer (NaN outside the frames' estimate symbols), the records
    and the oracle's (cfo, time_offset) per frame, built once per key."""
    if key in _TABLES:
        return _TABLES[key]
    c = case or CASES[key]
    sf, osr, hann, est = c["sf"], c["osr"], c["hann"], c["est"]
    step = (1 << sf) * osr
    samples = [n * step + part for n, part in c["frames"]]
    ns = [_nsyms(s, est, step) for s in samples]
    rng = np.random.default_rng(7000 + sum(map(ord, key)))
    kinds = [k for k in EST_KINDS if k != "packet_gap0"]
    if heads is None:
        heads = []
        for f, n in enumerate(ns):
            kind = kinds[(f + len(key)) % 4]
            if kind == "packet_gap" and n >= 2 and f % 8 >= 4:
                kind = "packet_gap0"
            heads.append(_estimate_head(oracle, rng, kind, sf, osr, n) if n else np.zeros(0, np.complex64))
    assert [h.size for h in heads] == [n * step for n in ns]
    # frames in shuffled address order with gaps of 1..5 samples (or back to back)
    order = rng.permutation(len(samples)) if c.get("shuffle") else np.arange(len(samples))
    desc = np.zeros(len(samples), lphy.RAGGED_DESC_DTYPE)  # (no record [frames]: it is not read)
    pos = 3 if c.get("shuffle") else 0
    for f in order:
        desc["iq_offset"][f] = pos
        pos += samples[f] + (1 + int(f) % 5 if c.get("shuffle") else 0)
    desc["samples"] = samples
    desc["sym_offset"], desc["unit_offset"] = 0xDEADBEEF, 0xFEEDFACE  # not read
    iq = np.full(max(pos, 1), NAN, np.complex64)
    for f, h in enumerate(heads):
        o = int(desc["iq_offset"][f])
        iq[o: o + h.size] = h
    want = [oracle.estimate_offsets(h, sf, osr, hann) if h.size else None for h in heads]
    iq.setflags(write=False)
    desc.setflags(write=False)
    _TABLES[key] = dict(sf=sf, osr=osr, hann=hann, est=est, step=step, samples=samples, ns=ns, iq=iq, desc=desc,
                        want=want, extent=pos)
    return _TABLES[key]


def _demod(lphy, t, **kw):
    return lphy.Demodulator(t["sf"], 125000, t["osr"], lphy.WINDOW_HANN if t["hann"] else lphy.WINDOW_NONE, **kw)


def _run(lphy, d, t, est=None, fill=SENTINEL):
    """estimate_ragged on table t with every record filled with `fill`; the records' raw bytes."""
    dev = torch.device("cuda", d.device)
    frames = len(t["samples"])
    t_iq = torch.from_numpy(t["iq"].view(np.float32).copy()).to(dev)
    t_desc = torch.from_numpy(t["desc"].view(np.uint8).copy()).to(dev)
    t_meta = torch.full((frames * 32,), fill, dtype=torch.uint8, device=dev)
    d.estimate_ragged(t_iq, t_desc, frames, t["est"] if est is None else est, t_meta,
                      stream=torch.cuda.current_stream().cuda_stream, iq_samples=t["extent"])
    torch.cuda.synchronize()
    assert (t_desc.cpu().numpy() == t["desc"].view(np.uint8)).all(), "d_desc written"
    return t_meta.cpu().numpy()


def _check_table(lphy, t, raw, fill=SENTINEL, nonfinite=()):
    """Every record of `raw` as include/lphy_hip.h states it for table t."""
    meta = raw.view(lphy.META_DTYPE)
    N = 1 << t["sf"]
    for f, n in enumerate(t["ns"]):
        if n == 0:
            assert (raw[32 * f: 32 * f + 32] == fill).all(), f"frame {f}: no whole symbol, record written"
            continue
        try:
            _check(meta[f: f + 1], [t["want"][f]], N, nonfinite=f in nonfinite)
        except AssertionError as e:
            raise AssertionError(f"frame {f} ({n} symbols): {e}") from None
        m = meta[f]
        assert m["status"] == 0 and _bits(m["scale"]) == _bits(1.0), f"frame {f}"
        assert m["have_sync"] == (t["samples"][f] // t["step"] >= 2), f"frame {f}: have_sync"
        for name in ("sw0", "sw1", "sync_word", "crc_ok", "normalised"):
            assert m[name] == 0, f"frame {f}: {name}"


# ---- what the shapes reach (no device work) -----------------------------------
def test_cases_reach_their_paths():
    ns = {k: [_nsyms(n * (1 << c["sf"]) * c["osr"] + part, 0, (1 << c["sf"]) * c["osr"]) for n, part in c["frames"]]
          for k, c in CASES.items()}
    # case 1: three workgroups, the last partly filled; U < T, U == T and U > T in one group; a pass
    # with the tail of one frame, whole frames and the head of the next
    g = _passes(7, 1, ns["sf7"])
    assert _fpw(7) == 16 and len(g) == 3 and len(ns["sf7"]) - 2 * 16 == 8
    assert ns["sf7"].count(0) == 8  # the 0-sample and the half-symbol frames
    for g0 in (0, 16, 32):
        us = [u for u in ns["sf7"][g0: g0 + 16] if u]
        assert min(us) < 32 and 32 in us and max(us) > 32
    mixed = [p for passes in g for p in passes
             if len(p) >= 3 and p[0][1] > 0 and p[-1][1] == 0 and p[-1][2] < ns["sf7"][p[-1][0]]
             and all(u == 0 and k == ns["sf7"][f] for f, u, k in p[1:-1])]
    assert mixed, "no pass holds a tail, whole frames and a head"
    # osr > 1: two workgroups each; SF 7 osr 3: a pass starts between the phases of a symbol
    for key, sf, osr in (("sf7-osr3", 7, 3), ("sf8-osr2", 8, 2), ("sf9-osr4-hann", 9, 4)):
        g = _passes(sf, osr, ns[key])
        assert len(g) == 2 and min(ns[key]) == 1 and max(ns[key]) == 11
        assert any(len(passes) > 1 for passes in g)
    assert _tile_units(7) % 3 != 0
    assert any(p[0][1] % 3 != 0 for passes in _passes(7, 3, ns["sf7-osr3"]) for p in passes)
    # large SF: T <= 4, 3-5 frames of 1..5 symbols: every frame of more than T units lies in more than
    # one pass (there is one), its fold carried across them
    for key, sf, osr in (("sf10", 10, 1), ("sf11", 11, 1), ("sf12", 12, 1), ("sf12-osr2", 12, 2)):
        T = _tile_units(sf)
        assert T <= 4 and 3 <= len(ns[key]) <= 5 and min(ns[key]) == 1 and max(ns[key]) == 5
        g = _passes(sf, osr, ns[key])
        seen = {f: sum(1 for passes in g for p in passes for r in p if r[0] == f) for f in range(len(ns[key]))}
        assert all(seen[f] > 1 for f, n in enumerate(ns[key]) if n * osr > T) and max(seen.values()) > 1
    # the caps: frames of 1, 2 and 9 symbols in one workgroup
    assert sorted({n for n, _ in CAP_FRAMES}) == [1, 2, 9] and len(CAP_FRAMES) <= _fpw(7)
    assert [_nsyms(n * 128 + p, 2 * 128, 128) for n, p in CAP_FRAMES] == [1, 2, 2, 2, 2, 1]
    assert [_nsyms(n * 128 + p, 2 * 128 + 5, 128) for n, p in CAP_FRAMES] == [1, 2, 2, 2, 2, 1]


# ---- against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_estimate_ragged_vs_oracle(oracle, lphy, key):
    t = _table(oracle, lphy, key)
    _check_table(lphy, t, _run(lphy, _demod(lphy, t), t))


@pytest.mark.parametrize("name", list(CAPS))
def test_estimate_ragged_cap(oracle, lphy, name):
    """est_samples caps the estimate: what lies past the cap's whole symbols is NaN here."""
    case = dict(sf=7, osr=1, hann=False, est=CAPS[name], frames=CAP_FRAMES, shuffle=True)
    t = _table(oracle, lphy, "cap-" + name, case)
    assert t["ns"] == [1, 2, 2, 2, 2, 1]
    _check_table(lphy, t, _run(lphy, _demod(lphy, t), t))


def test_estimate_ragged_cap_beyond_every_frame_is_cap_zero(oracle, lphy):
    t = _table(oracle, lphy, "sf8-osr2")
    d = _demod(lphy, t)
    whole = _run(lphy, d, t, est=0)
    for est in (max(t["samples"]) + 1, 1 << 40):
        assert (_run(lphy, d, t, est=est) == whole).all()
    _check_table(lphy, t, whole)


@pytest.mark.parametrize("sf,osr,n,frames,hann", [(7, 1, 5, 13, False), (7, 3, 11, 5, False), (9, 1, 20, 3, True),
                                                  (12, 1, 3, 2, False)])
def test_estimate_ragged_equals_uniform_call(oracle, lphy, sf, osr, n, frames, hann):
    """On a table from ragged_layout with equal lengths the records equal
    estimate_batch's bytewise (and the oracle's, through _check_table)."""
    step = (1 << sf) * osr
    fs, est = (n + 2) * step + 3, n * step + step - 1
    case = dict(sf=sf, osr=osr, hann=hann, est=est, frames=[(n + 2, 3)] * frames)
    t = _table(oracle, lphy, f"uniform-{sf}-{osr}-{n}", case)
    d = _demod(lphy, t)
    desc = d.ragged_layout([fs] * frames, lphy.MODE_DEMODULATE)
    assert (desc["iq_offset"][:-1] == t["desc"]["iq_offset"]).all() and t["extent"] == frames * fs
    dev = torch.device("cuda", d.device)
    st = torch.cuda.current_stream().cuda_stream
    t_iq = torch.from_numpy(t["iq"].view(np.float32).copy()).to(dev)
    t_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    a = torch.full((frames * 32,), SENTINEL, dtype=torch.uint8, device=dev)
    b = torch.full((frames * 32,), 0x3C, dtype=torch.uint8, device=dev)
    d.estimate_ragged(t_iq, t_desc, frames, est, a, stream=st, iq_samples=frames * fs)
    d.estimate_batch(t_iq, frames, fs, est, b, stream=st)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    _check_table(lphy, t, a.cpu().numpy())


@pytest.mark.parametrize("sf,n,lens", [(7, 5, (3, 1, 40, 2)), (9, 20, (7,))], ids=["sf7", "sf9"])
def test_estimate_ragged_nonfinite(oracle, lphy, sf, n, lens):
    """A NaN sample in one symbol, an Inf sample in another, and both, among
    finite frames of other lengths in one workgroup; NaN results compare as NaN."""
    step = 1 << sf
    bad = _estimate_nonfinite(oracle, np.random.default_rng(600 + sf), sf, 1, n)
    rng = np.random.default_rng(640 + sf)
    fin = [_estimate_head(oracle, rng, "packet", sf, 1, k) for k in lens]
    heads = [fin[0], bad[0], bad[1]] + fin[1:] + [bad[2]]
    assert len(heads) <= _fpw(sf)
    case = dict(sf=sf, osr=1, hann=False, est=0, frames=[(h.size // step, 9) for h in heads], shuffle=True)
    t = _table(oracle, lphy, f"nonfinite-{sf}", case, heads=heads)
    assert np.isfinite(t["want"][1]).all()  # the NaN-only frame still estimates
    _check_table(lphy, t, _run(lphy, _demod(lphy, t), t), nonfinite=(1, 2, len(heads) - 1))


# ---- hand-written tables, return codes ----------------------------------------
def test_estimate_ragged_frame_of_2_31_samples(oracle, lphy):
    """samples = 2^31: status -ERANGE, the record otherwise zero, nothing read
    (its iq_offset lies far outside the buffer); its neighbours in the group
    are unaffected."""
    t = _table(oracle, lphy, "sf8-osr2")
    frames = len(t["samples"])
    big = 2
    desc = t["desc"].copy()
    desc["samples"][big] = 1 << 31
    desc["iq_offset"][big] = 1 << 40
    assert big < _fpw(8) and frames > _fpw(8)
    d = _demod(lphy, t)
    raw = _run(lphy, d, dict(t, desc=desc))
    zero = np.zeros(1, lphy.META_DTYPE)
    zero["status"] = -errno.ERANGE
    assert raw[32 * big: 32 * big + 32].tobytes() == zero.tobytes()
    # the other records: as the oracle gives them (the frame's own record put aside)
    rest = raw.copy()
    rest[32 * big: 32 * big + 32] = SENTINEL
    _check_table(lphy, dict(t, ns=[0 if f == big else n for f, n in enumerate(t["ns"])]), rest)


def test_estimate_ragged_return_codes(lphy):
    """include/lphy_hip.h's order, device and host form: null ctx, frames == 0,
    null buffers, frames >= 2^31, SF < 7.  Nothing is launched."""
    EINVAL, ERANGE, ENOTSUP = -errno.EINVAL, -errno.ERANGE, -errno.ENOTSUP
    dev = torch.device("cuda", 0)
    t = torch.full((64,), 1.5, dtype=torch.float32, device=dev)
    t_meta = torch.full((64,), SENTINEL, dtype=torch.uint8, device=dev)
    t_desc = torch.zeros(64, dtype=torch.uint8, device=dev)
    cur = torch.cuda.current_stream().cuda_stream
    h_iq, h_desc, h_meta = np.zeros(8, np.float32), np.zeros(2, lphy.RAGGED_DESC_DTYPE), np.zeros(1, lphy.META_DTYPE)
    for sf in (7, 6):
        d = lphy.Demodulator(sf)
        fn, p, pd, pm = d.lib.lphy_hip_estimate_ragged, t.data_ptr(), t_desc.data_ptr(), t_meta.data_ptr()
        assert fn(None, p, pd, 0, 0, pm, cur) == EINVAL
        assert fn(d.ctx, None, None, 0, 0, None, cur) == 0
        assert fn(d.ctx, None, pd, 1, 0, pm, cur) == EINVAL
        assert fn(d.ctx, p, None, 1, 0, pm, cur) == EINVAL
        assert fn(d.ctx, p, pd, 1, 0, None, cur) == EINVAL
        assert fn(d.ctx, None, pd, 1 << 31, 0, pm, cur) == EINVAL
        assert fn(d.ctx, p, pd, 1 << 31, 0, pm, cur) == ERANGE
        fh, q, qd, qm = d.lib.lphy_hip_estimate_ragged_host, h_iq.ctypes.data, h_desc.ctypes.data, h_meta.ctypes.data
        assert fh(None, q, qd, 0, 0, qm) == EINVAL
        assert fh(d.ctx, None, None, 0, 0, None) == 0
        assert fh(d.ctx, None, qd, 1, 0, qm) == EINVAL
        assert fh(d.ctx, q, None, 1, 0, qm) == EINVAL
        assert fh(d.ctx, q, qd, 1, 0, None) == EINVAL
        assert fh(d.ctx, q, qd, 1 << 31, 0, qm) == ERANGE
        if sf < 7:
            assert fn(d.ctx, p, pd, 1, 0, pm, cur) == ENOTSUP
            assert fh(d.ctx, q, qd, 1, 0, qm) == ENOTSUP
    # the host form reads its table before any device call
    d = lphy.Demodulator(7)
    big = np.array([(0, 1 << 31, 0, 0), (0, 0, 0, 0)], lphy.RAGGED_DESC_DTYPE)
    assert d.lib.lphy_hip_estimate_ragged_host(d.ctx, h_iq.ctypes.data, big.ctypes.data, 1, 0,
                                               h_meta.ctypes.data) == ERANGE
    torch.cuda.synchronize()
    assert (t == 1.5).all() and (t_meta == SENTINEL).all() and (h_meta.view(np.uint8) == 0).all()


def test_estimate_ragged_binding_checks(oracle, lphy):
    t = _table(oracle, lphy, "sf10")
    d = _demod(lphy, t)
    dev = torch.device("cuda", d.device)
    frames = len(t["samples"])
    t_iq = torch.zeros(t["extent"] * 2, dtype=torch.float32, device=dev)
    t_desc = torch.zeros(frames * 32, dtype=torch.uint8, device=dev)
    t_meta = torch.zeros(frames * 32, dtype=torch.uint8, device=dev)
    for iq, desc, meta in ((t_iq[:-2], t_desc, t_meta), (t_iq, t_desc[:-1], t_meta), (t_iq, t_desc, t_meta[:-1]),
                           (t_iq.cpu(), t_desc, t_meta)):
        with pytest.raises(ValueError):
            d.estimate_ragged(iq, desc, frames, 0, meta, iq_samples=t["extent"])


# ---- the host form ----------------------------------------------------------------
def test_estimate_ragged_host(oracle, lphy):
    """Equal to the device form; records of frames without a whole symbol keep
    the caller's values; a second call on a context reserved for the
    documented shape (`frames` frames of up to frame_samples each)."""
    t = _table(oracle, lphy, "sf7")
    frames = len(t["samples"])
    d = _demod(lphy, t)
    dev_raw = _run(lphy, d, t)
    desc = np.concatenate([t["desc"], np.zeros(1, lphy.RAGGED_DESC_DTYPE)])
    mine = np.frombuffer(bytes(range(32)) * frames, lphy.META_DTYPE)
    h = _demod(lphy, t)
    h.reserve(frames, max(t["samples"]))
    for _ in range(2):
        got, _ = h.estimate_ragged_host(t["iq"], desc, 0, meta=mine)
        raw = got.view(np.uint8)
        for f, n in enumerate(t["ns"]):
            want = mine.view(np.uint8)[32 * f: 32 * f + 32] if n == 0 else dev_raw[32 * f: 32 * f + 32]
            assert (raw[32 * f: 32 * f + 32] == want).all(), f"frame {f}"
    assert t["ns"].count(0) == 8
    # lengths in, frames back to back, a cap
    t2 = _table(oracle, lphy, "cap-host", dict(sf=7, osr=1, hann=False, est=2 * 128 + 5, frames=CAP_FRAMES))
    got, desc2 = h.estimate_ragged_host(t2["iq"], t2["samples"], t2["est"])
    assert (desc2["iq_offset"][:-1] == t2["desc"]["iq_offset"]).all()
    _check_table(lphy, t2, got.view(np.uint8), fill=0)


# ---- the checked build ----------------------------------------------------------------
@pytest.mark.parametrize("key", BOUNDS)
def test_estimate_ragged_bounds_build(oracle, lphy, key):
    """The same cases through lib/test/: no device index check fails, same records."""
    t = _table(oracle, lphy, key)
    d = _demod(lphy, t, test_build=True)
    d.bounds_violations(reset=True)
    _check_table(lphy, t, _run(lphy, d, t))
    assert d.bounds_violations() == 0
