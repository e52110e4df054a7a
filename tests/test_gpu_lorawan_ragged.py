"""LoRaWAN on the ragged table (csrc/lphy_lorawan.hip: k_lw_build,
k_lw_parse_ragged; include/lphy_hip.h: lphy_hip_lorawan_build_ragged,
lphy_hip_lorawan_parse_ragged), SF 7 throughout:

* build against the reference's build_frame outcomes (tests/golden/lorawan_v1.json):
  one packed table, a caller's table (reverse order, one-byte gaps, prefilled
  buffers, failing frames mixed in), an osr 2 context;
* parse against the oracle and the golden, modes 1 and 0, with the
  demodulator's status gating the rows;
* keys found by DevAddr in a session table, against a Python model on
  oracle.lorawan_mic;
* the second trip of the grid-stride loops, against lphy_hip_lorawan_parse_batch;
* the whole chain build -> tx_ragged -> demod_ragged -> parse on one stream;
* every call-level return code."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = json.loads((Path(__file__).resolve().parent / "golden" / "lorawan_v1.json").read_text())
CLEAN = [c for c in GOLD["frames"] if c["variant"] == "clean"]
EINVAL, ERANGE, ENOKEY = -22, -34, -126
N = 128          # SF 7
FILL = 0xA5
FIELDS = ("status", "devaddr", "mic", "calc_mic", "payload_offset", "payload_len", "fcnt", "mhdr", "fctrl",
          "fopts_len")


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def dm(lphy):
    d = lphy.Demodulator(7)
    yield d
    d.close()


def _up(dev, a):
    torch, d = dev
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(d)


def _i32(dev, a):
    torch, d = dev
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32).copy()).to(d)


def _table(lphy, lens_bytes, step=N, total=None, byte_offsets=None):
    """A hand-written table: frame f of total[f] symbols (default 2 len + 2) with
    its bytes at byte_offsets[f] (default: back to back)."""
    lens_bytes = np.asarray(lens_bytes, np.uint64)
    total = 2 * lens_bytes + 2 if total is None else np.asarray(total, np.uint64)
    if byte_offsets is None:
        byte_offsets = np.concatenate([[0], np.cumsum(lens_bytes)])[:-1]
    desc = np.zeros(lens_bytes.size + 1, lphy.RAGGED_DESC_DTYPE)
    desc["samples"][:-1] = total * np.uint64(step)
    desc["iq_offset"] = np.concatenate([[0], np.cumsum(desc["samples"][:-1])])
    desc["sym_offset"][:-1] = 2 * np.asarray(byte_offsets, np.uint64)
    desc["unit_offset"] = np.concatenate([[0], np.cumsum(total)])
    desc["sym_offset"][-1] = int((desc["sym_offset"][:-1] + 2 * lens_bytes).max()) if lens_bytes.size else 0
    return desc


def _golden_tx(lphy, cases, rng):
    """LORAWAN_TX_DTYPE records, the source buffer (FOpts then FRMPayload per
    frame, a few stray bytes in between so that the offsets take every
    alignment) and the keys of golden build cases."""
    tx = np.zeros(len(cases), lphy.LORAWAN_TX_DTYPE)
    src = bytearray(rng.integers(0, 256, 5, dtype=np.uint8).tobytes())
    keys = np.zeros((len(cases), 16), np.uint8)
    for i, c in enumerate(cases):
        b = c["build"]
        fo, pl = bytes.fromhex(b["fopts"]), bytes.fromhex(b["payload"])
        tx[i]["src_offset"], tx[i]["devaddr"], tx[i]["key"] = len(src), b["devaddr"], i
        tx[i]["payload_len"], tx[i]["fcnt"], tx[i]["mtype"], tx[i]["major"] = len(pl), b["fcnt"], b["mtype"], b["major"]
        tx[i]["fctrl"], tx[i]["fopts_len"] = b["fctrl"], len(fo)
        src += fo + pl + rng.integers(0, 256, int(rng.integers(0, 4)), dtype=np.uint8).tobytes()
        keys[i] = np.frombuffer(bytes.fromhex(c["key"]), np.uint8)
    return tx, np.frombuffer(bytes(src) + b"\0\0\0\0", np.uint8), keys


def _build(lphy, dev, step, src, tx, desc, keys, nbytes, with_syms=True):
    """Runs lorawan_build_ragged on buffers prefilled with FILL; returns
    (bytes, symbols or None, status)."""
    torch, d = dev
    nf = tx.size
    t_bytes = torch.full((max(nbytes, 1),), FILL, dtype=torch.uint8, device=d)
    t_syms = torch.full((max(2 * nbytes, 1),), FILL * 257 - 65536, dtype=torch.int16, device=d) if with_syms else None
    t_status = torch.full((nf,), 12345, dtype=torch.int32, device=d)
    lphy.lorawan_build_ragged(_up(dev, src), _up(dev, tx), _up(dev, desc), nf, step, _up(dev, keys), t_bytes, t_status,
                              syms_out=t_syms, src_bytes=src.size, out_syms=2 * nbytes)
    torch.cuda.synchronize()
    syms = t_syms.cpu().numpy().view(np.uint16) if with_syms else None
    return t_bytes.cpu().numpy(), syms, t_status.cpu().numpy()


def _want_frame(c):
    b = np.frombuffer(bytes.fromhex(c["build"]["bytes"]), np.uint8)
    s = np.frombuffer(bytes.fromhex(c["symbols"]), "<u2")
    assert s.size == 2 * b.size == c["build"]["ret"]
    return b, s


# ----------------------------------------------------------------- build
def test_build_golden_on_a_packed_table(lphy, dev, dm):
    """Every clean golden build on one table from lorawan_tx_layout: frames
    byte-adjacent at odd alignments, payloads 0..222 and FOpts 0..15 bytes."""
    tx, src, keys = _golden_tx(lphy, CLEAN, np.random.default_rng(21))
    assert {int(t["fopts_len"]) for t in tx} >= {0, 15} and int(tx["payload_len"].max()) == 222
    desc = dm.lorawan_tx_layout(tx)
    assert dm.symbol_samples() == N
    nbytes = int(desc["sym_offset"][-1]) // 2
    got, syms, status = _build(lphy, dev, N, src, tx, desc, keys, nbytes)
    assert len({int(o) // 2 % 4 for o in desc["sym_offset"][:-1]}) == 4    # every alignment
    for i, c in enumerate(CLEAN):
        b, s = _want_frame(c)
        o = int(desc["sym_offset"][i])
        assert status[i] == c["build"]["ret"], i
        np.testing.assert_array_equal(got[o // 2:o // 2 + b.size], b, err_msg=f"frame {i}")
        np.testing.assert_array_equal(syms[o:o + s.size], s, err_msg=f"frame {i}")
    assert nbytes == sum(len(c["build"]["bytes"]) // 2 for c in CLEAN)     # no byte without an owner
    # without d_syms_out: the same bytes
    got2, _, status2 = _build(lphy, dev, N, src, tx, desc, keys, nbytes, with_syms=False)
    np.testing.assert_array_equal(got2, got)
    np.testing.assert_array_equal(status2, status)


def test_build_callers_table_gaps_and_failures(lphy, dev):
    """The same frames on a caller's table: reverse address order, one-byte gaps
    (sym_offset + 2), prefilled buffers whose unowned bytes and symbols must
    stay, and failing frames mixed in, each of which writes nothing."""
    rng = np.random.default_rng(22)
    tx, src, keys = _golden_tx(lphy, CLEAN, rng)
    nk = len(CLEAN)
    # failing frames, appended to the records: (what to change, expected status)
    base = int(np.argmax(tx["payload_len"] == 13)) if (tx["payload_len"] == 13).any() else 0
    fails = [("cap+1", ERANGE), ("cap-1", ERANGE), ("one_symbol", ERANGE), ("no_symbol", ERANGE),
             ("fopts16", EINVAL), ("mtype8", EINVAL), ("key", ENOKEY), ("huge", ERANGE)]
    ftx = np.repeat(tx[base:base + 1], len(fails))
    L0 = 12 + int(tx[base]["fopts_len"]) + int(tx[base]["payload_len"])
    slot = np.full(len(fails), L0)          # bytes of the slot each failing frame is given
    total = 2 * slot + 2
    for j, (what, _) in enumerate(fails):
        if what == "cap+1":
            slot[j], total[j] = L0 + 1, 2 * (L0 + 1) + 2
        elif what == "cap-1":
            slot[j], total[j] = L0 - 1, 2 * (L0 - 1) + 2
        elif what == "one_symbol":
            total[j] = 1
        elif what == "no_symbol":
            total[j] = 0
        elif what == "fopts16":
            ftx[j]["fopts_len"] = 16
            slot[j] = L0 + 16 - int(tx[base]["fopts_len"])
            total[j] = 2 * slot[j] + 2
        elif what == "mtype8":
            ftx[j]["mtype"] = 8
        elif what == "key":
            ftx[j]["key"] = nk
    alltx = np.concatenate([tx, ftx])
    lens = np.concatenate([[len(c["build"]["bytes"]) // 2 for c in CLEAN], slot])
    totals = np.concatenate([[2 * n + 2 for n in lens[:nk]], total])
    # interleave the failing frames with the good ones, then lay the slots out in
    # reverse record order with one free byte in front of each
    order = rng.permutation(alltx.size)
    alltx, lens, totals = alltx[order], lens[order], totals[order]
    offs = np.zeros(alltx.size, np.int64)
    at = 0
    for f in range(alltx.size - 1, -1, -1):
        at += 1
        offs[f] = at
        at += int(lens[f])
    nbytes = at + 1
    desc = _table(lphy, lens, total=totals, byte_offsets=offs)
    huge = int(np.flatnonzero(order == nk + 7)[0])
    desc["samples"][huge] = 1 << 31
    got, syms, status = _build(lphy, dev, N, src, alltx, desc, keys, nbytes)
    want_b = np.full(nbytes, FILL, np.uint8)
    want_s = np.full(2 * nbytes, FILL * 257, np.uint16)
    want_st = np.zeros(alltx.size, np.int32)
    for f, rec in enumerate(order):
        if rec < nk:
            b, s = _want_frame(CLEAN[rec])
            want_b[offs[f]:offs[f] + b.size] = b
            want_s[2 * offs[f]:2 * offs[f] + s.size] = s
            want_st[f] = CLEAN[rec]["build"]["ret"]
        else:
            want_st[f] = fails[rec - nk][1]
    np.testing.assert_array_equal(status, want_st)
    np.testing.assert_array_equal(got, want_b)
    np.testing.assert_array_equal(syms, want_s)


def test_build_odd_symbol_offset(lphy, dev):
    """A slot whose sym_offset is odd: the bytes at sym_offset // 2, the symbols
    at sym_offset as 16-bit stores, their neighbours untouched."""
    tx, src, keys = _golden_tx(lphy, CLEAN[:3], np.random.default_rng(23))
    lens = [len(c["build"]["bytes"]) // 2 for c in CLEAN[:3]]
    offs = np.array([1, 3 + lens[0], 6 + lens[0] + lens[1]])
    desc = _table(lphy, lens, byte_offsets=offs)
    desc["sym_offset"][:3] += 1
    nbytes = int(offs[2]) + lens[2] + 2
    got, syms, status = _build(lphy, dev, N, src, tx, desc, keys, nbytes)
    want_b, want_s = np.full(nbytes, FILL, np.uint8), np.full(2 * nbytes, FILL * 257, np.uint16)
    for i, c in enumerate(CLEAN[:3]):
        b, s = _want_frame(c)
        want_b[offs[i]:offs[i] + b.size] = b
        want_s[2 * offs[i] + 1:2 * offs[i] + 1 + s.size] = s
    np.testing.assert_array_equal(got, want_b)
    np.testing.assert_array_equal(syms, want_s)
    assert list(status) == [c["build"]["ret"] for c in CLEAN[:3]]


def test_build_slot_uses_the_contexts_symbol_samples(lphy, dev):
    """osr 2: a symbol is 256 samples, and the slot follows it."""
    d2 = lphy.Demodulator(7, osr=2)
    try:
        assert d2.symbol_samples() == 256
        tx, src, keys = _golden_tx(lphy, CLEAN[:6], np.random.default_rng(24))
        desc = d2.lorawan_tx_layout(tx)
        nbytes = int(desc["sym_offset"][-1]) // 2
        got, syms, status = _build(lphy, dev, 256, src, tx, desc, keys, nbytes)
        assert list(status) == [c["build"]["ret"] for c in CLEAN[:6]]
        np.testing.assert_array_equal(got, np.concatenate([_want_frame(c)[0] for c in CLEAN[:6]]))
        np.testing.assert_array_equal(syms, np.concatenate([_want_frame(c)[1] for c in CLEAN[:6]]))
        # the same table read with 128 samples per symbol: every slot is twice the frame
        got, syms, status = _build(lphy, dev, 128, src, tx, desc, keys, nbytes)
        assert (status == ERANGE).all() and (got == FILL).all() and (syms == FILL * 257).all()
    finally:
        d2.close()


# ----------------------------------------------------------------- parse
def _parse(lphy, dev, data, desc, mode, keys, step=N, meta=None, key_index=None, sessions=None):
    torch, d = dev
    nf = desc.size - 1
    t_out = torch.full((nf * 32,), 0x5A, dtype=torch.uint8, device=d)
    t_used = torch.full((nf,), 7, dtype=torch.int32, device=d)
    lphy.lorawan_parse_ragged(_up(dev, data), _up(dev, desc), nf, step, mode, _up(dev, keys), t_out,
                              meta=_up(dev, meta) if meta is not None else None,
                              key_index=_i32(dev, key_index) if key_index is not None else None,
                              sessions=_up(dev, sessions) if sessions is not None else None, key_used=t_used,
                              out_syms=2 * data.size)
    torch.cuda.synchronize()
    return t_out.cpu().numpy().view(lphy.LORAWAN_FRAME_DTYPE), t_used.cpu().numpy().view(np.uint32)


def _same(rec, want, what):
    for k in FIELDS:
        assert int(rec[k]) == want[k], (what, k, int(rec[k]), want[k])


@pytest.fixture(scope="module")
def golden_rows(oracle):
    """The decoded rows of every golden frame with the oracle's record, once."""
    rows = [bytes.fromhex(c["decoded"]) for c in GOLD["frames"]]
    keys = np.stack([np.frombuffer(bytes.fromhex(c["key"]), np.uint8) for c in GOLD["frames"]])
    want = [oracle.lorawan_parse(k, r) for k, r in zip(keys, rows)]
    for c, w in zip(GOLD["frames"], want):
        assert w["status"] == c["parse_ret"]
    assert {c["variant"] for c in GOLD["frames"]} == {"clean", "mic_flip", "bit_error", "truncated", "fopts_overrun"}
    return rows, keys, want


@pytest.mark.parametrize("mode", [1, 0])
def test_parse_golden_rows(lphy, dev, golden_rows, mode):
    """All golden rows in one ragged byte buffer; every third row sits in a frame
    with an odd symbol count (2 len + 3 symbols), the table hand-written; the
    demodulator's status gates a few rows."""
    rows, keys, want = golden_rows
    nf = len(rows)
    lens = np.array([len(r) for r in rows])
    total = 2 * lens + 2 + (np.arange(nf) % 3 == 1)
    desc = _table(lphy, lens, total=total)
    desc["samples"][:-1] += np.arange(nf, dtype=np.uint64) % 5 * (0 if mode == 0 else 25)   # a partial symbol
    data = np.frombuffer(b"".join(rows) + b"\0", np.uint8)
    meta = np.zeros(nf, lphy.META_DTYPE)
    meta["crc_ok"] = np.arange(nf) % 2          # not consulted
    meta["status"][5::17] = EINVAL
    meta["status"][9::23] = ERANGE
    recs, used = _parse(lphy, dev, data, desc, mode, keys, meta=meta, key_index=np.arange(nf))
    gated = 0
    for f in range(nf):
        if meta["status"][f]:
            w = dict.fromkeys(FIELDS, 0)
            w["status"] = int(meta["status"][f])
            gated += 1
        else:
            w = want[f]
        _same(recs[f], w, (f, GOLD["frames"][f]["variant"]))
        assert not recs[f]["reserved"].any()
        assert used[f] == (f if not meta["status"][f] and lens[f] >= 12 else lphy.LW_NO_KEY)
    assert gated > 10 and sum(1 for f in range(nf) if recs[f]["status"] >= 0) > 40
    # without d_meta nothing is gated, and without d_key_index every row gets key 0
    recs, used = _parse(lphy, dev, data, desc, mode, keys[:1])
    assert int(recs[0]["status"]) == want[0]["status"] and used[0] == 0
    assert all(int(recs[f]["status"]) == (ERANGE if lens[f] < 12 else EINVAL) for f in range(1, nf)
               if bytes(keys[f]) != bytes(keys[0]))


def test_parse_length_statuses(lphy, dev, golden_rows):
    """A frame of 2^31 samples, rows below 12 and above 65535 bytes: -ERANGE,
    the record zero otherwise; and an absent key index."""
    rows, keys, want = golden_rows
    f0 = next(i for i, c in enumerate(GOLD["frames"]) if c["variant"] == "clean")
    row = rows[f0]
    desc = _table(lphy, [len(row)] * 6, byte_offsets=[0] * 6)
    desc["samples"][1] = 1 << 31
    desc["samples"][2] = (2 * 11 + 2) * N
    desc["samples"][3] = (2 * 65536 + 2) * N
    desc["samples"][4] = N                   # one symbol: mode 1 leaves one symbol, no byte
    recs, used = _parse(lphy, dev, np.frombuffer(row + b"\0", np.uint8), desc, 1, keys[f0:f0 + 1],
                        key_index=[0, 0, 0, 0, 0, 1])
    _same(recs[0], want[f0], 0)
    for f, st in ((1, ERANGE), (2, ERANGE), (3, ERANGE), (4, ERANGE), (5, ENOKEY)):
        w = dict.fromkeys(FIELDS, 0)
        w["status"] = st
        _same(recs[f], w, f)
    assert list(used) == [0] + [lphy.LW_NO_KEY] * 5


# -------------------------------------------------------------- sessions
def _frame(oracle, rng, key, devaddr, payload_len, fopts_len, mtype=None):
    body = bytearray(rng.integers(0, 256, 8 + fopts_len + payload_len, dtype=np.uint8).tobytes())
    mtype = int(rng.integers(0, 8)) if mtype is None else mtype
    body[0] = mtype << 5 | int(rng.integers(0, 4))
    body[1:5] = int(devaddr).to_bytes(4, "little")
    body[5] = (body[5] & 0xF0) | fopts_len
    mic = oracle.lorawan_mic(key, (mtype & 1) == 0, int(devaddr), int.from_bytes(body[6:8], "little"), bytes(body))
    return bytes(body) + mic.to_bytes(4, "little")


def _session_model(oracle, lphy, sessions, keys, row):
    """The record and the key lphy_hip_lorawan_parse_ragged documents for a row
    (at least 12 bytes) looked up in `sessions`."""
    devaddr = int.from_bytes(row[1:5], "little")
    i = int(np.searchsorted(sessions["devaddr"], devaddr, side="left"))
    cand = [int(s["key"]) for s in sessions[i:i + 8] if int(s["devaddr"]) == devaddr]
    cand = [k for k in cand if k < len(keys)]
    if not cand:
        w = dict.fromkeys(FIELDS, 0)
        w.update(status=ENOKEY, devaddr=devaddr, mic=int.from_bytes(row[-4:], "little"),
                 fcnt=int.from_bytes(row[6:8], "little"), mhdr=row[0], fctrl=row[5], fopts_len=row[5] & 15)
        return w, lphy.LW_NO_KEY
    carried = int.from_bytes(row[-4:], "little")
    for k in cand:
        if oracle.lorawan_mic(keys[k], ((row[0] >> 5) & 1) == 0, devaddr, int.from_bytes(row[6:8], "little"),
                              row[:-4]) == carried:
            return oracle.lorawan_parse(keys[k], row), k
    return oracle.lorawan_parse(keys[cand[0]], row), cand[0]


def test_sessions_find_the_key_by_devaddr(oracle, lphy, dev):
    """1,000 frames of 64 devices, the key found in a sorted session table.
    DevAddrs shared by 2, 8 and 9 sessions with the right key first, last,
    eighth and ninth (the ninth is not tried: -EINVAL with the first candidate's
    calc_mic), an unknown DevAddr, a session whose key index is past the keys,
    one such session in front of the right one, and wrong MICs."""
    rng = np.random.default_rng(31)
    nkeys = 64
    keys = rng.integers(0, 256, (nkeys, 16), dtype=np.uint8)
    addr = np.unique(rng.integers(1000, 2 ** 32 - 1000, 80, dtype=np.int64))[:44]
    assert addr.size == 44
    X2, X8, X9, XBAD, XSKIP, XUNKNOWN = 7, 0x01020304, 0xFFFFFFFF, 0, 555, 600
    dev_addr = np.zeros(nkeys, np.int64)       # device i owns key i
    dev_addr[:40] = addr[:40]
    dev_addr[40:42] = X2
    dev_addr[42:50] = X8
    dev_addr[50:59] = X9
    dev_addr[59] = XBAD                         # its session names key nkeys + 3
    dev_addr[60] = XUNKNOWN                     # no session at all
    dev_addr[61] = XSKIP                        # behind a session with an unusable key
    dev_addr[62:] = addr[40:42]
    recs = [(int(dev_addr[i]), i) for i in range(nkeys) if i not in (59, 60)]
    recs += [(XBAD, nkeys + 3), (XSKIP, 1 << 31)]
    # sorted by DevAddr, devices in index order within one DevAddr; XSKIP's unusable record first
    recs.sort(key=lambda r: (r[0], r[1] != 1 << 31, r[1]))
    sessions = np.array(recs, lphy.LORAWAN_SESSION_DTYPE)
    assert lphy.lorawan_sessions_check(sessions) and not lphy.lorawan_sessions_check(sessions[::-1])
    nf = 1000
    who = rng.integers(0, nkeys, nf)
    who[:64] = np.arange(64)                    # every device at least once
    rows = []
    for f in range(nf):
        r = _frame(oracle, rng, keys[who[f]], dev_addr[who[f]], int(rng.integers(0, 31)), int(rng.integers(0, 16)))
        if f % 13 == 5:
            r = r[:-2] + bytes([r[-2] ^ 0x10]) + r[-1:]     # a wrong MIC
        rows.append(r)
    desc = _table(lphy, [len(r) for r in rows])
    data = np.frombuffer(b"".join(rows) + b"\0", np.uint8)
    got, used = _parse(lphy, dev, data, desc, 1, keys, sessions=sessions)
    seen = set()
    for f in range(nf):
        w, k = _session_model(oracle, lphy, sessions, keys, rows[f])
        _same(got[f], w, (f, int(who[f])))
        assert used[f] == k, (f, int(who[f]), int(used[f]), k)
        seen.add((int(who[f]), w["status"] >= 0))
    # what the cases above are there for, as the model sees them
    for i in (40, 41, 42, 49, 50, 57, 61, 0, 63):
        assert (i, True) in seen, i                         # first, last, eighth, behind an unusable record
    assert (58, True) not in seen and (58, False) in seen   # the ninth is not tried
    f58 = int(np.flatnonzero(who == 58)[0])
    assert int(got[f58]["status"]) == EINVAL and used[f58] == 50
    assert int(got[f58]["calc_mic"]) == oracle.lorawan_parse(keys[50], rows[f58])["calc_mic"]
    for i in (59, 60):
        f = int(np.flatnonzero(who == i)[0])
        assert int(got[f]["status"]) == ENOKEY and int(got[f]["calc_mic"]) == 0 and used[f] == lphy.LW_NO_KEY
        assert int(got[f]["devaddr"]) == dev_addr[i] and int(got[f]["mic"]) == int.from_bytes(rows[f][-4:], "little")
    # both ways to name a key at once: refused
    with pytest.raises(lphy.LphyError) as e:
        _parse(lphy, dev, data, desc, 1, keys, sessions=sessions, key_index=np.zeros(nf))
    assert e.value.rc == EINVAL


# ----------------------------------------------------------- grid-stride
def test_second_trip_of_the_grid_stride_loops(oracle, lphy, dev):
    """2048 * 256 + 257 frames of 12..24 bytes: every lane of every workgroup
    takes a second trip, the last one partial.  parse_ragged against the
    existing lphy_hip_lorawan_parse_batch on the rows repacked to padded rows;
    build_ragged on as many frames, parsed back all valid; every 997th frame
    also against the oracle."""
    torch, d = dev
    rng = np.random.default_rng(41)
    nf, nkeys, stride = 2048 * 256 + 257, 16, 24
    keys = rng.integers(0, 256, (nkeys, 16), dtype=np.uint8)
    lens = rng.integers(12, 25, nf)
    desc = _table(lphy, lens)
    offs = (desc["sym_offset"][:-1] // 2).astype(np.int64)
    data = rng.integers(0, 256, int(lens.sum()) + 1, dtype=np.uint8)
    kidx = rng.integers(0, nkeys, nf)
    t_desc, t_keys = _up(dev, desc), _up(dev, keys)
    t_out = torch.zeros(nf * 32, dtype=torch.uint8, device=d)
    lphy.lorawan_parse_ragged(_up(dev, data), t_desc, nf, N, 1, t_keys, t_out, key_index=_i32(dev, kidx),
                              out_syms=2 * (data.size - 1))
    # the route without the ragged call: padded rows and a length array
    idx = offs[:, None] + np.arange(stride)[None, :]
    padded = np.where(np.arange(stride)[None, :] < lens[:, None], data[np.minimum(idx, data.size - 1)], 0)
    t_ref = torch.zeros(nf * 32, dtype=torch.uint8, device=d)
    lphy.lorawan_parse_batch(_up(dev, padded.astype(np.uint8)), nf, stride, 0, t_keys, t_ref, lens=_i32(dev, lens),
                             key_index=_i32(dev, kidx))
    torch.cuda.synchronize()
    assert torch.equal(t_out, t_ref)
    got = t_out.cpu().numpy().view(lphy.LORAWAN_FRAME_DTYPE)
    for f in list(range(0, nf, 997)) + [nf - 1]:
        _same(got[f], oracle.lorawan_parse(keys[kidx[f]], data[offs[f]:offs[f] + lens[f]].tobytes()), f)

    # build as many frames on the same table (fopts 0..3, the payload what is left), parse them back
    tx = np.zeros(nf, lphy.LORAWAN_TX_DTYPE)
    tx["fopts_len"] = np.minimum(rng.integers(0, 4, nf), lens - 12)
    tx["payload_len"] = lens - 12 - tx["fopts_len"]
    tx["src_offset"] = offs                       # any bytes of `data` serve as FOpts and payload
    tx["devaddr"] = rng.integers(0, 2 ** 32, nf, dtype=np.uint64)
    tx["fcnt"] = rng.integers(0, 65536, nf)
    tx["mtype"], tx["major"], tx["fctrl"], tx["key"] = rng.integers(0, 8, nf), rng.integers(0, 4, nf), 0xA0, kidx
    t_bytes = torch.zeros(data.size, dtype=torch.uint8, device=d)
    t_status = torch.zeros(nf, dtype=torch.int32, device=d)
    lphy.lorawan_build_ragged(_up(dev, data), _up(dev, tx), t_desc, nf, N, t_keys, t_bytes, t_status,
                              src_bytes=data.size, out_syms=2 * (data.size - 1))
    lphy.lorawan_parse_ragged(t_bytes, t_desc, nf, N, 1, t_keys, t_out, key_index=_i32(dev, kidx),
                              out_syms=2 * (data.size - 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(t_status.cpu().numpy(), 2 * lens)
    got = t_out.cpu().numpy().view(lphy.LORAWAN_FRAME_DTYPE)
    np.testing.assert_array_equal(got["status"], tx["payload_len"].astype(np.int32))
    np.testing.assert_array_equal(got["devaddr"], tx["devaddr"])
    np.testing.assert_array_equal(got["mic"], got["calc_mic"])
    built = t_bytes.cpu().numpy()
    for f in list(range(0, nf, 997)) + [nf - 1]:
        row = built[offs[f]:offs[f] + lens[f]].tobytes()
        assert row[8:-4] == data[offs[f]:offs[f] + lens[f] - 12].tobytes()
        assert int(got["mic"][f]) == oracle.lorawan_mic(keys[kidx[f]], (int(tx["mtype"][f]) & 1) == 0,
                                                        int(tx["devaddr"][f]), int(tx["fcnt"][f]), row[:-4])


# ------------------------------------------------------------ whole chain
def test_chain_build_tx_demod_parse_on_one_stream(oracle, lphy, dev, dm):
    """lorawan_build_ragged -> tx_ragged -> demod_ragged(dechirp + demodulate,
    decode) -> lorawan_parse_ragged(d_meta, d_sessions) on one table and one
    stream, no host copy between the calls: 300 frames, payloads 0..40 bytes."""
    torch, d = dev
    rng = np.random.default_rng(51)
    nf, ndev = 300, 24
    keys = rng.integers(0, 256, (ndev, 16), dtype=np.uint8)
    addrs = np.unique(rng.integers(0, 2 ** 32, 4 * ndev, dtype=np.uint64))[:ndev].astype(np.uint32)
    sessions = np.zeros(ndev, lphy.LORAWAN_SESSION_DTYPE)
    sessions["devaddr"], sessions["key"] = addrs, rng.permutation(ndev)
    who = rng.integers(0, ndev, nf)
    tx = np.zeros(nf, lphy.LORAWAN_TX_DTYPE)
    tx["payload_len"] = rng.integers(0, 41, nf)
    tx["payload_len"][:2] = 0, 40
    tx["fopts_len"] = rng.integers(0, 16, nf)
    body = tx["payload_len"] + tx["fopts_len"]
    tx["src_offset"] = np.concatenate([[0], np.cumsum(body)])[:-1]
    tx["devaddr"], tx["key"] = sessions["devaddr"][who], sessions["key"][who]
    tx["fcnt"], tx["mtype"], tx["major"] = rng.integers(0, 65536, nf), rng.integers(0, 8, nf), rng.integers(0, 4, nf)
    tx["fctrl"] = rng.integers(0, 256, nf)
    src = rng.integers(0, 256, int(body.sum()) + 4, dtype=np.uint8)
    desc = dm.lorawan_tx_layout(tx)
    n_iq, n_sym = int(desc["iq_offset"][-1]), int(desc["sym_offset"][-1])
    step = dm.symbol_samples()
    st = torch.cuda.current_stream().cuda_stream
    t_desc, t_keys = _up(dev, desc), _up(dev, keys)
    t_built = torch.zeros(n_sym // 2, dtype=torch.uint8, device=d)
    t_status = torch.zeros(nf, dtype=torch.int32, device=d)
    t_iq = torch.zeros(2 * n_iq, dtype=torch.float32, device=d)
    t_syms = torch.zeros(n_sym, dtype=torch.int16, device=d)
    t_meta = torch.zeros(nf * 32, dtype=torch.uint8, device=d)
    t_pay = torch.zeros(n_sym // 2, dtype=torch.uint8, device=d)
    t_out = torch.zeros(nf * 32, dtype=torch.uint8, device=d)
    t_used = torch.zeros(nf, dtype=torch.int32, device=d)
    t_src, t_tx, t_sess = _up(dev, src), _up(dev, tx), _up(dev, sessions)
    lphy.lorawan_build_ragged(t_src, t_tx, t_desc, nf, step, t_keys, t_built, t_status, stream=st,
                              src_bytes=src.size, out_syms=n_sym)
    dm.tx_ragged(t_built, t_desc, nf, t_iq, stream=st, iq_samples=n_iq, out_syms=n_sym)
    dm.demod_ragged(t_iq, t_desc, nf, t_syms, t_meta, lphy.MODE_DECHIRP_LORA_DEMODULATE, lphy.F_DECODE,
                    payload=t_pay, stream=st, iq_samples=n_iq, out_syms=n_sym)
    lphy.lorawan_parse_ragged(t_pay, t_desc, nf, step, lphy.MODE_DECHIRP_LORA_DEMODULATE, t_keys, t_out,
                              meta=t_meta, sessions=t_sess, key_used=t_used, stream=st, out_syms=n_sym)
    torch.cuda.synchronize()
    L = 12 + body
    np.testing.assert_array_equal(t_status.cpu().numpy(), 2 * L)
    assert torch.equal(t_pay, t_built)
    recs = t_out.cpu().numpy().view(lphy.LORAWAN_FRAME_DTYPE)
    np.testing.assert_array_equal(recs["status"], tx["payload_len"].astype(np.int32))
    np.testing.assert_array_equal(t_used.cpu().numpy().view(np.uint32), tx["key"])
    np.testing.assert_array_equal(recs["devaddr"], tx["devaddr"])
    np.testing.assert_array_equal(recs["fcnt"], tx["fcnt"])
    assert (t_meta.cpu().numpy().view(lphy.META_DTYPE)["status"] == 0).all()
    built = t_built.cpu().numpy()
    for f in range(0, nf, 37):
        o = int(desc["sym_offset"][f]) // 2
        _same(recs[f], oracle.lorawan_parse(keys[tx["key"][f]], built[o:o + L[f]].tobytes()), f)


# -------------------------------------------------------- argument errors
def test_call_level_return_codes(lphy, dev):
    """Every return code of the two calls that comes before a launch."""
    torch, d = dev
    lib = lphy.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device=d)
    p = buf.data_ptr()
    assert p % 16 == 0
    big = 1 << 31

    def build(src=p, tx=p, desc=p, frames=1, step=N, keys=p, nkeys=1, out=p, syms=None, status=p):
        return lib.lphy_hip_lorawan_build_ragged(src, tx, desc, frames, step, keys, nkeys, out, syms, status, None)

    assert build(frames=0) == 0 and build(frames=0, src=None, tx=None, desc=None, keys=None, out=None,
                                          status=None) == 0
    for kw in (dict(src=None), dict(tx=None), dict(desc=None), dict(keys=None), dict(out=None), dict(status=None),
               dict(step=0), dict(nkeys=0), dict(keys=p + 8), dict(tx=p + 16 + 4)):
        assert build(**kw) == EINVAL, kw
    assert build(frames=big) == ERANGE and build(frames=big + 5) == ERANGE

    def parse(data=p, desc=p, frames=1, step=N, mode=1, meta=None, keys=p, nkeys=1, kidx=None, sess=None, nsess=0,
              out=p, used=None):
        return lib.lphy_hip_lorawan_parse_ragged(data, desc, frames, step, mode, meta, keys, nkeys, kidx, sess, nsess,
                                                 out, used, None)

    assert parse(frames=0) == 0 and parse(frames=0, data=None, desc=None, keys=None, out=None) == 0
    for kw in (dict(data=None), dict(desc=None), dict(keys=None), dict(out=None), dict(nkeys=0), dict(mode=3),
               dict(mode=-1), dict(step=0), dict(keys=p + 4), dict(out=p + 8), dict(kidx=p, sess=p, nsess=1),
               dict(sess=p, nsess=0)):
        assert parse(**kw) == EINVAL, kw
    assert parse(frames=big) == ERANGE
    torch.cuda.synchronize()
    assert not buf.any()        # nothing was launched


def test_tx_layout_through_the_binding(lphy, dm):
    tx = np.zeros(3, lphy.LORAWAN_TX_DTYPE)
    tx["fopts_len"], tx["payload_len"] = [0, 15, 2], [0, 7, 222]
    desc = dm.lorawan_tx_layout(tx)
    np.testing.assert_array_equal(desc, dm.tx_layout([12, 34, 236]))
    assert dm.lorawan_tx_layout(tx[:0]).size == 1
    tx["fopts_len"][1] = 16
    with pytest.raises(lphy.LphyError) as e:
        dm.lorawan_tx_layout(tx)
    assert e.value.rc == EINVAL
