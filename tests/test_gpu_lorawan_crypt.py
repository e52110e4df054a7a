"""The LoRaWAN FRMPayload cipher on the GPU (csrc/lphy_lorawan.hip: k_lw_crypt;
include/lphy_hip.h: lphy_hip_lorawan_crypt_batch, _crypt_tx_ragged,
_crypt_rx_ragged, _crypt_host), against the restatement of LoRaWAN 1.0.x 4.3.3
in tests/lorawan_crypt_model.py on the checkers' AES-128:

* batch: ranges of 0..4080 bytes at every alignment, byte-adjacent, guards
  around them, with and without d_status, twice (its own inverse);
* refused jobs between good ones;
* the later trips of the grid-stride loop;
* crypt_tx_ragged + build_ragged against build_frame on the host-ciphered
  payload;
* the whole loop crypt_tx -> build -> tx -> demod -> parse -> crypt_rx on one
  stream, with refused frames;
* forged parse records; every call-level return code; the host form."""
import numpy as np
import pytest

from lorawan_crypt_model import checkers_cipher

pytestmark = pytest.mark.gpu
EINVAL, ERANGE, ENOKEY = -22, -34, -126
N = 128          # SF 7
FILL = 0xA5
GUARD = 64
LENGTHS = (0, 1, 3, 15, 16, 17, 31, 32, 33, 47, 48, 255, 4080)


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def dm(lphy):
    d = lphy.Demodulator(7)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cipher():
    return checkers_cipher()


def _up(dev, a):
    torch, d = dev
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(d)


def _i32(dev, a):
    torch, d = dev
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32).copy()).to(d)


def _distinct(rng, n):
    """n 32-bit values whose four bytes all differ."""
    b = np.stack([rng.permutation(256)[:4] for _ in range(n)]).astype(np.uint64)
    return (b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16 | b[:, 3] << 24).astype(np.uint32)


def _table(lphy, lens_bytes, byte_offsets=None):
    """Frame f of 2 len + 2 symbols with its bytes at byte_offsets[f] (default:
    back to back)."""
    lens_bytes = np.asarray(lens_bytes, np.uint64)
    total = 2 * lens_bytes + 2
    if byte_offsets is None:
        byte_offsets = np.concatenate([[0], np.cumsum(lens_bytes)])[:-1]
    desc = np.zeros(lens_bytes.size + 1, lphy.RAGGED_DESC_DTYPE)
    desc["samples"][:-1] = total * np.uint64(N)
    desc["iq_offset"] = np.concatenate([[0], np.cumsum(desc["samples"][:-1])])
    desc["sym_offset"][:-1] = 2 * np.asarray(byte_offsets, np.uint64)
    desc["unit_offset"] = np.concatenate([[0], np.cumsum(total)])
    desc["sym_offset"][-1] = int((desc["sym_offset"][:-1] + 2 * lens_bytes).max()) if lens_bytes.size else 0
    return desc


def _crypt_batch(lphy, dev, buf, jobs, keys, with_status=True):
    torch, d = dev
    t_buf = _up(dev, buf)
    t_status = torch.full((jobs.size,), 12345, dtype=torch.int32, device=d) if with_status else None
    lphy.lorawan_crypt_batch(t_buf, _up(dev, jobs), _up(dev, keys), status=t_status)
    torch.cuda.synchronize()
    return t_buf.cpu().numpy(), (t_status.cpu().numpy() if with_status else None)


# ----------------------------------------------------------------- batch
@pytest.fixture(scope="module")
def batch_case(lphy, cipher):
    """300 jobs: every length at every start alignment five times (a gap of up to
    three unowned bytes where the alignment needs one), then 40 strictly back to
    back; 64 guard bytes in front, behind and in four gaps.  The expectation is
    computed once."""
    rng = np.random.default_rng(61)
    nkeys = 5
    keys = rng.integers(0, 256, (nkeys, 16), dtype=np.uint8)
    combos = [(n, a) for n in LENGTHS for a in range(4)] * 5
    order = rng.permutation(len(combos))
    plan = [combos[i] for i in order] + [(int(n), None) for n in rng.choice(LENGTHS[:-1], 40)]
    jobs = np.zeros(len(plan), lphy.LORAWAN_DESC_DTYPE)
    at = GUARD
    for j, (n, align) in enumerate(plan):
        if j and j % 60 == 0:
            at += GUARD
        if align is not None:
            at += (align - at) % 4
        jobs[j]["offset"], jobs[j]["len"] = at, n
        at += n
    jobs["devaddr"], jobs["fcnt"] = _distinct(rng, jobs.size), _distinct(rng, jobs.size)
    jobs["key"], jobs["uplink"] = rng.integers(0, nkeys, jobs.size), rng.integers(0, 2, jobs.size) * 3
    buf = rng.integers(0, 256, at + GUARD, dtype=np.uint8)
    want = buf.copy()
    for j in jobs:
        o, n = int(j["offset"]), int(j["len"])
        want[o:o + n] ^= cipher.keystream(keys[j["key"]], bool(j["uplink"]), int(j["devaddr"]), int(j["fcnt"]), n)
    assert jobs.size == 300 and {(int(j["len"]), int(j["offset"]) % 4) for j in jobs} >= set(combos)
    assert len(set(jobs["key"])) == nkeys and len(set(jobs["uplink"] != 0)) == 2
    return keys, jobs, buf, want


@pytest.mark.parametrize("with_status", [True, False])
def test_batch_every_length_and_alignment(lphy, dev, batch_case, with_status):
    """Every range is plaintext XOR keystream, every byte outside the ranges is
    unchanged, every status is 0, and a second call restores the buffer."""
    keys, jobs, buf, want = batch_case
    got, status = _crypt_batch(lphy, dev, buf, jobs, keys, with_status)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], int(np.searchsorted(jobs["offset"], bad[0], side="right")) - 1)
    assert (got != buf).sum() > 0.99 * int(jobs["len"].sum())
    back, status2 = _crypt_batch(lphy, dev, got, jobs, keys, with_status)
    np.testing.assert_array_equal(back, buf)
    if with_status:
        assert not status.any() and not status2.any()


def test_refused_jobs_between_good_ones(lphy, dev, cipher):
    rng = np.random.default_rng(62)
    nkeys = 3
    keys = rng.integers(0, 256, (nkeys, 16), dtype=np.uint8)
    lens = [20, 4081, 33, 10, 5, 4080]
    jobs = np.zeros(len(lens), lphy.LORAWAN_DESC_DTYPE)
    jobs["len"] = lens
    jobs["offset"] = GUARD + 1 + np.concatenate([[0], np.cumsum(lens)])[:-1]
    jobs["devaddr"], jobs["fcnt"] = _distinct(rng, jobs.size), _distinct(rng, jobs.size)
    jobs["key"], jobs["uplink"] = [0, 1, 2, nkeys, 1, 0], [1, 1, 0, 1, 0, 1]
    buf = rng.integers(0, 256, GUARD + 1 + sum(lens) + GUARD, dtype=np.uint8)
    want, want_st = buf.copy(), [0, ERANGE, 0, ENOKEY, 0, 0]
    for j, st in zip(jobs, want_st):
        if st == 0:
            o, n = int(j["offset"]), int(j["len"])
            want[o:o + n] ^= cipher.keystream(keys[j["key"]], bool(j["uplink"]), int(j["devaddr"]), int(j["fcnt"]), n)
    got, status = _crypt_batch(lphy, dev, buf, jobs, keys)
    assert list(status) == want_st
    np.testing.assert_array_equal(got, want)
    # without d_status the refused jobs still write nothing
    got, _ = _crypt_batch(lphy, dev, buf, jobs, keys, with_status=False)
    np.testing.assert_array_equal(got, want)


def test_later_trips_of_the_grid_stride_loop(lphy, dev, cipher):
    """2048 * 256 + 1 one-byte jobs, byte-adjacent from an odd offset: with 2048
    workgroups of 256 threads every workgroup takes a second trip whatever the
    number of lanes a job gets (with G lanes per job, 2048 * 256 / G + 1 jobs
    are enough).  One keystream byte per job, from 64 sessions."""
    torch, d = dev
    rng = np.random.default_rng(63)
    nj, ns, nkeys = 2048 * 256 + 1, 64, 8
    keys = rng.integers(0, 256, (nkeys, 16), dtype=np.uint8)
    s_addr, s_fcnt = _distinct(rng, ns), _distinct(rng, ns)
    s_key, s_up = rng.integers(0, nkeys, ns), rng.integers(0, 2, ns)
    s_byte = np.array([cipher.block_s(keys[s_key[i]], bool(s_up[i]), int(s_addr[i]), int(s_fcnt[i]), 1)[0]
                       for i in range(ns)], np.uint8)
    who = rng.integers(0, ns, nj)
    jobs = np.zeros(nj, lphy.LORAWAN_DESC_DTYPE)
    jobs["offset"], jobs["len"] = 3 + np.arange(nj), 1
    jobs["devaddr"], jobs["fcnt"], jobs["key"], jobs["uplink"] = s_addr[who], s_fcnt[who], s_key[who], s_up[who]
    buf = rng.integers(0, 256, 3 + nj + 4, dtype=np.uint8)
    want = buf.copy()
    want[3:3 + nj] ^= s_byte[who]
    got, status = _crypt_batch(lphy, dev, buf, jobs, keys)
    assert not status.any()
    np.testing.assert_array_equal(got, want)


# -------------------------------------------------------------------- tx
def _tx_frames(lphy, rng, nkeys, fopts, payload):
    """LORAWAN_TX_DTYPE records over a source buffer with a few stray bytes
    between the frames' FOpts + FRMPayload (every alignment, and bytes no frame
    owns)."""
    nf = len(fopts)
    tx = np.zeros(nf, lphy.LORAWAN_TX_DTYPE)
    tx["fopts_len"], tx["payload_len"] = fopts, payload
    at, offs = 5, []
    for f in range(nf):
        offs.append(at)
        at += int(fopts[f]) + int(payload[f]) + int(rng.integers(0, 4))
    tx["src_offset"] = offs
    tx["devaddr"], tx["fcnt"] = _distinct(rng, nf), rng.integers(0, 65536, nf)
    tx["key"], tx["mtype"], tx["major"] = rng.integers(0, nkeys, nf), rng.integers(0, 8, nf), rng.integers(0, 4, nf)
    tx["fctrl"] = rng.integers(0, 256, nf)
    src = rng.integers(0, 256, at + 8, dtype=np.uint8)
    return tx, src


def _host_frame(oracle, cipher, t, src, nwk, app, skip):
    """MHDR .. MIC of record t as the LoRaWAN text builds it: the FRMPayload
    ciphered with the AppSKey (its first `skip` bytes clear), the MIC over the
    result with the NwkSKey.  Also the FOpts and the ciphered payload."""
    o, fol, pl = int(t["src_offset"]), int(t["fopts_len"]), int(t["payload_len"])
    uplink = (int(t["mtype"]) & 1) == 0
    fopts, plain = src[o:o + fol].tobytes(), src[o + fol:o + fol + pl]
    pay = plain.copy()
    pay[skip:] = cipher.crypt(app[t["key"]], uplink, int(t["devaddr"]), int(t["fcnt"]), plain[skip:].tobytes())
    body = (bytes([int(t["mtype"]) << 5 | int(t["major"]) & 3]) + int(t["devaddr"]).to_bytes(4, "little")
            + bytes([int(t["fctrl"]) & 0xF0 | fol]) + int(t["fcnt"]).to_bytes(2, "little") + fopts + pay.tobytes())
    mic = oracle.lorawan_mic(nwk[t["key"]], uplink, int(t["devaddr"]), int(t["fcnt"]), body)
    return np.frombuffer(body + mic.to_bytes(4, "little"), np.uint8), fopts, pay


@pytest.mark.parametrize("skip", [0, 1])
def test_tx_then_build_equals_build_frame_on_the_ciphered_payload(oracle, lphy, dev, cipher, skip):
    """40 frames at SF 7 (FOpts 0, 3, 15; FRMPayload 0, 1, 2, 16, 17, 40 bytes; up
    and down), different NwkSKey and AppSKey tables, and three frames both calls
    refuse.  d_bytes equals the reference's build_frame on the host-ciphered
    payload (where the reference was built) and the frame assembled from the
    LoRaWAN text with the oracle's MIC (always)."""
    from checkers import Reference, reference_available
    torch, d = dev
    rng = np.random.default_rng(64 + skip)
    nkeys = 6
    nwk, app = rng.integers(0, 256, (2, nkeys, 16), dtype=np.uint8)
    combos = [(fo, pl) for fo in (0, 3, 15) for pl in (0, 1, 2, 16, 17, 40)]
    good = combos * 2 + [(3, 40), (15, 17), (0, 16), (15, 40)]
    fopts, payload = [c[0] for c in good], [c[1] for c in good]
    # the refused ones, in the middle
    bad = {7: ("fopts16", EINVAL), 19: ("mtype8", EINVAL), 30: ("key", ENOKEY)}
    for f in sorted(bad):
        fopts.insert(f, 16 if bad[f][0] == "fopts16" else 3)
        payload.insert(f, 17)
    tx, src = _tx_frames(lphy, rng, nkeys, fopts, payload)
    for f, (what, _) in bad.items():
        if what == "mtype8":
            tx[f]["mtype"] = 8
        elif what == "key":
            tx[f]["key"] = nkeys
    nf = tx.size
    assert nf == 43 and (tx["mtype"] & 1).any() and not (tx["mtype"][tx["mtype"] < 8] & 1).all()
    desc = _table(lphy, 12 + tx["fopts_len"].astype(np.int64) + tx["payload_len"])
    nbytes = int(desc["sym_offset"][-1]) // 2
    t_src, t_tx = _up(dev, src), _up(dev, tx)
    t_cst = torch.full((nf,), 12345, dtype=torch.int32, device=d)
    t_bst = torch.full((nf,), 12345, dtype=torch.int32, device=d)
    t_bytes = torch.full((nbytes,), FILL, dtype=torch.uint8, device=d)
    st = torch.cuda.current_stream().cuda_stream
    lphy.lorawan_crypt_tx_ragged(t_src, t_tx, nf, _up(dev, app), skip=skip, status=t_cst, stream=st, src_bytes=src.size)
    lphy.lorawan_build_ragged(t_src, t_tx, _up(dev, desc), nf, N, _up(dev, nwk), t_bytes, t_bst, stream=st,
                              src_bytes=src.size, out_syms=2 * nbytes)
    torch.cuda.synchronize()
    got, got_src = t_bytes.cpu().numpy(), t_src.cpu().numpy()
    ref = Reference() if reference_available() else None
    want, want_src = np.full(nbytes, FILL, np.uint8), src.copy()
    for f in range(nf):
        if f in bad:
            assert t_cst[f].item() == bad[f][1] == t_bst[f].item(), f
            continue
        frame, fo, pay = _host_frame(oracle, cipher, tx[f], src, nwk, app, skip)
        if ref is not None:
            t = tx[f]
            r, _, tmp = ref.lorawan_build(nwk[t["key"]], int(t["mtype"]), int(t["major"]), int(t["devaddr"]),
                                          int(t["fctrl"]), int(t["fcnt"]), fo, pay.tobytes())
            assert r == 2 * frame.size and np.array_equal(tmp[:frame.size], frame), f
        o = int(desc["sym_offset"][f]) // 2
        want[o:o + frame.size] = frame
        so = int(tx[f]["src_offset"]) + int(tx[f]["fopts_len"])
        want_src[so:so + pay.size] = pay
        assert t_cst[f].item() == 0 and t_bst[f].item() == 2 * frame.size, f
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_src, want_src)     # FOpts, skipped bytes, strays and refused frames as they were


# ------------------------------------------------------------------ loop
@pytest.mark.parametrize("skip", [0, 1])
def test_loop_crypt_tx_build_tx_demod_parse_crypt_rx(lphy, dev, dm, cipher, skip):
    """The six calls on one table and one stream, no host read in between: 43
    frames at SF 7.  Every accepted frame's FRMPayload comes back as the
    plaintext, the rest of its row as build wrote it; three refused frames keep
    every byte of their rows."""
    torch, d = dev
    rng = np.random.default_rng(66 + skip)
    ndev = 8
    nwk, app = rng.integers(0, 256, (2, ndev, 16), dtype=np.uint8)
    addrs = np.sort(_distinct(rng, ndev))
    sessions = np.zeros(ndev, lphy.LORAWAN_SESSION_DTYPE)
    sessions["devaddr"], sessions["key"] = addrs, rng.permutation(ndev)
    assert lphy.lorawan_sessions_check(sessions)
    combos = [(fo, pl) for fo in (0, 3, 15) for pl in (0, 1, 2, 16, 17, 40)]
    good = combos * 2 + [(3, 40), (15, 17), (0, 16), (15, 40), (0, 40), (3, 17), (15, 16)]
    tx, src = _tx_frames(lphy, rng, ndev, [c[0] for c in good], [c[1] for c in good])
    nf = tx.size
    who = rng.integers(0, ndev, nf)
    who[sessions["key"][who] == ndev - 1] = int(np.flatnonzero(sessions["key"] != ndev - 1)[0])
    F_MIC, F_ADDR, F_KEY = 40, 41, 42               # the three refused frames (40 bytes of payload or more)
    who[F_KEY] = int(np.flatnonzero(sessions["key"] == ndev - 1)[0])   # its key is past the payload keys given to rx
    tx["devaddr"], tx["key"] = sessions["devaddr"][who], sessions["key"][who]
    tx["devaddr"][F_ADDR] = int(addrs[0]) ^ 0x00010000
    assert int(tx["devaddr"][F_ADDR]) not in set(addrs.tolist())
    desc = dm.lorawan_tx_layout(tx)
    n_iq, n_sym = int(desc["iq_offset"][-1]), int(desc["sym_offset"][-1])
    assert n_iq * 8 < 8 << 20
    step = dm.symbol_samples()
    offs = (desc["sym_offset"][:-1] // 2).astype(np.int64)
    L = 12 + tx["fopts_len"].astype(np.int64) + tx["payload_len"]
    st = torch.cuda.current_stream().cuda_stream
    t_desc, t_nwk, t_app = _up(dev, desc), _up(dev, nwk), _up(dev, app)
    t_src, t_tx, t_sess = _up(dev, src), _up(dev, tx), _up(dev, sessions)
    t_built = torch.zeros(n_sym // 2, dtype=torch.uint8, device=d)
    t_cst = torch.full((nf,), 12345, dtype=torch.int32, device=d)
    t_bst = torch.zeros(nf, dtype=torch.int32, device=d)
    t_iq = torch.zeros(2 * n_iq, dtype=torch.float32, device=d)
    t_syms = torch.zeros(n_sym, dtype=torch.int16, device=d)
    t_meta = torch.zeros(nf * 32, dtype=torch.uint8, device=d)
    t_pay = torch.zeros(n_sym // 2, dtype=torch.uint8, device=d)
    t_out = torch.zeros(nf * 32, dtype=torch.uint8, device=d)
    t_used = torch.zeros(nf, dtype=torch.int32, device=d)
    t_rst = torch.full((nf,), 12345, dtype=torch.int32, device=d)
    mode = lphy.MODE_DECHIRP_LORA_DEMODULATE
    lphy.lorawan_crypt_tx_ragged(t_src, t_tx, nf, t_app, skip=skip, status=t_cst, stream=st, src_bytes=src.size)
    lphy.lorawan_build_ragged(t_src, t_tx, t_desc, nf, step, t_nwk, t_built, t_bst, stream=st, src_bytes=src.size,
                              out_syms=n_sym)
    dm.tx_ragged(t_built, t_desc, nf, t_iq, stream=st, iq_samples=n_iq, out_syms=n_sym)
    dm.demod_ragged(t_iq, t_desc, nf, t_syms, t_meta, mode, lphy.F_DECODE, payload=t_pay, stream=st,
                    iq_samples=n_iq, out_syms=n_sym)
    t_pay[int(offs[F_MIC] + L[F_MIC]) - 2] ^= 0x20   # a MIC byte flipped after demodulation, on the same stream
    t_rows = t_pay.clone()
    lphy.lorawan_parse_ragged(t_pay, t_desc, nf, step, mode, t_nwk, t_out, meta=t_meta, sessions=t_sess,
                              key_used=t_used, stream=st, out_syms=n_sym)
    lphy.lorawan_crypt_rx_ragged(t_pay, t_desc, t_out, nf, step, mode, t_app[:16 * (ndev - 1)], key_used=t_used,
                                 skip=skip, status=t_rst, stream=st, out_syms=n_sym)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(t_cst.cpu().numpy(), 0)
    np.testing.assert_array_equal(t_bst.cpu().numpy(), 2 * L)
    recs = t_out.cpu().numpy().view(lphy.LORAWAN_FRAME_DTYPE)
    want_st = np.zeros(nf, np.int32)
    want_st[[F_MIC, F_ADDR, F_KEY]] = EINVAL, ENOKEY, ENOKEY
    assert int(recs["status"][F_MIC]) == EINVAL and int(recs["status"][F_ADDR]) == ENOKEY
    assert int(recs["status"][F_KEY]) == int(tx["payload_len"][F_KEY]) and t_used[F_KEY].item() == ndev - 1
    np.testing.assert_array_equal(t_rst.cpu().numpy(), want_st)
    built, rows, got = t_built.cpu().numpy(), t_rows.cpu().numpy(), t_pay.cpu().numpy()
    assert np.array_equal(np.flatnonzero(built != rows), [offs[F_MIC] + L[F_MIC] - 2])
    want = rows.copy()
    ciphered = 0
    for f in range(nf):
        if want_st[f]:
            continue
        assert int(recs["status"][f]) == int(tx["payload_len"][f])
        so = int(tx["src_offset"][f]) + int(tx["fopts_len"][f])
        po = int(offs[f]) + 8 + int(tx["fopts_len"][f])
        plain = src[so:so + int(tx["payload_len"][f])]
        want[po + skip:po + plain.size] = plain[skip:]
        # what was on air was not the plaintext (16 keystream bytes or more are not all zero)
        ciphered += plain.size >= 16 and not np.array_equal(built[po + skip:po + plain.size], plain[skip:])
    assert ciphered == sum(1 for f in range(nf) if not want_st[f] and tx["payload_len"][f] >= 16) > 20
    np.testing.assert_array_equal(got, want)     # header, FOpts, skipped byte, MIC and refused rows as they were


# ------------------------------------------------------- forged records
def test_forged_parse_records_cannot_leave_the_row(lphy, dev, cipher):
    """Records with status >= 0 that parse_ragged would not write: an extent one
    past the row, a payload in the header, a length of 2^32 - 1.  Each gets
    -EINVAL and the whole buffer, guards included, stays; a good record next to
    them is deciphered."""
    torch, d = dev
    rng = np.random.default_rng(68)
    keys = rng.integers(0, 256, (2, 16), dtype=np.uint8)
    row = 30
    offs = GUARD + 1 + np.arange(5) * row
    desc = _table(lphy, [row] * 5, byte_offsets=offs)
    rec = np.zeros(5, lphy.LORAWAN_FRAME_DTYPE)
    rec["devaddr"], rec["fcnt"], rec["mhdr"] = _distinct(rng, 5), rng.integers(0, 65536, 5), [0x40, 0x60, 0x80, 0xA0, 0x40]
    rec["payload_offset"] = [10, 10, 7, 8, 26]
    rec["payload_len"] = [16, 17, 5, 0xFFFFFFFF, 0]
    rec["status"] = [16, 17, 5, 3, 0]
    buf = rng.integers(0, 256, int(offs[-1]) + row + GUARD, dtype=np.uint8)
    t_buf = _up(dev, buf)
    t_status = torch.full((5,), 12345, dtype=torch.int32, device=d)
    lphy.lorawan_crypt_rx_ragged(t_buf, _up(dev, desc), _up(dev, rec), 5, N, 1, _up(dev, keys),
                                 key_used=_i32(dev, [1, 1, 1, 1, 1]), status=t_status, out_syms=2 * buf.size)
    torch.cuda.synchronize()
    assert t_status.cpu().tolist() == [0, EINVAL, EINVAL, EINVAL, 0]
    want = buf.copy()
    o = int(offs[0]) + 10
    want[o:o + 16] ^= cipher.keystream(keys[1], True, int(rec["devaddr"][0]), int(rec["fcnt"][0]), 16)
    np.testing.assert_array_equal(t_buf.cpu().numpy(), want)
    # without d_key_used: key 0
    t_buf = _up(dev, buf)
    lphy.lorawan_crypt_rx_ragged(t_buf, _up(dev, desc), _up(dev, rec), 5, N, 1, _up(dev, keys), status=t_status,
                                 out_syms=2 * buf.size)
    torch.cuda.synchronize()
    want = buf.copy()
    want[o:o + 16] ^= cipher.keystream(keys[0], True, int(rec["devaddr"][0]), int(rec["fcnt"][0]), 16)
    np.testing.assert_array_equal(t_buf.cpu().numpy(), want)
    assert t_status.cpu().tolist() == [0, EINVAL, EINVAL, EINVAL, 0]


# -------------------------------------------------------- argument errors
def test_call_level_return_codes(lphy, dev):
    """Every return code of the three device forms that comes before a launch."""
    torch, d = dev
    lib = lphy.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device=d)
    p = buf.data_ptr()
    assert p % 16 == 0
    big = 1 << 31

    def batch(data=p, desc=p, jobs=1, keys=p, nkeys=1, status=None):
        return lib.lphy_hip_lorawan_crypt_batch(data, desc, jobs, keys, nkeys, status, None)

    assert batch(jobs=0) == 0 and batch(jobs=0, data=None, desc=None, keys=None) == 0
    for kw in (dict(data=None), dict(desc=None), dict(keys=None), dict(nkeys=0), dict(keys=p + 8), dict(desc=p + 4)):
        assert batch(**kw) == EINVAL, kw
    assert batch(jobs=big) == ERANGE and batch(jobs=big + 5) == ERANGE

    def tx(src=p, rec=p, frames=1, keys=p, nkeys=1, skip=0, status=None):
        return lib.lphy_hip_lorawan_crypt_tx_ragged(src, rec, frames, keys, nkeys, skip, status, None)

    assert tx(frames=0) == 0 and tx(frames=0, src=None, rec=None, keys=None) == 0
    for kw in (dict(src=None), dict(rec=None), dict(keys=None), dict(nkeys=0), dict(keys=p + 4), dict(rec=p + 16 + 8),
               dict(skip=2), dict(skip=0xFFFFFFFF)):
        assert tx(**kw) == EINVAL, kw
    assert tx(frames=big) == ERANGE

    def rx(data=p, desc=p, parsed=p, used=None, frames=1, step=N, mode=1, keys=p, nkeys=1, skip=0, status=None):
        return lib.lphy_hip_lorawan_crypt_rx_ragged(data, desc, parsed, used, frames, step, mode, keys, nkeys, skip,
                                                    status, None)

    assert rx(frames=0) == 0 and rx(frames=0, data=None, desc=None, parsed=None, keys=None) == 0
    for kw in (dict(data=None), dict(desc=None), dict(parsed=None), dict(keys=None), dict(nkeys=0), dict(keys=p + 8),
               dict(parsed=p + 4), dict(skip=2), dict(step=0), dict(mode=3), dict(mode=-1)):
        assert rx(**kw) == EINVAL, kw
    assert rx(frames=big) == ERANGE
    torch.cuda.synchronize()
    assert not buf.any()        # nothing was launched


def test_host_form(lphy, cipher):
    rng = np.random.default_rng(69)
    key = rng.integers(0, 256, 16, dtype=np.uint8)
    for n, uplink in ((0, True), (1, False), (37, True), (4080, False)):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        got = lphy.lorawan_crypt(key, uplink, 0x01020304, 0x0A0B0C0D, data)
        assert got == cipher.crypt(key, uplink, 0x01020304, 0x0A0B0C0D, data).tobytes(), n
        assert lphy.lorawan_crypt(key, uplink, 0x01020304, 0x0A0B0C0D, got) == data
    lib = lphy.load()
    big = np.zeros(4081, np.uint8)
    assert lib.lphy_hip_lorawan_crypt_host(0, key.ctypes.data, 1, 1, 1, big.ctypes.data, 4081) == ERANGE
    assert not big.any()
    assert lib.lphy_hip_lorawan_crypt_host(0, None, 1, 1, 1, big.ctypes.data, 16) == EINVAL
    assert lib.lphy_hip_lorawan_crypt_host(0, key.ctypes.data, 1, 1, 1, None, 16) == EINVAL
    assert lib.lphy_hip_lorawan_crypt_host(1 << 20, key.ctypes.data, 1, 1, 1, big.ctypes.data, 16) == -19
    with pytest.raises(lphy.LphyError) as e:
        lphy.lorawan_crypt(key, True, 1, 1, bytes(4081))
    assert e.value.rc == ERANGE
