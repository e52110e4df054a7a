"""The true CRC verdict of the decode finalisation (csrc/lphy_final.h) in its
three forms and at its three call sites, on rows that carry a matching SX1272
checksum and rows that just miss one (tests/decode_cases.py), against the CPU
oracle row by row: bytes, crc_ok and status, and the call's count of
crc_ok == 1.  tests/test_decode_cases_cpu.py shows, without a device, which
form every case below reaches and that the oracle alone gives every case at
least a third of each verdict, so none of them passes on a constant flag.

The register form (finalize_frame_regs) with a checksum to compute is out of
reach of lphy_hip_decode_batch, lphy_hip_decode_host and k_post whatever the
arguments: those calls have sym_stride == nsyms and workgroups of kTile
threads, so a row of 4 k <= 32 bytes on aligned bases is taken by the block
form first, and a misaligned base misaligns every such row
(test_forced_rows_and_the_register_form_in_uniform_calls).  test_ragged_table
covers it: k_rg_final has no block form."""
import numpy as np
import pytest
import torch

import decode_cases as dc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
STATUS = -34      # the record of a row the call must leave alone
PAT = 0xA5        # payload bytes before the call
SYM_PAT = 0xEEEE  # symbol slots around the rows
GUARD = 64        # bytes on either side of a buffer's used range


@pytest.fixture(scope="module")
def dem(lphy):
    d = lphy.Demodulator(7)
    yield d
    d.close()


def _meta_in(lphy, status):
    """Records with every field set, so that a field the call should not
    touch shows when it does."""
    m = np.zeros(len(status), lphy.META_DTYPE)
    m["status"] = status
    m["cfo"], m["time_offset"], m["rate"], m["scale"], m["t_off"] = 1.5, -2.25, 0.125, 3.0, -7
    m["sw0"], m["sw1"], m["sync_word"], m["crc_ok"], m["normalised"], m["have_sync"] = 0x123, 0x456, 0x5A, 7, 1, 1
    return m


def _decode_batch(lphy, d, rows, status, s_off=0, b_off=0):
    """lphy_hip_decode_batch on slices of one allocation each: the symbols
    s_off bytes and the payload b_off bytes past a 16-byte boundary, GUARD
    bytes of pattern on either side.  -> (payload [frames, nb], records out,
    records in); the guards and the symbols are checked here."""
    frames, per = rows.shape
    nb, g = per // 2, GUARD // 2
    a = np.full(g + s_off // 2 + frames * per + g, SYM_PAT, np.uint16)
    a[g + s_off // 2: g + s_off // 2 + frames * per] = rows.reshape(-1)
    t_all = torch.from_numpy(a.view(np.int16).copy()).to(DEV)
    t_syms = t_all[g + s_off // 2: g + s_off // 2 + frames * per]
    t_pall = torch.full((GUARD + b_off + frames * nb + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    t_pay = t_pall[GUARD + b_off: GUARD + b_off + frames * nb]
    assert t_syms.data_ptr() % 16 == s_off and t_pay.data_ptr() % 16 == b_off
    m_in = _meta_in(lphy, status)
    t_meta = torch.from_numpy(m_in.view(np.uint8).copy()).to(DEV)
    d.decode_batch(t_syms, frames, per, t_pay, t_meta, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pall = t_pall.cpu().numpy()
    assert (pall[: GUARD + b_off] == PAT).all() and (pall[GUARD + b_off + frames * nb:] == PAT).all(), "payload guards"
    np.testing.assert_array_equal(t_all.cpu().numpy().view(np.uint16), a, err_msg="the symbols are read only")
    pay = pall[GUARD + b_off: GUARD + b_off + frames * nb].reshape(frames, nb)
    return pay, t_meta.cpu().numpy().view(lphy.META_DTYPE), m_in


def _check(pay, meta, m_in, want):
    """Every row against oracle.decode; rows of a non-zero status untouched;
    nothing of a record but crc_ok changes."""
    wp, wc = want
    skip = m_in["status"] != 0
    assert (pay[skip] == PAT).all(), "a row of a non-zero status was written"
    assert meta[skip].tobytes() == m_in[skip].tobytes(), "a record of a non-zero status was written"
    np.testing.assert_array_equal(pay[~skip], wp[~skip])
    bad = np.flatnonzero(meta["crc_ok"][~skip] != wc[~skip])
    assert bad.size == 0, f"crc_ok differs from the oracle at decoded rows {bad[:8]} ({bad.size} rows)"
    assert (meta["status"][~skip] == 0).all()
    assert int((meta["crc_ok"][~skip] == 1).sum()) == int(wc[~skip].sum())
    rest = meta.copy()
    rest["crc_ok"] = m_in["crc_ok"]
    assert rest.tobytes() == m_in.tobytes(), "a field other than crc_ok changed"


def _uniform(oracle, lphy, d, nb, frames):
    if frames == 1:  # once per row of the kind cycle, then once with a status to respect
        rows = dc.single_rows(oracle, nb)
        want = dc.expected(oracle, rows, ("single", nb))
        for i in range(len(rows)):
            _check(*_decode_batch(lphy, d, rows[i:i + 1], np.zeros(1, np.int32)), (want[0][i:i + 1], want[1][i:i + 1]))
        _check(*_decode_batch(lphy, d, rows[:1], np.full(1, STATUS, np.int32)), (want[0][:1], want[1][:1]))
        return
    rows = dc.batch_rows(oracle, nb, frames)
    status = np.where(dc.skipped(frames), STATUS, 0).astype(np.int32)
    _check(*_decode_batch(lphy, d, rows, status), dc.expected(oracle, rows, ("batch", nb, frames)))


@pytest.mark.parametrize("nb,frames", dc.BLOCK_CASES)
def test_decode_batch_block_form(oracle, lphy, dem, nb, frames):
    """finalize_block behind k_finalize: rows of 4 to 32 bytes, kinds
    interleaved, every third row with a status to respect; 255, 256, 257 and
    513 rows: a partial last workgroup and one exactly full."""
    _uniform(oracle, lphy, dem, nb, frames)


@pytest.mark.parametrize("nb,frames", dc.MEMORY_CASES)
def test_decode_batch_memory_form(oracle, lphy, dem, nb, frames):
    """The memory form (the only one that calls sx1272_checksum): the scalar
    tail alone at 5, 6, 7 bytes, rows just past the register limit, long rows;
    rows of both alignments where nb is no multiple of 4."""
    _uniform(oracle, lphy, dem, nb, frames)


@pytest.mark.parametrize("kind", dc.HUGE_KINDS)
def test_decode_batch_longest_row(oracle, lphy, dem, kind):
    """One row of 65,534 bytes: the checksum's int length of 65,530."""
    rows = dc.row(oracle, dc.NB_HUGE, kind)[None, :]
    pay, meta, m_in = _decode_batch(lphy, dem, rows, np.zeros(1, np.int32))
    _check(pay, meta, m_in, dc.expected(oracle, rows))
    assert meta["crc_ok"][0] == (kind == "valid")


@pytest.mark.parametrize("nb", dc.NB_FORCED[1:])
def test_decode_batch_rows_below_four_bytes(oracle, lphy, dem, nb):
    """No checksum fits: crc_ok is written 0 (over the 7 the records hold).
    (Rows of 0 bytes have no buffer to pass here; test_ragged_table has them.)"""
    rows = dc.batch_rows(oracle, nb, dc.FORCED_FRAMES)
    status = np.where(dc.skipped(dc.FORCED_FRAMES), STATUS, 0).astype(np.int32)
    pay, meta, m_in = _decode_batch(lphy, dem, rows, status)
    _check(pay, meta, m_in, dc.expected(oracle, rows))
    assert (meta["crc_ok"][status == 0] == 0).all()


@pytest.mark.parametrize("nb", dc.BLOCK_NB)
def test_decode_batch_misaligned_bases(oracle, lphy, dem, nb):
    """d_syms 2 and 8 bytes, d_bytes 1 and 2 bytes off their alignment: the
    call silently leaves the block form for the memory form's scalar loop
    (test_misaligned_bases_switch_the_form) and must give the aligned call's
    results, inside its own range."""
    frames = dc.MISALIGNED_FRAMES
    rows = dc.batch_rows(oracle, nb, frames)
    status = np.where(dc.skipped(frames), STATUS, 0).astype(np.int32)
    want = dc.expected(oracle, rows, ("batch", nb, frames))
    pay0, meta0, m_in = _decode_batch(lphy, dem, rows, status)
    _check(pay0, meta0, m_in, want)
    for s_off, b_off in dc.MISALIGNED:
        pay, meta, _ = _decode_batch(lphy, dem, rows, status, s_off, b_off)
        _check(pay, meta, m_in, want)
        np.testing.assert_array_equal(pay, pay0, err_msg=f"offsets {s_off}, {b_off}")
        assert meta.tobytes() == meta0.tobytes(), (s_off, b_off)


@pytest.mark.parametrize("nb", dc.HOST_NB)
def test_decode_host(oracle, lphy, dem, nb):
    got = []
    for kind in dc.HOST_KINDS:
        r = dc.row(oracle, nb, kind)
        rc, out, meta = dem.decode_host(r)
        n, obytes, ocrc = oracle.decode(r)
        assert rc == 0 and n == nb
        np.testing.assert_array_equal(out, obytes)
        assert meta["crc_ok"] == ocrc and meta["status"] == 0, kind
        got.append(int(meta["crc_ok"]))
    assert got == [1, 0]


# ---- k_post: the finalisation after the demodulator kernels ----------------
@pytest.mark.parametrize("sf,mode,frames,nb,form", dc.POST_CASES)
def test_post_finalisation(oracle, lphy, sf, mode, frames, nb, form):
    """lphy_hip_demod_host with LPHY_F_DECODE on clean frames of the table's
    rows: after the fused kernel (fused_min_frames 0, units spanning frames at
    SF 7), after the library's own launch choice and after the separate
    launches.  Symbols, sync word, bytes, crc_ok and status against the
    oracle's chain on the same IQ; in mode 2 the symbols are the rows."""
    iq, (syms, sync, pay, crc) = dc.post_case(oracle, sf, mode, frames, nb)
    d = lphy.Demodulator(sf)
    for fused_min, flags in ((0, 0), (-1, 0), (-1, lphy.F_UNFUSED)):
        what = f"fused_min_frames {fused_min}, flags {flags}"
        d.set_fused_min_frames(fused_min)
        gs, gp, meta = d.demod_host(iq, frames, iq.shape[1], mode, lphy.F_DECODE | flags)
        np.testing.assert_array_equal(gs, syms, err_msg=what)
        np.testing.assert_array_equal(meta["sync_word"], sync, err_msg=what)
        np.testing.assert_array_equal(gp, pay, err_msg=what)
        np.testing.assert_array_equal(meta["crc_ok"], crc, err_msg=what)
        assert (meta["status"] == 0).all(), what
        assert int((meta["crc_ok"] == 1).sum()) == int(crc.sum()), what
    d.close()


# ---- the ragged call site ---------------------------------------------------
@pytest.mark.parametrize("mode", dc.RAGGED_MODES)
def test_ragged_table(oracle, lphy, mode):
    """lphy_hip_demod_ragged with LPHY_F_DECODE on lphy_hip_tx_layout's table of
    0 to 36-byte frames, its records shuffled (unit_offset again the prefix in
    record order): k_rg_final takes rows of 4, 8, 12 and 32 bytes in registers
    where their symbols start on 16 bytes and from memory elsewhere, and both
    occur (test_ragged_table_reaches_the_register_form_at_both_alignments)."""
    sf = dc.RAGGED_SF
    lens = dc.ragged_lens()
    frames = len(lens)
    iq, want = dc.ragged_case(oracle, mode)
    d = lphy.Demodulator(sf)
    desc = d.tx_layout(lens)
    offs = dc.ragged_sym_offsets(lens)
    assert list(desc["sym_offset"][:-1]) == offs
    assert list(desc["iq_offset"][:-1]) == list(np.cumsum([0] + [x.size for x in iq[:-1]]))
    order = dc.ragged_order()
    table = desc.copy()
    table[:frames] = desc[order]
    total = table["samples"][:frames] >> np.uint64(sf)
    table["unit_offset"][:frames] = np.concatenate([[0], np.cumsum(total)[:-1]]).astype(np.uint64)
    assert table["unit_offset"][frames] == total.sum()
    n_iq, n_out = d._ragged_extent(table, mode)
    assert n_out == 2 * sum(lens)
    t_iq = torch.from_numpy(np.concatenate(iq).view(np.float32).copy()).to(DEV)
    t_desc = torch.from_numpy(table.view(np.uint8).copy()).to(DEV)
    t_syms = torch.full((n_out + GUARD,), SYM_PAT - 65536, dtype=torch.int16, device=DEV)
    t_pay = torch.full((n_out // 2 + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    t_meta = torch.zeros(frames * 32, dtype=torch.uint8, device=DEV)
    assert t_syms.data_ptr() % 16 == 0 and t_pay.data_ptr() % 4 == 0
    d.demod_ragged(t_iq, t_desc, frames, t_syms, t_meta, mode, lphy.F_DECODE, payload=t_pay,
                   stream=torch.cuda.current_stream().cuda_stream, iq_samples=n_iq, out_syms=n_out)
    torch.cuda.synchronize()
    syms = t_syms.cpu().numpy().view(np.uint16)
    pay = t_pay.cpu().numpy()
    meta = t_meta.cpu().numpy().view(lphy.META_DTYPE)
    assert (syms[n_out:] == SYM_PAT).all() and (pay[n_out // 2:] == PAT).all()
    ones = 0
    for k, a in enumerate(order):
        nb, off = lens[a], offs[a]
        wsyms, wsync, wpay, wcrc = want[a]
        what = f"record {k}: frame {a} of {nb} bytes at symbol {off}, {dc.ragged_form(nb, off)} form"
        np.testing.assert_array_equal(syms[off: off + 2 * nb], wsyms, err_msg=what)
        np.testing.assert_array_equal(pay[off // 2: off // 2 + nb], wpay, err_msg=what)
        assert meta["status"][k] == 0 and meta["sync_word"][k] == wsync, what
        assert meta["crc_ok"][k] == wcrc, what
        ones += wcrc
    assert int((meta["crc_ok"] == 1).sum()) == ones
    d.close()
