"""The decode case table (tests/decode_cases.py) on the CPU oracle alone:
every case's verdict is what its kind promises, every GPU case of
tests/test_gpu_decode.py reaches the form it is named after (by the
predicates read off csrc/lphy_final.h), and every GPU case's rows are, by the
oracle, at least one third crc_ok == 1 and one third crc_ok == 0: no GPU test
can pass on a flag that is always 0 or always 1."""
import numpy as np
import pytest

import decode_cases as dc


def _thirds(crc, what):
    ones, n = int(np.sum(crc)), len(crc)
    assert 3 * ones >= n and 3 * (n - ones) >= n, f"{what}: {ones} of {n} rows verify"


@pytest.mark.parametrize("nb", dc.NB_TABLE + (dc.NB_HUGE,))
def test_verdicts_are_what_the_kinds_promise(oracle, nb):
    for variant in (0, 1, 7):
        valid = dc.row(oracle, nb, "valid", variant)
        for kind in dc.kinds_for(nb):
            r = dc.row(oracle, nb, kind, variant)
            n, out, crc = oracle.decode(r)
            assert n == nb and r.size == 2 * nb
            want = dc.promised(nb, kind)
            if want is None:
                want = dc.CORRECTED_VERDICT[nb]
            assert crc == want, (nb, kind, variant)
            if kind == "valid" or (kind == "junk_high" and nb):
                assert out.tobytes() == dc.payload_of(oracle, nb, "valid", variant)
            if kind == "junk_high" and nb:
                assert (r >> 8).any() and np.array_equal(r & 0xFF, valid)
            if kind in ("payload_off", "crc_off"):  # one payload bit away from the valid row
                diff = np.frombuffer(out.tobytes(), np.uint8) ^ np.frombuffer(
                    dc.payload_of(oracle, nb, "valid", variant), np.uint8)
                assert sum(bin(int(x)).count("1") for x in diff) == 1
                where = int(np.flatnonzero(diff)[0])
                assert (2 <= where < nb - 2) if kind == "payload_off" else (where >= nb - 2)
            if kind == "corrected":
                x = r ^ valid
                hit = sorted(set(np.flatnonzero(x) // 2))
                assert hit == dc.corrected_bytes(nb)
                assert all(bin(int(v)).count("1") == 1 and v < 256 for v in x[x != 0])
                assert np.count_nonzero(x) == 2 * len(hit)


def test_every_length_class_has_a_corrected_row_that_verifies():
    for name, nbs in dc.LENGTH_CLASSES.items():
        assert any(dc.CORRECTED_VERDICT[nb] == 1 for nb in nbs), name


def test_byte_counts_are_the_branch_points():
    assert dc.NB_TABLE == (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 28, 32, 33, 34, 35, 36, 64, 255, 1024)
    assert set(dc.BLOCK_NB + dc.MEMORY_NB + dc.NB_FORCED) == set(dc.NB_TABLE)  # decode_batch runs them all
    assert [n for nb, n in dc.BLOCK_CASES if nb == 4] == [1, 255, 256, 257, 513]
    assert dc.memory_counts(64) == [1, 255, 256, 257, 513] and dc.memory_counts(255) == [1, 255, 256, 257]
    assert dc.memory_counts(1024) == [1, 64]


# ---- the forms ------------------------------------------------------------
@pytest.mark.parametrize("nb,frames", dc.BLOCK_CASES)
def test_block_case_reaches_the_block_form(nb, frames):
    assert dc.batch_forms(nb, frames) == {"block"}


@pytest.mark.parametrize("nb,frames", dc.MEMORY_CASES)
def test_memory_case_reaches_the_memory_form(nb, frames):
    assert dc.batch_forms(nb, frames) == {"memory"}
    vec = {dc.memory_vector(nb, 0, 0, f) for f in range(frames)}
    if nb in (36, 64, 1024):
        assert vec == {True}       # every row starts aligned: 16-byte loads
    elif frames > 16:
        assert vec == {True, False}  # rows of both alignments
    assert dc.form_of(2 * dc.NB_HUGE, 2 * dc.NB_HUGE) == "memory"


def test_forced_rows_and_the_register_form_in_uniform_calls():
    """In a uniform call (sym_stride == nsyms, a workgroup of kTile threads)
    a row that passes finalize_frame_regs' test with 4 <= nb passes
    finalize_block's first, and a misaligned base misaligns every row of 4 k
    bytes: over every nb to 40, every base alignment and 64 rows, the
    register form takes only empty rows (nb == 0, crc_ok = 0).  So
    lphy_hip_decode_batch, lphy_hip_decode_host and k_post never reach its
    checksum; the ragged call site does (k_rg_final has no block form)."""
    seen = set()
    for nb in range(0, 41):
        for s16 in range(0, 16, 2):
            for b4 in range(4):
                for f in range(64):
                    if dc.form_of(2 * nb, 2 * nb, s16, b4, dc.TILE, f) == "regs":
                        seen.add(nb)
    assert seen == {0}
    assert dc.batch_forms(0, dc.FORCED_FRAMES) == {"regs"}
    for nb in (1, 2, 3):
        assert dc.batch_forms(nb, dc.FORCED_FRAMES) == {"memory"}


@pytest.mark.parametrize("nb", dc.BLOCK_NB)
def test_misaligned_bases_switch_the_form(nb):
    """Which form each offset of d_syms / d_bytes selects: the aligned call
    takes the block form, every misaligned one the memory form, with its
    scalar loop alone (neither pointer of any row is aligned)."""
    assert dc.batch_forms(nb, dc.MISALIGNED_FRAMES, 0, 0) == {"block"}
    for s, b in dc.MISALIGNED:
        assert dc.batch_forms(nb, dc.MISALIGNED_FRAMES, s, b) == {"memory"}, (s, b)
        assert not any(dc.memory_vector(nb, s, b, f) for f in range(dc.MISALIGNED_FRAMES))
    assert sorted(dc.MISALIGNED) == [(0, 1), (0, 2), (2, 0), (2, 1), (2, 2), (8, 0), (8, 1), (8, 2)]


@pytest.mark.parametrize("nb", dc.HOST_NB)
def test_host_case_forms(nb):
    """lphy_hip_decode_host stages its buffers on 256-byte boundaries
    (csrc/lphy_stage_plan.h align_up), one row."""
    assert dc.batch_forms(nb, 1) == ({"block"} if nb in (4, 32) else {"memory"})


@pytest.mark.parametrize("sf,mode,frames,nb,form", dc.POST_CASES)
def test_post_case_reaches_its_form(sf, mode, frames, nb, form):
    """k_post on lphy_hip_demod_host's staged (256-byte-aligned) buffers:
    sym_stride == nsyms == 2 nb."""
    assert dc.batch_forms(nb, frames) == {form}


def test_ragged_table_reaches_the_register_form_at_both_alignments():
    lens = dc.ragged_lens()
    assert set(lens) == set(dc.RAGGED_SET)
    offs = dc.ragged_sym_offsets(lens)
    forms = {}
    for nb, o in zip(lens, offs):
        assert o % 2 == 0
        forms.setdefault(nb, set()).add((dc.ragged_form(nb, o), o % 8 == 0))
    for nb in (4, 8, 12, 32):  # 16-byte-aligned rows in registers, the others from memory
        assert forms[nb] == {("regs", True), ("memory", False)}, nb
    assert forms[0] == {("regs", True), ("memory", False)}
    assert forms[36] == {("memory", True), ("memory", False)}
    for nb in (1, 3, 5, 9, 33):
        assert {f for f, _ in forms[nb]} == {"memory"}
    order = dc.ragged_order()
    assert sorted(order) == list(range(len(lens))) and list(order) != sorted(order)


def test_ragged_slots_see_every_kind(oracle):
    """Each (length, alignment) slot of the pass takes all of its kinds over
    the passes, so the register form gives both verdicts at every length."""
    lens, rows = dc.ragged_lens(), dc.ragged_rows(oracle)
    offs = dc.ragged_sym_offsets(lens)
    seen = {}
    for nb, o, r in zip(lens, offs, rows):
        if nb >= 4:
            seen.setdefault((nb, dc.ragged_form(nb, o)), set()).add(oracle.decode(r)[2])
    for key, verdicts in seen.items():
        assert verdicts == {0, 1}, key
    assert {k for k in seen if k[1] == "regs"} == {(nb, "regs") for nb in (4, 8, 12, 32)}


# ---- both verdicts in every GPU case ---------------------------------------
@pytest.mark.parametrize("nb,frames", dc.BLOCK_CASES + dc.MEMORY_CASES)
def test_decode_batch_case_has_both_verdicts(oracle, nb, frames):
    if frames == 1:
        crc = dc.expected(oracle, dc.single_rows(oracle, nb))[1]
    else:
        rows = dc.batch_rows(oracle, nb, frames)
        crc = dc.expected(oracle, rows)[1][~dc.skipped(frames)]
    _thirds(crc, f"nb {nb} x {frames}")


def test_misaligned_host_and_long_cases_have_both_verdicts(oracle):
    for nb in dc.BLOCK_NB:
        rows = dc.batch_rows(oracle, nb, dc.MISALIGNED_FRAMES)
        _thirds(dc.expected(oracle, rows)[1][~dc.skipped(dc.MISALIGNED_FRAMES)], f"misaligned nb {nb}")
    for nb in dc.HOST_NB:
        assert [oracle.decode(dc.row(oracle, nb, k))[2] for k in dc.HOST_KINDS] == [1, 0]
    assert [oracle.decode(dc.row(oracle, dc.NB_HUGE, k))[2] for k in dc.HUGE_KINDS] == [1, 0]


@pytest.mark.parametrize("sf,mode,frames,nb,form", dc.POST_CASES)
def test_post_case_verdicts(oracle, sf, mode, frames, nb, form):
    """Mode 2: the oracle's chain returns the rows' low sf bits, sync word
    0x12, and both verdicts in thirds.  Mode 0: the estimate over a clean
    frame's two sync symbols moves every symbol (decode_cases.POST_SHAPES), so
    the chain's symbols are not the rows; those cases compare with the chain
    as it is."""
    iq, (syms, sync, pay, crc) = dc.post_case(oracle, sf, mode, frames, nb)
    rows = dc.fed(dc.batch_rows(oracle, nb, frames), sf)
    assert iq.shape == (frames, (2 * nb + 2) << sf) and syms.shape == rows.shape
    if mode == 2:
        np.testing.assert_array_equal(syms, rows)
        assert (sync == 0x12).all()
        np.testing.assert_array_equal(crc, dc.expected(oracle, rows)[1])
        _thirds(crc, f"SF{sf} mode 2 nb {nb}")
    else:
        assert (syms != rows).mean() > 0.9
        _, (_, _, _, crc2) = dc.post_case(oracle, sf, 2, frames, nb)
        _thirds(crc2, f"SF{sf} nb {nb}: the mode 2 case on the same IQ")


def test_ragged_table_verdicts(oracle):
    lens = dc.ragged_lens()
    rows = dc.ragged_rows(oracle)
    iq, got = dc.ragged_case(oracle, 2)
    for nb, r, x, (syms, sync, pay, crc) in zip(lens, rows, iq, got):
        assert x.size == (2 * nb + 2) << dc.RAGGED_SF
        np.testing.assert_array_equal(syms, dc.fed(r, dc.RAGGED_SF))
        assert sync == 0x12 and crc == oracle.decode(r)[2]   # SF 8 carries the whole code word
    _thirds([g[3] for g in got], "ragged, mode 2")
    _, got0 = dc.ragged_case(oracle, 0)
    assert all(g[0].size == 2 * nb for nb, g in zip(lens, got0))
