"""The decode finalisation's case table (csrc/lphy_final.h), importable without
a GPU: rows of symbols built from payloads that do or do not carry a matching
SX1272 checksum, the byte counts at the code's branch points, the batches the
GPU tests of tests/test_gpu_decode.py run, and the three form predicates
restated in plain Python.  tests/test_decode_cases_cpu.py checks the table on
the oracle alone; tests/test_oracle_vs_reference.py pins the oracle's decode
to the reference build on it.

A uniformly random row matches its checksum with probability 2^-16, so only
rows built here make crc_ok == 1 appear."""
from __future__ import annotations

import numpy as np

KINDS = ("valid", "payload_off", "crc_off", "corrected", "junk_high")

# byte counts by the code's branch points (lphy_final.h)
NB_FORCED = (0, 1, 2, 3)               # crc_ok forced to 0 (:95, :111-113, :156-161)
NB_EMPTY = (4,)                        # a checksum over zero bytes
NB_TAIL = (5, 6, 7)                    # memory form, scalar tail only
NB_REGS = (8, 12, 16, 24, 28, 32)      # register / block forms; 28, 32: the unrolled loop's last steps
NB_PAST = (33, 34, 35, 36)             # just past the register limit; 36 a multiple of 4
NB_LONG = (64, 255, 1024)
NB_HUGE = 65534                        # one row, single-row calls only
NB_TABLE = NB_FORCED + NB_EMPTY + NB_TAIL + NB_REGS + NB_PAST + NB_LONG   # all but NB_HUGE
LENGTH_CLASSES = {"empty": NB_EMPTY, "tail": NB_TAIL, "regs": NB_REGS, "past": NB_PAST, "long": NB_LONG}

# the oracle's verdict on the `corrected` rows as built (every variant),
# recorded; the CPU test holds the oracle to it.  Every flip is a single bit
# in its code word, which Hamming(8,4) repairs or, in a parity bit, ignores.
CORRECTED_VERDICT = {nb: 1 for nb in NB_TABLE + (NB_HUGE,) if nb >= 4}


def kinds_for(nb: int):
    """The kinds a row of nb bytes can have: below 4 bytes there is no checksum
    (the payload is random; every verdict is 0), and at 4 the checksummed body
    payload[2:2] has no bit to flip."""
    if nb < 4:
        return ("valid", "junk_high")
    if nb == 4:
        return ("valid", "crc_off", "corrected", "junk_high")
    return KINDS


def kind_cycle(nb: int):
    """The kinds of a batch's rows in turn, five long so that the rows of a
    non-zero status (every third) take every kind: three kinds of verdict 1
    and two of verdict 0."""
    if nb < 4:
        return ("valid", "junk_high", "valid", "junk_high", "valid")
    if nb == 4:
        return ("valid", "crc_off", "corrected", "crc_off", "junk_high")
    return ("valid", "payload_off", "corrected", "crc_off", "junk_high")


def promised(nb: int, kind: str):
    """crc_ok the kind promises; None where the oracle alone decides."""
    if nb < 4:
        return 0
    return {"valid": 1, "junk_high": 1, "payload_off": 0, "crc_off": 0, "corrected": None}[kind]


def payload_of(oracle, nb: int, kind: str = "valid", variant: int = 0) -> bytes:
    """The payload a row encodes: random bytes whose last two are
    sx_checksum(payload[2:nb-2]), low byte first (as
    tests/golden/make_golden.py:crc_payload), then the kind's bit flip."""
    assert kind in kinds_for(nb), (nb, kind)
    rng = np.random.default_rng([nb, variant])
    p = bytearray(rng.integers(0, 256, nb, dtype=np.uint8).tobytes())
    if nb >= 4:
        c = oracle.sx_checksum(bytes(p[2:nb - 2]))
        p[nb - 2], p[nb - 1] = c & 0xFF, c >> 8
    flip = np.random.default_rng([nb, variant, 1])
    if kind == "payload_off":
        p[2 + int(flip.integers(0, nb - 4))] ^= 1 << int(flip.integers(0, 8))
    elif kind == "crc_off":
        p[nb - 2 + int(flip.integers(0, 2))] ^= 1 << int(flip.integers(0, 8))
    return bytes(p)


def corrected_bytes(nb: int):
    """The bytes whose code words `corrected` flips: the first and the last
    byte of the checksummed body and the two checksum bytes."""
    body = [2, nb - 3] if nb > 4 else []
    return sorted(set(body + [nb - 2, nb - 1]))


_ROWS = {}


def row(oracle, nb: int, kind: str, variant: int = 0) -> np.ndarray:
    """2 nb symbols (uint16, read-only) of one case; built once."""
    key = (nb, kind, variant)
    if key not in _ROWS:
        base = "valid" if kind in ("corrected", "junk_high") else kind
        r = oracle.encode(payload_of(oracle, nb, base, variant)).copy()
        rng = np.random.default_rng([nb, variant, 2])
        if kind == "corrected":
            for b in corrected_bytes(nb):  # one bit in each of the byte's two code words
                r[2 * b] ^= np.uint16(1 << int(rng.integers(0, 8)))
                r[2 * b + 1] ^= np.uint16(1 << int(rng.integers(0, 8)))
        elif kind == "junk_high":
            r |= rng.integers(0, 256, r.size, dtype=np.uint16) << np.uint16(8)
        r.setflags(write=False)
        _ROWS[key] = r
    return _ROWS[key]


def batch_rows(oracle, nb: int, frames: int, start: int = 0) -> np.ndarray:
    """frames rows of nb bytes, kinds interleaved by kind_cycle from `start`;
    the variant changes with every turn of the cycle.  [frames, 2 nb] uint16."""
    cyc = kind_cycle(nb)
    out = np.zeros((frames, 2 * nb), np.uint16)
    for f in range(frames):
        out[f] = row(oracle, nb, cyc[(f + start) % 5], (f + start) // 5)
    return out


def skipped(frames: int) -> np.ndarray:
    """The rows of a decode_batch call that carry a non-zero status."""
    return np.arange(frames) % 3 == 2


_WANT = {}


def expected(oracle, rows: np.ndarray, key=None):
    """oracle.decode of every row -> (bytes [frames, nb], crc_ok [frames]);
    kept under `key` when given, and read-only."""
    if key is not None and key in _WANT:
        return _WANT[key]
    nb = rows.shape[1] // 2
    pay = np.zeros((rows.shape[0], nb), np.uint8)
    crc = np.zeros(rows.shape[0], np.uint8)
    for f, r in enumerate(rows):
        n, b, c = oracle.decode(r)
        assert n == nb
        pay[f], crc[f] = b, c
    pay.setflags(write=False)
    crc.setflags(write=False)
    if key is not None:
        _WANT[key] = (pay, crc)
    return pay, crc


# ---------------------------------------------------------------------------
# The three forms, restated from csrc/lphy_final.h.  Addresses enter as the
# base pointers modulo 16 (symbols) and modulo 4 (bytes); row f starts at
# syms + f * sym_stride symbols and bytes + f * nb.
# ---------------------------------------------------------------------------
TILE = 256  # kTile (csrc/lphy_fft.h)


def block_form(nsyms, sym_stride, syms_mod16, bytes_mod4, block_dim=TILE, decode=True) -> bool:
    """finalize_block's test, lphy_final.h:180-183 (f0 >= frames aside: such a
    workgroup has no row), behind k_finalize's blockDim.x == kTile
    (lphy_hip.hip:163); k_post always runs kTile threads.  block_dim None: a
    call site without the block form (k_rg_final, lphy_ragged.h:329)."""
    nb = nsyms // 2
    return bool(block_dim == TILE and decode and nsyms % 2 == 0 and 4 <= nb <= 32 and nb % 4 == 0
                and sym_stride % 8 == 0 and syms_mod16 % 16 == 0 and bytes_mod4 % 4 == 0)


def regs_form(nsyms, sym_stride, syms_mod16, bytes_mod4, f=0, decode=True) -> bool:
    """finalize_frame_regs' test on row f, lphy_final.h:67-68."""
    nb = nsyms // 2
    return bool(decode and nsyms % 2 == 0 and nb <= 32 and nb % 4 == 0
                and (syms_mod16 + 2 * f * sym_stride) % 16 == 0 and (bytes_mod4 + f * nb) % 4 == 0)


def form_of(nsyms, sym_stride, syms_mod16=0, bytes_mod4=0, block_dim=TILE, f=0) -> str:
    """The form row f takes: block, else regs, else memory (the rest of
    finalize_frame, lphy_final.h:122-164)."""
    if block_form(nsyms, sym_stride, syms_mod16, bytes_mod4, block_dim):
        return "block"
    return "regs" if regs_form(nsyms, sym_stride, syms_mod16, bytes_mod4, f) else "memory"


def batch_forms(nb, frames, syms_mod16=0, bytes_mod4=0, block_dim=TILE):
    """The forms the rows of a uniform call take (sym_stride == nsyms)."""
    return {form_of(2 * nb, 2 * nb, syms_mod16, bytes_mod4, block_dim, f) for f in range(frames)}


def memory_vector(nb, syms_mod16, bytes_mod4, f=0) -> bool:
    """The memory form's 16-byte loads run on row f (lphy_final.h:136), else
    the scalar loop takes the whole row."""
    return (syms_mod16 + 4 * f * nb) % 16 == 0 and (bytes_mod4 + f * nb) % 4 == 0 and nb >= 4


# ---------------------------------------------------------------------------
# The GPU tests' cases (tests/test_gpu_decode.py)
# ---------------------------------------------------------------------------
FRAME_COUNTS = (1, 255, 256, 257, 513)   # a partial last workgroup, and one exactly full
BLOCK_NB = (4, 8, 12, 16, 24, 28, 32)
MEMORY_NB = (5, 6, 7, 33, 34, 35, 36, 64, 255, 1024)
BLOCK_CASES = [(nb, n) for nb in BLOCK_NB for n in FRAME_COUNTS]


def memory_counts(nb):
    """FRAME_COUNTS capped at 64 KiB of payload per call."""
    return sorted({min(n, 65536 // nb) for n in FRAME_COUNTS})


MEMORY_CASES = [(nb, n) for nb in MEMORY_NB for n in memory_counts(nb)]
MISALIGNED = [(s, b) for s in (0, 2, 8) for b in (0, 1, 2) if s or b]   # d_syms, d_bytes offsets in bytes
MISALIGNED_FRAMES = 257
HOST_NB = (4, 32, 33, 1024)
HOST_KINDS = ("valid", "crc_off")
HUGE_KINDS = ("valid", "payload_off")
FORCED_FRAMES = 5


def single_rows(oracle, nb):
    """A one-row call is made once for each of the cycle's five rows, so that
    its case sees both verdicts."""
    return batch_rows(oracle, nb, 5)


# k_post call site: sf, mode, frames; every nb below at each.  Mode 2 (dechirp,
# lora_demodulate) returns a clean frame's own symbols.  Mode 0
# (lora_phy::demodulate) does not: its estimate over the two sync symbols of a
# clean frame is about -N / 3 samples and half a bin (phy.cpp:81-148 on two
# chirps), so the compensated symbols come out moved by a constant and hardly
# any row verifies.  The mode 0 shapes hold k_post to the oracle's chain on
# the same IQ; the mode 2 shapes at the same SFs carry the true verdicts.
POST_SHAPES = [(7, 0, 300), (7, 2, 300), (9, 0, 60), (9, 2, 60), (11, 0, 12), (11, 2, 12)]
POST_NB = {"block": (4, 8, 16, 32), "memory": (5, 33)}
POST_CASES = [(sf, mode, frames, nb, form) for sf, mode, frames in POST_SHAPES
              for form, nbs in POST_NB.items() for nb in nbs]


def fed(rows: np.ndarray, sf: int) -> np.ndarray:
    """What goes on the air of `rows`: a symbol is a chirp's start bin, so only
    its low sf bits (at SF 7 a code word's bit 7, a parity bit, is lost; from
    SF 9 up junk_high's bits 8 .. sf-1 are carried)."""
    return rows & np.uint16((1 << sf) - 1)


def chain(oracle, iq, sf, mode):
    """The oracle's receive chain on one frame -> (symbols, sync word, bytes,
    crc_ok): demodulate (mode 0) or dechirp + lora_demodulate (mode 2), then
    decode."""
    if mode == 0:
        n, syms, sync, _ = oracle.demodulate(iq, sf)
    else:
        n, syms, sync, _ = oracle.lora_demodulate(oracle.dechirp(iq, sf), sf)
    assert n == syms.size and n % 2 == 0
    nb, pay, crc = oracle.decode(syms)
    assert nb == n // 2
    return syms, sync, pay, crc


_POST = {}


def post_case(oracle, sf, mode, frames, nb):
    """One k_post case: the clean IQ of its rows [frames, (2 nb + 2) N] (shared
    between the modes) and the oracle chain's (symbols, sync words, bytes,
    crc_ok) per frame; built once, read-only."""
    if (sf, frames, nb) not in _POST:
        iq = np.stack([oracle.modulate(r, sf) for r in fed(batch_rows(oracle, nb, frames), sf)])
        iq.setflags(write=False)
        _POST[sf, frames, nb] = iq
    iq = _POST[sf, frames, nb]
    if (sf, mode, frames, nb) not in _POST:
        got = [chain(oracle, x, sf, mode) for x in iq]
        want = (np.stack([g[0] for g in got]), np.array([g[1] for g in got], np.uint8),
                np.stack([g[2] for g in got]), np.array([g[3] for g in got], np.uint8))
        for a in want:
            a.setflags(write=False)
        _POST[sf, mode, frames, nb] = want
    return iq, _POST[sf, mode, frames, nb]


# ragged call site: one pass of frame byte counts; frame j of pass p takes
# kind (j + p) % 5 of its cycle, so over RAGGED_PASSES passes every slot of
# the pass sees every kind.  The sums put 4, 8, 12, 32 on 16-byte-aligned
# symbol offsets first, then (after the 1) on unaligned ones.
RAGGED_SF = 8   # the smallest SF that carries all 8 bits of a code word
RAGGED_PASS = (4, 8, 12, 32, 1, 4, 8, 12, 32, 3, 5, 9, 33, 36, 0, 1, 36, 0)
RAGGED_PASSES = 5
RAGGED_SET = (0, 1, 3, 4, 5, 8, 9, 12, 32, 33, 36)


def ragged_lens():
    return list(RAGGED_PASS) * RAGGED_PASSES


def ragged_sym_offsets(lens):
    """lphy_hip_tx_layout's sym_offset: twice the exclusive prefix of the byte counts."""
    return [2 * int(x) for x in np.concatenate([[0], np.cumsum(lens)[:-1]])]


def ragged_rows(oracle):
    """The rows of the ragged table in address order."""
    n = len(RAGGED_PASS)
    return [row(oracle, nb, kind_cycle(nb)[(i % n + i // n) % 5], i // n) for i, nb in enumerate(ragged_lens())]


def ragged_order():
    """The table's record order: a fixed shuffle of the address order."""
    return np.random.default_rng(2024).permutation(len(ragged_lens()))


def ragged_form(nb, sym_offset) -> str:
    """k_rg_final's row (frames == 1, f == 0, no block form) at a 16-byte-aligned
    d_syms and a 4-byte-aligned d_bytes."""
    return form_of(2 * nb, 2 * nb, (2 * sym_offset) % 16, (sym_offset // 2) % 4, None, 0)


RAGGED_MODES = (2, 0)   # mode 2 carries the verdicts; mode 0 as in POST_SHAPES
_RAGGED = {}


def ragged_case(oracle, mode):
    """The ragged table's frames in address order: (clean IQ per frame, the
    oracle chain's (symbols, sync word, bytes, crc_ok) per frame); built once."""
    if "iq" not in _RAGGED:
        _RAGGED["iq"] = [oracle.modulate(fed(r, RAGGED_SF), RAGGED_SF) for r in ragged_rows(oracle)]
    if mode not in _RAGGED:
        _RAGGED[mode] = [chain(oracle, x, RAGGED_SF, mode) for x in _RAGGED["iq"]]
    return _RAGGED["iq"], _RAGGED[mode]
