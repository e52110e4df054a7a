"""Shared by tests/test_gpu_detect_ragged.py, tests/test_detect_ragged_cpu.py
and tests/golden/make_detect_ragged_golden.py: the mixed-length frames of the
ragged detector's tests and what lphy_hip_detect_ragged must return for a
table, from the CPU oracle alone (tests/detect_cases.py per frame).

Frame f of a table feeds the detector, per whole symbol s, the N samples
iq[iq_offset + s * N * osr + phase + i * osr]; its records are those of
dc.expected(first = iq_offset + phase, hop = N * osr, step = osr, windows = n)
and lie at unit_offset.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

import detect_cases as dc
from test_gpu_ragged import MIXED, mixed_frames

# whole symbols per frame.  SF 7-8: 196 units, 7 tiles of 32 / 13 of 16 (the
# last partial); SF 10: 11 units, 3 tiles of 4; SF 12: 6 tiles of 1
COUNTS = {7: MIXED[7], 8: MIXED[8], 10: [0, 1, 2, 5, 3], 12: [0, 1, 3, 2]}
GOLDEN = Path(__file__).parent / "golden" / "detect_ragged_v1.npz"
GOLDEN_SFS = (7, 10)


def tile_of(sf):
    """Geo<SF>::T: symbols per tile of 256 threads, N / 16 lanes each."""
    return 256 // max(1, (1 << sf) // 16)


def tailed(counts):
    """The two frames that carry a partial symbol of N / 2 samples: one inside
    the buffer (the frames behind it then start off the symbol grid), and the
    last (its tail ends the buffer)."""
    return (2, len(counts) - 1)


def frames_of(oracle, sf, dechirp):
    """The frames of COUNTS[sf] as a call with (dechirp=True) or without
    LPHY_DET_DECHIRP is given them (dc.detector_feed per frame: the detector
    sees dechirped symbols either way); the partial symbols stay raw."""
    N = 1 << sf
    counts = COUNTS[sf]
    out = []
    for k, x in enumerate(mixed_frames(oracle, sf, counts, tail=N // 2)):
        whole = counts[k] * N
        x = x if k in tailed(counts) else x[:whole]
        if not dechirp:
            x = np.concatenate([oracle.dechirp(x[:whole], sf), x[whole:]])
        out.append(np.ascontiguousarray(x, np.complex64))
    return out


def expected_table(oracle, lphy, iq, desc, sf, dechirp, hann, osr=1, phase=0):
    """All records of one ragged call: dc.expected per frame at unit_offset."""
    N = 1 << sf
    step = N * osr
    units = int(desc["unit_offset"][-1])
    out = np.zeros(units, lphy.DETECT_DTYPE)
    for f in range(desc.size - 1):
        n = int(desc["samples"][f]) // step
        u = int(desc["unit_offset"][f])
        out[u: u + n] = dc.expected(oracle, lphy, iq, sf, int(desc["iq_offset"][f]) + phase, step, osr, n, dechirp,
                                    hann)
    return out


def packed_table(lphy, lens, step):
    """What lphy_hip_ragged_layout gives for frames back to back (mode 0; the
    detector does not read sym_offset), without a context."""
    lens = np.asarray(lens, np.uint64)
    total = lens // np.uint64(step)
    desc = np.zeros(lens.size + 1, lphy.RAGGED_DESC_DTYPE)
    desc["iq_offset"] = np.concatenate([[0], np.cumsum(lens)])
    desc["samples"][:-1] = lens
    per = np.where(total >= 2, total - np.minimum(total, 2), 0)
    desc["sym_offset"] = np.concatenate([[0], np.cumsum((per + 1) & ~np.uint64(1))])
    desc["unit_offset"] = np.concatenate([[0], np.cumsum(total)])
    return desc


def load_golden():
    """{sf: (desc, records)}: the SF 7 and SF 10 tables of COUNTS, no Hann,
    LPHY_DET_DECHIRP, and the records the reference build's detect gave."""
    import lphy
    z = np.load(GOLDEN)
    return {sf: (z[f"desc_sf{sf}"].view(lphy.RAGGED_DESC_DTYPE).reshape(-1),
                 z[f"records_sf{sf}"].view(lphy.DETECT_DTYPE).reshape(-1)) for sf in GOLDEN_SFS}
