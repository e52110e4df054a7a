#!/usr/bin/env python3
"""Generate tests/golden/detect_ragged_v1.npz from the REFERENCE build (TEST
INFRASTRUCTURE ONLY): LoRaDetector<float>::detect of oracle/_ref/libloraref.so
(oracle/Makefile, `ref_detect`) on every whole symbol of the SF 7 and SF 10
mixed-length tables of tests/detect_ragged_cases.py, no Hann window, each
symbol dechirped first (the input of a LPHY_DET_DECHIRP call).

Recorded results only: per SF the table (frames + 1 records of four uint64)
and one 16-byte record per whole symbol in table order.  The frames
themselves are rebuilt from their seeds by whoever compares against it.

Usage: python tests/golden/make_detect_ragged_golden.py   (from the repo root)
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
for p in (ROOT / "tests", ROOT / "lora-sdr-lightweight-standalone-library-clean_amd"):
    sys.path.insert(0, str(p))
import detect_cases as dc  # noqa: E402
import detect_ragged_cases as rc  # noqa: E402
import lphy  # noqa: E402  (the record layouts only)
from checkers import Oracle, Reference  # noqa: E402


def main() -> None:
    orc, ref = Oracle(), Reference()
    out = {}
    for sf in rc.GOLDEN_SFS:
        N = 1 << sf
        frames = rc.frames_of(orc, sf, dechirp=True)
        flat = np.concatenate(frames)
        desc = rc.packed_table(lphy, [x.size for x in frames], N)
        rec = np.zeros(int(desc["unit_offset"][-1]), lphy.DETECT_DTYPE)
        for f in range(len(frames)):
            u = int(desc["unit_offset"][f])
            for s in range(int(desc["samples"][f]) // N):
                x = dc.window_input(orc, flat, sf, int(desc["iq_offset"][f]), N, 1, s, False, False)
                idx, p, pa, fi, _ = ref.detect(ref.dechirp(x, sf))
                rec[u + s] = (p, pa, fi, idx, 0)
        out[f"desc_sf{sf}"] = desc.view(np.uint64).reshape(-1, 4)
        out[f"records_sf{sf}"] = rec.view(np.uint8).reshape(-1, 16)
    np.savez_compressed(rc.GOLDEN, **out)
    print(f"{rc.GOLDEN}: {rc.GOLDEN.stat().st_size} bytes")


if __name__ == "__main__":
    main()
