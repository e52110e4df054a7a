"""The frame search without a device: the host-compilable logic of
csrc/lphy_find_scan.h and find_frames_args (csrc/lphy_ragged_layout.h) as a
stand-alone program under ASan + UBSan (tests/cpp/find_frames_check.cpp), and
the numpy model of the definition (tests/find_frames_model.py) against three
tables written out by hand."""
import re
from pathlib import Path

import numpy as np

import hostcc
import find_frames_model as model

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "lora-sdr-lightweight-standalone-library-clean_amd"
CSRC = PKG / "csrc"


def test_scan_logic_under_the_host_sanitizers(tmp_path):
    out = hostcc.run_check("find_frames_check.cpp", tmp_path)
    assert out.strip() == "find_frames_check: ok", out


def test_binding_knows_the_tile():
    """lphy.FIND_TILE, which the device tests place their edges by, is the header's."""
    import lphy
    text = (CSRC / "lphy_find_scan.h").read_text()
    assert int(re.search(r"kFindTile = (\d+);", text).group(1)) == lphy.FIND_TILE
    assert lphy.FIND_PARAMS.itemsize == 48 and lphy.FIND_INFO.itemsize == 32
    assert lphy.DETECT_DTYPE == model.DETECT_DTYPE and lphy.RAGGED_DESC_DTYPE == model.DESC_DTYPE


def _rows(desc):
    return [tuple(int(x) for x in r) for r in desc]


def test_model_table_one_bridged_and_one_split_gap():
    # S = 128, hop = S, mode 2.  Active 2-4, 6-7 (gap 1: bridged), 10 (gap 2: split).
    act = np.zeros(12, bool)
    act[[2, 3, 4, 6, 7, 10]] = True
    p = model.params(total_samples=12 * 128, max_gap=1)
    desc, info = model.find_frames(model.records(act), p, 128, 2, 4)
    assert _rows(desc) == [(256, 768, 0, 0),       # windows 2 .. 7: 6 symbols, 4 data symbols
                           (1280, 128, 4, 6),      # window 10: 1 symbol, slot (1 + 1) & ~1 = 2
                           (1408, 0, 6, 7), (1408, 0, 6, 7), (1408, 0, 6, 7)]
    assert info == dict(frames=2, bursts=2, dropped_short=0, dropped_long=0, overflow=0, active=6)


def test_model_table_short_drop_clip_and_overflow():
    # S = 128, hop = 32 (a quarter), lead = 64, mode 1, min_symbols = 2, max_frames = 2.
    # Bursts: 0-3 (128 samples: 1 symbol, short), 8-19 (384: 3 symbols), 24-31 (256: 2),
    # 40-47 (256: 2, overflow), 60-63 (start 1984, clipped by 2000 to 16: short).
    act = np.zeros(64, bool)
    for a, b in ((0, 3), (8, 19), (24, 31), (40, 47), (60, 63)):
        act[a:b + 1] = True
    p = model.params(hop=32, lead=64, total_samples=2000, min_symbols=2)
    desc, info = model.find_frames(model.records(act), p, 128, 1, 2)
    assert _rows(desc) == [(64 + 256, 384, 0, 0),  # 3 symbols: 1 data symbol, slot 2
                           (64 + 768, 256, 2, 3),  # 2 symbols: no data symbol, slot 0
                           (64 + 768 + 256, 0, 2, 5)]
    assert info == dict(frames=2, bursts=5, dropped_short=2, dropped_long=0, overflow=1, active=36)


def test_model_table_values_and_empty():
    # the flag of each record, by the definition: float32 difference >= threshold, NaN inactive
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    rec = np.zeros(8, model.DETECT_DTYPE)
    rec["power"] = [-inf, inf, nan, 5.0, 12.5, 12.4999, inf, -3.0]
    rec["power_avg"] = [-inf, 0.0, 0.0, nan, 2.5, 2.5, inf, -inf]
    assert list(model.active_flags(rec, 10.0)) == [False, True, False, False, True, False, False, True]
    assert list(model.active_flags(rec, -np.inf)) == [False, True, False, False, True, True, False, True]
    assert list(model.active_flags(rec, np.inf)) == [False, True, False, False, False, False, False, True]
    # mode 0, first = 1000: windows 1, 4 and 7 are three one-symbol frames with no output symbol
    p = model.params(first=1000, total_samples=1000 + 8 * 128)
    desc, info = model.find_frames(rec, p, 128, 0, 3)
    assert _rows(desc) == [(1128, 128, 0, 0), (1512, 128, 0, 1), (1896, 128, 0, 2), (2024, 0, 0, 3)]
    assert info == dict(frames=3, bursts=3, dropped_short=0, dropped_long=0, overflow=0, active=3)
    # no record at all: the all-padding table and a zero info
    desc, info = model.find_frames(rec[:0], p, 128, 0, 2)
    assert _rows(desc) == [(0, 0, 0, 0)] * 3 and not any(info.values())
