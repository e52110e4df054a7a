"""CPU-side foundations of tests/test_gpu_detect_ragged.py (no GPU):

* tests/golden/detect_ragged_v1.npz (tests/golden/make_detect_ragged_golden.py)
  holds what the reference build's LoRaDetector::detect gave for every whole
  symbol of the SF 7 and SF 10 mixed-length tables, no Hann, dechirped.  The
  per-frame expectation of the GPU test (detect_ragged_cases.expected_table
  over detect_cases.expected) is pinned to it bit for bit, and so is the table
  those tests build;
* the fixture has the shape the GPU test relies on: a frame without a whole
  symbol, two frames with a partial symbol (one inside the buffer), a unit
  total that is no multiple of the tile;
* the binding's buffer checks, which need no context."""
import numpy as np
import pytest
import torch

import detect_cases as dc
import detect_ragged_cases as rc


@pytest.mark.parametrize("sf", rc.GOLDEN_SFS)
def test_expected_table_is_the_reference_builds(oracle, lphy, sf):
    N = 1 << sf
    desc, want = rc.load_golden()[sf]
    frames = rc.frames_of(oracle, sf, dechirp=True)
    mine = rc.packed_table(lphy, [x.size for x in frames], N)
    for k in ("iq_offset", "samples", "unit_offset"):
        np.testing.assert_array_equal(mine[k], desc[k], err_msg=k)
    got = rc.expected_table(oracle, lphy, np.concatenate(frames), desc, sf, True, False)
    dc.assert_records_equal(got, want, f"SF{sf}")
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))   # no NaN among them
    assert np.isfinite(want["power_avg"]).all()


@pytest.mark.parametrize("sf", sorted(rc.COUNTS))
def test_fixture_shape(sf):
    N, T = 1 << sf, rc.tile_of(sf)
    counts = rc.COUNTS[sf]
    units = sum(counts)
    assert counts[0] == 0 and min(counts[1:]) >= 1
    assert -(-units // T) >= 3 and (T == 1 or units % T != 0)
    a, b = rc.tailed(counts)
    assert 0 < a < b == len(counts) - 1 and counts[a] > 0
    # the frames behind the first tail start off the symbol grid
    assert (sum(counts[: a + 1]) * N + N // 2) % N != 0


def test_binding_checks_its_buffers(lphy):
    """Demodulator.detect_ragged checks its tensors (lphy._dev_buf) before the
    library is called: no context is needed to see that."""
    class Ctx:  # the attributes detect_ragged reads before its first library call
        device, ctx, lib = 0, None, None
    iq, desc, out = torch.zeros(64), torch.zeros(96, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="cpu"):
        lphy.Demodulator.detect_ragged(Ctx(), iq, desc, 2, out, iq_samples=8, units=4)
    with pytest.raises(ValueError, match="device tensor"):
        lphy.Demodulator.detect_ragged(Ctx(), np.zeros(64, np.float32), desc, 2, out, iq_samples=8, units=4)
    with pytest.raises(ValueError, match="device tensor"):
        lphy.Demodulator.detect_ragged(Ctx(), None, desc, 2, out)
    assert "lphy_hip_detect_ragged" in lphy.EXPORTS and "lphy_hip_detect_ragged_host" in lphy.EXPORTS
