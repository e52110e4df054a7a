"""The channeliser without a device: the host-compilable part of it
(csrc/lphy_resample_plan.h: argument check, output count, tile geometry, LDS image)
as a stand-alone program under ASan + UBSan (tests/cpp/channelize_check.cpp),
the binding's constants against the headers, the numpy model of the definition
(tests/channelize_model.py) against tables written out by hand, and the design
helper lphy.chan_design against the model's own float64 maths."""
import re
from fractions import Fraction as F
from pathlib import Path

import numpy as np
import pytest

import hostcc
import channelize_model as model

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "lora-sdr-lightweight-standalone-library-clean_amd"
CSRC = PKG / "csrc"


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    return hostcc.run_check("channelize_check.cpp", tmp_path_factory.mktemp("channelize")).strip()


def test_plan_logic_under_the_host_sanitizers(check_output):
    assert re.fullmatch(r"channelize_check: ok kChanTile=\d+ sizeof\(lphy_chan_plan\)=\d+", check_output), check_output


def test_binding_knows_the_tile_and_the_plan(check_output):
    """lphy.CHAN_TILE, which the device tests place their edges by, is the
    header's, and CHAN_PLAN is lphy_chan_plan as the C compiler lays it out."""
    import lphy
    text = (CSRC / "lphy_resample_plan.h").read_text()
    assert int(re.search(r"kResTile = (\d+);", text).group(1)) == lphy.CHAN_TILE
    tile, size = (int(x) for x in re.findall(r"=(\d+)", check_output))
    assert tile == lphy.CHAN_TILE and size == lphy.CHAN_PLAN.itemsize == 64
    p = lphy.chan_plan(first=1, in_samples=2, outputs=3, out_stride=4, rot_first=5, channels=6, taps=7, decim=8,
                       rot_period=9)
    assert p.tobytes() == np.array([1, 2, 3, 4, 5], "<u8").tobytes() + np.array([6, 7, 8, 9, 0, 0], "<u4").tobytes()


def _c(*v):
    return np.array(v, np.complex64)


def test_model_unit_taps_are_a_copy_times_rot():
    x = _c(1 + 2j, -3 + 0.5j, 0.25 - 4j, 7j, -1)
    taps = _c(1, 1).reshape(2, 1)
    rot = np.stack([_c(1, 1j, -1), _c(2, -1j, 0.5)])     # R = 3
    y = model.channelize(x, taps, rot, 1)
    assert y.shape == (2, 5)
    np.testing.assert_array_equal(y[0], _c(1 + 2j, (-3 + 0.5j) * 1j, -(0.25 - 4j), 7j, -1j))
    np.testing.assert_array_equal(y[1], _c(2 + 4j, (-3 + 0.5j) * -1j, 0.125 - 2j, 14j, 1j))


def test_model_decim_past_the_taps_skips_samples():
    # T = 2, D = 3: output m is 2 x[3m] + 1j x[3m + 1]; x[3m + 2] is never read
    x = _c(1, 1, np.nan, 2, 3j, np.inf, -1, -1j)
    assert model.outputs(8, 0, 2, 3) == 3 and model.outputs(7, 0, 2, 3) == 2 and model.outputs(8, 1, 2, 3) == 2
    y = model.channelize(x, _c(2, 1j).reshape(1, 2), _c(1).reshape(1, 1), 3)
    np.testing.assert_array_equal(y[0], _c(2 + 1j, 4 - 3, -2 + 1))
    # first = 1 and a count of 1: x[1], x[2] alone
    y = model.channelize(x[:3], _c(1, 0).reshape(1, 2), _c(1).reshape(1, 1), 3, first=1, n_out=1)
    assert y.shape == (1, 1) and np.isnan(y[0, 0].real)   # 1 + nan * 0


def test_model_rot_first_wraps():
    x = _c(1, 1, 1, 1, 1)
    rot = _c(1, 2, 3).reshape(1, 3)
    taps = _c(1).reshape(1, 1)
    np.testing.assert_array_equal(model.channelize(x, taps, rot, 1, rot_first=2)[0], _c(3, 1, 2, 3, 1))
    np.testing.assert_array_equal(model.channelize(x, taps, rot, 1, rot_first=(1 << 40) + 3)[0],
                                  _c(*[[1, 2, 3][((1 << 40) + 3 + m) % 3] for m in range(5)]))
    # two blocks with the phase carried equal one
    one = model.channelize(x, taps, rot, 1, rot_first=1)
    two = np.concatenate([model.channelize(x[:2], taps, rot, 1, rot_first=1),
                          model.channelize(x, taps, rot, 1, first=2, rot_first=3)], axis=1)
    np.testing.assert_array_equal(one, two)


def test_model_keeps_the_order_of_the_sums():
    # 1e8 + 1 - 1e8 in float32, left to right, is 0; any other order gives 1
    x = _c(1e8, 1, -1e8)
    y = model.channelize(x, _c(1, 1, 1).reshape(1, 3), _c(1).reshape(1, 1), 1)
    assert y[0, 0] == 0
    # the accumulator starts at +0: a sum of negative zeros is +0
    y = model.channelize(_c(-0.0, -0.0), _c(1, 1).reshape(1, 2), _c(1).reshape(1, 1), 1)
    assert not np.signbit(y[0, 0].real)


@pytest.mark.parametrize("centres, decim, taps, cutoff, beta", [
    ([F(-3, 10), F(1, 10), F(3, 10)], 8, 129, 0.09, 8.0),
    ([F(0), F(1, 7), F(-5, 16), F(2, 5)], 16, 65, 1 / 40, 8.0),
    ([F(1, 3)], 1, 1, 0.25, 5.0),
    ([F(k, 8) - F(7, 16) for k in range(8)], 5, 64, 0.05, 6.5),
])
def test_design_helper_equals_the_model(centres, decim, taps, cutoff, beta):
    import lphy
    t, r, R, delay = lphy.chan_design(centres, decim, taps, cutoff, beta)
    mt, mr, mR, mdelay = model.design(centres, decim, taps, cutoff, beta)
    assert (R, delay) == (mR, mdelay) and t.dtype == r.dtype == np.complex64
    assert t.shape == (len(centres), taps) and r.shape == (len(centres), R)
    assert t.tobytes() == mt.tobytes() and r.tobytes() == mr.tobytes()
    # what the tables mean: unit gain at the centre, R the period of the rotation
    k = np.arange(taps)
    for c, f in enumerate(centres):
        gain = np.sum(t[c].astype(np.complex128) * np.exp(2j * np.pi * float(f) * k))
        assert abs(gain - 1) < 1e-5
        assert abs(r[c, 1 % R] - np.exp(-2j * np.pi * float(f * decim) * (1 % R))) < 1e-6


def test_design_helper_refuses_a_long_period():
    import lphy
    assert lphy.chan_design([F(1, 65536)], 1, 3, 0.1, 8.0)[2] == 65536
    with pytest.raises(ValueError):
        lphy.chan_design([F(1, 65537)], 1, 3, 0.1, 8.0)
    with pytest.raises(ValueError):
        model.design([F(1, 65537)], 1, 3, 0.1, 8.0)
    assert lphy.chan_design([F(1, 65537)], 65537, 3, 0.1, 8.0)[2] == 1
