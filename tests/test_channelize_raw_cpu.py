"""lphy_hip_channelize_raw without a device: the host-compilable part of it
(csrc/lphy_resample_plan.h: the staging split, the sample sizes, the two new
rows of the argument check; csrc/lphy_stage_plan.h: the host form's upload) as
a stand-alone program under ASan + UBSan (tests/cpp/channelize_raw_check.cpp),
the binding's constants against the header, and the tests' own conversion
(tests/sample_formats.py) against values written out by hand."""
import re
from pathlib import Path

import numpy as np
import pytest

import hostcc
import sample_formats as sf

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    return hostcc.run_check("channelize_raw_check.cpp", tmp_path_factory.mktemp("channelize_raw")).strip()


def test_plan_logic_under_the_host_sanitizers(check_output):
    assert re.fullmatch(r"channelize_raw_check: ok CF32=\d+ SC16=\d+ SC8=\d+ CU8=\d+", check_output), check_output


def test_binding_knows_the_formats(check_output):
    """lphy.FMT_* are the header's enumerators as the C compiler numbers them,
    and the binding exports and declares the three new symbols."""
    import lphy
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", check_output)}
    assert got == {"CF32": lphy.FMT_CF32, "SC16": lphy.FMT_SC16, "SC8": lphy.FMT_SC8, "CU8": lphy.FMT_CU8}
    text = (ROOT / "include" / "lphy_hip.h").read_text()
    for name, value in got.items():
        assert int(re.search(rf"LPHY_FMT_{name}\s*=\s*(\d+)", text).group(1)) == value
    assert (lphy.FMT_CF32, lphy.FMT_SC16, lphy.FMT_SC8, lphy.FMT_CU8) == (sf.FMT_CF32, sf.FMT_SC16, sf.FMT_SC8,
                                                                          sf.FMT_CU8)
    for sym in ("lphy_hip_sample_bytes", "lphy_hip_channelize_raw", "lphy_hip_channelize_raw_host"):
        assert sym in lphy.EXPORTS and re.search(rf"\b{sym}\(", text)
    for fmt in (sf.FMT_CF32, *sf.INT_FORMATS):
        assert lphy._fmt_dtype(fmt) == sf.DTYPES[fmt] and sf.DTYPES[fmt].itemsize * 2 == sf.BYTES[fmt]
    with pytest.raises(ValueError):
        lphy._fmt_dtype(4)


def test_to_float_is_the_definition():
    x = np.array([[-32768, 32767], [-1, 0], [1, -32767]], "<i2")
    assert sf.to_float(x, sf.FMT_SC16).tolist() == [-32768 + 32767j, -1 + 0j, 1 - 32767j]
    assert sf.to_float(x.reshape(-1), sf.FMT_SC16).tobytes() == sf.to_float(x, sf.FMT_SC16).tobytes()
    x = np.array([[-128, 127], [0, -1]], np.int8)
    assert sf.to_float(x, sf.FMT_SC8).tolist() == [-128 + 127j, 0 - 1j]
    x = np.array([[0, 255], [127, 128]], np.uint8)
    assert sf.to_float(x, sf.FMT_CU8).tolist() == [-127.5 + 127.5j, -0.5 + 0.5j]
    # every value of every integer format survives the conversion: float32 holds them all
    for fmt, lo, hi in [(sf.FMT_SC16, -32768, 32767), (sf.FMT_SC8, -128, 127), (sf.FMT_CU8, 0, 255)]:
        v = np.arange(lo, hi + 1)
        f = sf.to_float(np.stack([v, v[::-1]], axis=1).astype(sf.DTYPES[fmt]), fmt)
        assert f.dtype == np.complex64
        off = 127.5 if fmt == sf.FMT_CU8 else 0.0
        np.testing.assert_array_equal(f.real.astype(np.float64), v - off)
        np.testing.assert_array_equal(f.imag.astype(np.float64), v[::-1] - off)


def test_quantiser():
    z = np.array([0.5 + 0.25j, -1 - 1j, 1 + 1j, 4 - 4j])
    np.testing.assert_array_equal(sf.quantise(z, sf.FMT_SC16, 8192), [[4096, 2048], [-8192, -8192], [8192, 8192],
                                                                     [32767, -32768]])
    np.testing.assert_array_equal(sf.quantise(z, sf.FMT_SC8, 64), [[32, 16], [-64, -64], [64, 64], [127, -128]])
    q = sf.quantise(z, sf.FMT_CU8, 32)
    np.testing.assert_array_equal(q, [[144, 136], [96, 96], [160, 160], [255, 0]])  # 143.5 rounds to even
    assert q.dtype == np.uint8
    # to_float(quantise(z)) / scale is z to within half a level where nothing clipped
    assert np.abs(sf.to_float(q, sf.FMT_CU8)[:3] / 32 - z[:3]).max() <= 0.5 / 32 * np.sqrt(2) + 1e-12
