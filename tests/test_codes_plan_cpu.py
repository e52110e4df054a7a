"""The whitening generators without a device: csrc/lphy_codes_plan.h (the
recurrences, their periods and the reduction of (kind, bit_ofs, j) to a table
position or a step count below one period, which k_whiten and
lphy_hip_whiten_batch use) as a stand-alone program under ASan + UBSan
(tests/cpp/codes_plan_check.cpp): the periods derived again by stepping, the
reduced masks against the unreduced walk, the positions around INT_MAX in 64
bits, and the masks of the first 4096 positions against the oracle's whitening
(pinned to the reference header by tests/test_oracle_vs_reference.py)."""
import re

import numpy as np
import pytest

import hostcc


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """codes_plan_check.cpp's output for the given arguments; built on the first call"""
    tmp = tmp_path_factory.mktemp("codes_plan")
    return lambda *args: hostcc.run_check("codes_plan_check.cpp", tmp, *args, timeout=120)


def test_periods_and_reduction_under_the_host_sanitizers(check):
    out = check()
    m = re.fullmatch(r"codes_plan_check: ok periods=511,510,255 checked=(\d+)", out.strip())
    assert m and int(m.group(1)) == 316456, out   # every comparison made: no loop came up empty


def test_reduced_masks_equal_the_oracle(check, oracle):
    """Whitening zeros gives the masks themselves: 4096 positions (eight
    periods) of every kind and rdd, from bit_ofs 0 and from 777."""
    lines = check("dump").splitlines()
    assert len(lines) == 3 * 5 * 2
    seen = set()
    for line in lines:
        kind, rdd, ofs, hexes = line.split()
        kind, rdd, ofs = int(kind), int(rdd), int(ofs)
        got = np.frombuffer(bytes.fromhex(hexes), np.uint8)
        assert got.size == 4096
        np.testing.assert_array_equal(got, oracle.whiten(np.zeros(4096, np.uint8), kind, ofs, rdd), str((kind, rdd, ofs)))
        seen.add((kind, rdd, ofs))
    assert seen == {(k, r_, o) for k in range(3) for r_ in range(5) for o in (0, 777)}
