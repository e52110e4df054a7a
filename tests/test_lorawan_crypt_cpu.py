"""The host side of the LoRaWAN FRMPayload cipher without a device
(csrc/lphy_lorawan_ragged.h, compiled into a host-only test library,
tests/cpp/lorawan_crypt_check.cpp, and called through ctypes):

* the A_i block the kernel encrypts, against a restatement of LoRaWAN 1.0.x
  4.3.3 (tests/lorawan_crypt_model.py);
* the three front ends that resolve a record to a job: the range, the fields
  and the order of the statuses lphy_hip.h documents;
* the same helpers as a stand-alone program under ASan + UBSan;
* the binding names the four entry points."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import hostcc
from lorawan_crypt_model import block_a

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "lora-sdr-lightweight-standalone-library-clean_amd"

DESC = np.dtype([("iq_offset", "<u8"), ("samples", "<u8"), ("sym_offset", "<u8"), ("unit_offset", "<u8")])
EINVAL, ERANGE, ENOKEY = -22, -34, -126
JOB = ("status", "offset", "len", "devaddr", "fcnt", "key", "uplink")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = hostcc.shared_lib("lorawan_crypt_check.cpp", tmp_path_factory.mktemp("lorawan_crypt"))
    L.lw_crypt_block_check.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.lw_crypt_block_check.restype = None
    L.lw_crypt_job_batch_check.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    L.lw_crypt_job_tx_check.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    L.lw_crypt_job_rx_check.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_uint64,
                                        C.c_uint32, C.c_void_p]
    L.lw_crypt_max_len_check.restype = C.c_uint32
    return L


@pytest.fixture(scope="module")
def lphy():
    import sys
    if str(PKG) not in sys.path:
        sys.path.insert(0, str(PKG))
    import lphy as m
    return m


@pytest.mark.parametrize("uplink", [True, False])
@pytest.mark.parametrize("i", [1, 16, 255])
def test_block_a_equals_the_restatement(lib, uplink, i):
    out = np.full(16, 0xEE, np.uint8)
    lib.lw_crypt_block_check(int(uplink), 0x01020304, 0x0A0B0C0D, i, out.ctypes.data)
    assert out.tobytes() == block_a(uplink, 0x01020304, 0x0A0B0C0D, i)
    # the restatement itself, byte by byte from the LoRaWAN text
    assert out.tobytes() == bytes([1, 0, 0, 0, 0, 0 if uplink else 1, 4, 3, 2, 1, 0x0D, 0x0C, 0x0B, 0x0A, 0, i])


def test_the_limit_is_255_blocks(lib):
    assert lib.lw_crypt_max_len_check() == 4080 == 255 * 16


def _job(fn, *args):
    out = np.full(7, -77, np.int64)
    fn(*args, out.ctypes.data)
    return dict(zip(JOB, (int(v) for v in out)))


def test_batch_front_end(lib, lphy):
    d = np.zeros(1, lphy.LORAWAN_DESC_DTYPE)
    d["offset"], d["len"], d["devaddr"], d["fcnt"], d["key"], d["uplink"] = 1 << 33, 4080, 0xDEADBEEF, 0xFEDCBA98, 4, 1

    def job(nkeys=5):
        return _job(lib.lw_crypt_job_batch_check, d.ctypes.data, nkeys)
    assert job() == dict(status=0, offset=1 << 33, len=4080, devaddr=0xDEADBEEF, fcnt=0xFEDCBA98, key=4, uplink=1)
    assert job(4)["status"] == ENOKEY
    d["len"] = 4081
    assert job()["status"] == ERANGE and job(4)["status"] == ENOKEY
    d["len"], d["uplink"] = 0, 0
    assert job()["status"] == 0 and job()["len"] == 0 and job()["uplink"] == 0


def test_tx_front_end_ranges_and_status_order(lib, lphy):
    t = np.zeros(1, lphy.LORAWAN_TX_DTYPE)
    t["src_offset"], t["devaddr"], t["key"], t["payload_len"] = 1000, 0x04030201, 2, 40
    t["fcnt"], t["mtype"], t["fopts_len"] = 0xBEEF, 2, 3

    def job(nkeys=3, skip=0):
        return _job(lib.lw_crypt_job_tx_check, t.ctypes.data, nkeys, skip)
    assert job() == dict(status=0, offset=1003, len=40, devaddr=0x04030201, fcnt=0xBEEF, key=2, uplink=1)
    assert job(skip=1) == dict(status=0, offset=1004, len=39, devaddr=0x04030201, fcnt=0xBEEF, key=2, uplink=1)
    t["mtype"] = 5
    assert job()["uplink"] == 0
    for pl, skip, want in [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 1), (2, 1, 1)]:
        t["payload_len"] = pl
        assert job(skip=skip)["len"] == want and job(skip=skip)["status"] == 0
    t["payload_len"] = 4081
    assert job()["status"] == ERANGE and job(skip=1)["status"] == 0
    # build's order: -EINVAL, then -ENOKEY, then -ERANGE
    assert job(nkeys=2)["status"] == ENOKEY
    t["fopts_len"] = 16
    assert job(nkeys=2)["status"] == EINVAL
    t["fopts_len"], t["mtype"] = 15, 8
    assert job(nkeys=2)["status"] == EINVAL
    t["mtype"] = 7
    assert job(nkeys=2)["status"] == ENOKEY and job()["status"] == ERANGE


def test_rx_front_end_ranges_and_status_order(lib, lphy):
    N = 128
    d = np.zeros(1, DESC)
    r = np.zeros(1, lphy.LORAWAN_FRAME_DTYPE)
    d["samples"], d["sym_offset"] = (2 * 40 + 2) * N + 17, 2 * 500 + 1      # a row of 40 bytes at byte 500
    r["status"], r["devaddr"], r["payload_offset"], r["payload_len"] = 17, 0xA1B2C3D4, 19, 17
    r["fcnt"], r["mhdr"] = 0x1234, 0x40

    def job(key=1, mode=1, nkeys=2, skip=0, step=N):
        return _job(lib.lw_crypt_job_rx_check, d.ctypes.data, r.ctypes.data, key, step, mode, nkeys, skip)
    assert job() == dict(status=0, offset=519, len=17, devaddr=0xA1B2C3D4, fcnt=0x1234, key=1, uplink=1)
    assert job(skip=1) == dict(status=0, offset=520, len=16, devaddr=0xA1B2C3D4, fcnt=0x1234, key=1, uplink=1)
    assert job(mode=0)["status"] == 0 and job(mode=2)["status"] == 0
    r["mhdr"] = 0x23 | 0x60
    assert job()["uplink"] == 0
    # payload_offset + payload_len + 4 > len
    r["payload_len"] = 18
    assert job()["status"] == EINVAL
    assert job(step=64)["status"] == 0          # the same samples are a row of 81 bytes at 64 a symbol
    r["payload_len"] = 0xFFFFFFFF
    assert job()["status"] == EINVAL
    r["payload_offset"], r["payload_len"] = 7, 0
    assert job()["status"] == EINVAL
    r["payload_offset"] = 36
    assert job()["status"] == 0 and job()["len"] == 0 and job(skip=1)["len"] == 0
    r["payload_offset"] = 37
    assert job()["status"] == EINVAL
    # the order: samples, the record's status, the record's extent, the key, the limit
    r["payload_offset"], r["payload_len"] = 19, 17
    assert job(key=2)["status"] == ENOKEY and job(key=0xFFFFFFFF, nkeys=1 << 40)["status"] == ENOKEY
    r["payload_len"] = 18
    assert job(key=2)["status"] == EINVAL
    r["status"] = ERANGE
    assert job(key=2)["status"] == ERANGE
    r["status"] = ENOKEY
    assert job()["status"] == ENOKEY
    r["status"] = EINVAL
    d["samples"] = 1 << 31
    assert job()["status"] == ERANGE
    d["samples"] = (2 * 4200 + 2) * N
    r["status"], r["payload_offset"], r["payload_len"] = 4081, 8, 4081
    assert job()["status"] == ERANGE and job(skip=1)["status"] == 0 and job(key=2)["status"] == ENOKEY


def test_front_ends_under_the_host_sanitizers(tmp_path):
    """The same source as a stand-alone program (-DLW_CRYPT_MAIN) under ASan +
    UBSan: the block and the three front ends on exactly-sized heap records."""
    out = hostcc.run_check("lorawan_crypt_check.cpp", tmp_path, define="LW_CRYPT_MAIN", skip_without_sanitizers=True)
    assert out.strip() == "lorawan_crypt_check: ok", out


def test_binding_names_the_entry_points(lphy):
    for name in ("lphy_hip_lorawan_crypt_batch", "lphy_hip_lorawan_crypt_tx_ragged",
                 "lphy_hip_lorawan_crypt_rx_ragged", "lphy_hip_lorawan_crypt_host"):
        assert name in lphy.EXPORTS
    for f in ("lorawan_crypt_batch", "lorawan_crypt_tx_ragged", "lorawan_crypt_rx_ragged", "lorawan_crypt"):
        assert callable(getattr(lphy, f))
    assert lphy.LW_CRYPT_MAX == 4080


def test_the_header_declares_the_entry_points_and_the_mic_caveat():
    text = (ROOT / "include" / "lphy_hip.h").read_text()
    for name in ("lphy_hip_lorawan_crypt_batch", "lphy_hip_lorawan_crypt_tx_ragged",
                 "lphy_hip_lorawan_crypt_rx_ragged", "lphy_hip_lorawan_crypt_host"):
        assert f"int {name}(" in text
    assert "no longer covers" in text
