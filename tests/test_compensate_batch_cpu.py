"""The batch forms of compensate_offsets (lphy_hip_compensate_batch, _ragged,
_batch_host) at the C ABI boundary, without a GPU: the library exports them,
the Python binding has bound them, and their argument checks come before any
device call."""
import ctypes as C
import errno

import pytest

from test_abi_cpu import HIP_SO, built  # noqa: F401  (the fixture builds the library when missing)

NAMES = ("lphy_hip_compensate_batch", "lphy_hip_compensate_ragged", "lphy_hip_compensate_batch_host")


def test_compensate_batch_argument_errors_without_device(built):  # noqa: F811
    lib = C.CDLL(str(HIP_SO))
    vp, sz = C.c_void_p, C.c_size_t
    lib.lphy_hip_compensate_batch.argtypes = [vp, vp, vp, sz, sz, vp, vp]
    lib.lphy_hip_compensate_ragged.argtypes = [vp, vp, vp, vp, sz, vp, vp]
    lib.lphy_hip_compensate_batch_host.argtypes = [vp, vp, sz, sz, vp]
    buf = (C.c_float * 64)()
    meta = (C.c_char * 64)()
    # a null context, with and without the other arguments
    assert lib.lphy_hip_compensate_batch(None, None, None, 1, 128, None, None) == -errno.EINVAL
    assert lib.lphy_hip_compensate_batch(None, buf, buf, 2, 4, meta, None) == -errno.EINVAL
    assert lib.lphy_hip_compensate_batch(None, buf, buf, 0, 0, meta, None) == -errno.EINVAL
    assert lib.lphy_hip_compensate_ragged(None, None, None, None, 1, None, None) == -errno.EINVAL
    assert lib.lphy_hip_compensate_ragged(None, buf, buf, meta, 2, meta, None) == -errno.EINVAL
    assert lib.lphy_hip_compensate_batch_host(None, None, 1, 128, None) == -errno.EINVAL
    assert lib.lphy_hip_compensate_batch_host(None, buf, 2, 4, meta) == -errno.EINVAL


def test_binding_has_bound_the_batch_forms(built, lphy):  # noqa: F811
    lib = lphy.load()
    for name in NAMES:
        assert name in lphy.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.lphy_hip_compensate_batch.argtypes) == 7
    assert len(lib.lphy_hip_compensate_ragged.argtypes) == 7
    assert len(lib.lphy_hip_compensate_batch_host.argtypes) == 5
    for name in ("compensate_batch", "compensate_ragged", "compensate_batch_host"):
        assert callable(getattr(lphy.Demodulator, name)), name
