"""csrc/libm_exact.h, the device sqrtf and detector_power as hipcc compiles
them for gfx950, against glibc.

The host build of the header is pinned to glibc over all 2^32 floats
(tests/test_cpu_checks.py), but the device's is another program: inv_pio4()
takes the shift form of the Payne-Hanek windows, and the float division,
sqrtf, the double square root, (int32_t)r, the double-to-float conversions and
the f32 subnormal handling are the AMDGPU lowerings.  The rest of the GPU
suite reaches it through whole demodulations, which feed it one slice of its
domain.  Here the test build's probe lphy_hip_test_libm (csrc/lphy_testing.h)
runs each function over the sets of tests/libm_cases.py, which enter every
branch from both sides of every threshold (tests/test_libm_cases_cpu.py), and
every output is compared bit for bit (NaNs as NaNs) with glibc's through the
oracle, libm_cases.reference.  No input is left out or masked.
"""
import numpy as np
import pytest

import libm_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(lphy):
    d = lphy.Demodulator(7, test_build=True)
    yield d
    d.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The host build of the header, for sincos_large's reference below 120
    and for the failure report."""
    from checkers import HostLibm
    return HostLibm(tmp_path_factory.mktemp("libm_capi"))


def run(probe, op, a, b):
    import torch
    dev = torch.device(f"cuda:{probe.device}")
    ta = torch.from_numpy(a.view(np.int32)).to(dev).view(torch.float32)
    tb = None if b is None else torch.from_numpy(b.view(np.int32)).to(dev).view(torch.float32)
    o0, o1 = probe.libm_probe(lc.OPS[op], ta, tb, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.view(torch.int32).cpu().numpy().view(np.float32) for o in (o0, o1))


@pytest.mark.parametrize("op,name", lc.CASES, ids=[f"{o}-{s}" for o, s in lc.CASES])
def test_device_equals_glibc(oracle, host, probe, op, name):
    a, b = lc.cases(op)[name]
    got = run(probe, op, a, b)
    want = lc.reference(op, a, b, oracle, host)
    bad = lc.mismatches(got, want)
    if bad.size:
        msg = lc.report(op, a, b, bad, device=got, glibc=oracle.libm(lc.OPS[op], a, b),
                        header=host.libm(lc.OPS[op], a, b))
        print(msg)
        pytest.fail(f"{op} / {name}: {bad.size} of {a.size} inputs differ on the device\n{msg}")


def test_split_is_exact(probe):
    """rotate_sample's form (sincosf_needs_large ? sincosf_large : sincosf_fast)
    and sincosf_exact give the same bits for every input."""
    for name in ("edges", "workload"):
        a = lc.one_arg_sets()[name]
        one, two = run(probe, "sincos_exact", a, None), run(probe, "sincos_split", a, None)
        for x, y in zip(one, two):
            np.testing.assert_array_equal(lc.bits(x), lc.bits(y), err_msg=name)


def test_return_codes(lphy, probe):
    import ctypes as C

    import torch
    dev = torch.device(f"cuda:{probe.device}")
    a = torch.full((5,), 0.5, dtype=torch.float32, device=dev)
    b = torch.full((5,), 2.0, dtype=torch.float32, device=dev)
    o0 = torch.full((5,), -7.0, dtype=torch.float32, device=dev)
    o1 = torch.full((5,), -7.0, dtype=torch.float32, device=dev)
    fn = probe.lib.lphy_hip_test_libm
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    pa, pb, p0, p1 = (t.data_ptr() for t in (a, b, o0, o1))
    einval, erange = -22, -34
    ops = lc.OPS
    assert fn(None, ops["logf"], pa, pb, p0, p1, 5, None) == einval
    assert fn(probe.ctx, ops["logf"], None, pb, p0, p1, 5, None) == einval
    assert fn(probe.ctx, ops["logf"], pa, pb, None, p1, 5, None) == einval
    for bad_op in (-1, len(ops), 1 << 20):
        assert fn(probe.ctx, bad_op, pa, pb, p0, p1, 5, None) == einval
    # d_b / d_out1: needed by the ops that use them only
    for op in ("atan2", "cabs", "detector_power"):
        assert fn(probe.ctx, ops[op], pa, None, p0, None, 5, None) == einval
        assert fn(probe.ctx, ops[op], pa, pb, p0, None, 5, None) == 0
    for op in ("sincos_exact", "sincos_split", "sincos_large"):
        assert fn(probe.ctx, ops[op], pa, None, p0, None, 5, None) == einval
        assert fn(probe.ctx, ops[op], pa, None, p0, p1, 5, None) == 0
    for op in ("logf", "log10f", "sqrtf"):
        assert fn(probe.ctx, ops[op], pa, None, p0, None, 5, None) == 0
    torch.cuda.synchronize()
    # the null checks come before n == 0, -ERANGE after it; neither touches memory
    o0.fill_(-7.0)
    torch.cuda.synchronize()
    assert fn(probe.ctx, ops["logf"], None, None, p0, None, 0, None) == einval
    assert fn(probe.ctx, ops["logf"], pa, None, p0, None, 0, None) == 0
    for n in (1 << 32, (1 << 32) + 5, (1 << 64) - 1):
        assert fn(probe.ctx, ops["logf"], pa, None, p0, None, n, None) == erange
    torch.cuda.synchronize()
    assert torch.all(o0 == -7.0)
    # a call of n elements writes n elements
    assert fn(probe.ctx, ops["sqrtf"], pa, None, p0, None, 3, None) == 0
    torch.cuda.synchronize()
    assert o0.cpu().tolist() == [np.float32(0.5 ** 0.5)] * 3 + [-7.0] * 2


def test_product_library_has_no_probe(lphy):
    d = lphy.Demodulator(7, lib_path=lphy.HIP_SO)
    assert not hasattr(d.lib, "lphy_hip_test_libm")
    import torch
    with pytest.raises(AttributeError):
        d.libm_probe(lphy.LIBM_SQRTF, torch.zeros(4, dtype=torch.float32, device=f"cuda:{d.device}"))
    d.close()
