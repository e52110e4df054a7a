"""lphy_hip_channelize / lphy_hip_channelize_host (csrc/lphy_chan.h) against
the definition in plain numpy float32 (tests/channelize_model.py, itself
checked by tests/test_channelize_cpu.py).  The result is a pure function of the
inputs, every operation a float32 one in a fixed order, so every comparison is
on the bytes.  Any SF: the call does not depend on it (SF 7 here).

K = lphy.CHAN_TILE outputs make a tile.  A plan takes the LDS path when a full
tile's padded span fits 64 KiB (T = 3 at D = 40 does not: the global path)."""
import numpy as np
import pytest

import channelize_model as model
from resample_helpers import BIG, EINVAL, ERANGE, _u8, dem, guarded, rand_c64, unguarded  # noqa: F401 (dem: a fixture)

pytestmark = pytest.mark.gpu

PAD = 3        # out_stride = outputs + PAD


def inputs(seed, C_, T, D, n_out, first, R, extra=2):
    rng = np.random.default_rng(seed)
    n = first + (n_out - 1) * D + T + extra if n_out else first + extra
    return rand_c64(rng, n), rand_c64(rng, C_, T), rand_c64(rng, C_, R)


def device_call(lphy, d, x, taps, rot, D, first, n_out, rot_first, fill=0xA5, offset8=False, in_samples=None):
    """The device form with the output between guard samples and everything
    pre-filled with `fill`: the [C, out_stride] complex64 output as left."""
    import torch
    dev = torch.device("cuda", d.device)
    C_, T = taps.shape
    R = rot.shape[1]
    stride = n_out + PAD
    xf = np.ascontiguousarray(x, np.complex64).view(np.float32)
    if offset8:  # the samples start 8 bytes into the (at least 16-byte aligned) allocation
        t_all = torch.zeros(xf.size + 2, dtype=torch.float32, device=dev)
        assert t_all.data_ptr() % 16 == 0
        t_x = t_all[2:]
        t_x.copy_(torch.from_numpy(xf.copy()))
        assert t_x.data_ptr() % 16 == 8
    else:
        t_x = torch.from_numpy(xf.copy()).to(dev)
        assert t_x.data_ptr() % 16 == 0
    t_taps = torch.from_numpy(taps.view(np.float32).copy()).to(dev)
    t_rot = torch.from_numpy(rot.view(np.float32).copy()).to(dev)
    t_all_out, t_out = guarded(dev, C_ * stride * 8, fill)
    plan = lphy.chan_plan(first, x.size if in_samples is None else in_samples, n_out, stride, rot_first, C_, T, D, R)
    d.channelize(t_x, plan, t_taps, t_rot, t_out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return unguarded(t_all_out, C_ * stride * 8, fill).view(np.complex64).reshape(C_, stride).copy()


def assert_output(got, want, n_out, fill, what):
    np.testing.assert_array_equal(_u8(got[:, :n_out]), _u8(want), err_msg=what)
    assert (_u8(got[:, n_out:]) == fill).all(), f"{what}: the gaps between the channels' streams were written"


def cases(lphy):
    K = lphy.CHAN_TILE
    #        C   T     D      outputs    first R  rot_first
    return [(1,  1,    1,     1,         0,    1, 0),        # LDS path
            (3,  5,    1,     K - 1,     1,    5, 4),
            (8,  5,    4,     K,         2,    7, 6),
            (64, 64,   16,    K + 1,     3,    5, BIG),
            (8,  67,   16,    3 * K + 5, 5,    7, BIG),
            (3,  3,    7,     K + 1,     1,    1, 0),
            (8,  129,  8,     3 * K + 5, 0,    5, 0),
            (1,  129,  8,     K,         3,    7, 6),
            (64, 5,    4,     1,         5,    5, 4),
            (1,  67,   16,    K - 1,     2,    1, BIG),
            (3,  64,   16,    3 * K + 5, 1,    7, 0),
            (8,  1,    1,     K + 1,     0,    5, BIG),
            (2,  5,    1,     3 * K + 5, 3,    7, 6),        # groups of 2
            (5,  3,    7,     K,         5,    5, 0),        # a group of 8 with 5 channels in it
            (12, 5,    4,     K + 1,     0,    1, 0),        # a full group and a partial one
            (4,  129,  8,     1,         1,    5, 4),
            (1,  4096, 1,     K + 1,     1,    7, 6),        # the longest filter, still in LDS
            (2,  4096, 300,   5,         1,    5, 4),        # global path: the span cannot fit
            (1,  3,    40,    1,         0,    1, 0),
            (3,  3,    40,    K - 1,     3,    7, BIG),
            (8,  3,    40,    K,         2,    5, 0),
            (2,  3,    40,    K + 1,     5,    7, 6),
            (64, 3,    40,    3 * K + 5, 1,    5, 4),
            (3,  1,    65536, 3,         0,    1, 0)]        # the largest decimation


@pytest.mark.parametrize("k", range(24))
def test_shapes_against_the_model(lphy, dem, k):
    C_, T, D, n_out, first, R, rf = cases(lphy)[k]
    what = f"C={C_} T={T} D={D} outputs={n_out} first={first} R={R} rot_first={rf}"
    x, taps, rot = inputs(500 + k, C_, T, D, n_out, first, R)
    want = model.channelize(x, taps, rot, D, first, n_out, rf)
    assert_output(device_call(lphy, dem, x, taps, rot, D, first, n_out, rf), want, n_out, 0xA5, what)


@pytest.mark.parametrize("first", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("offset8", [False, True])
@pytest.mark.parametrize("T, D", [(5, 4), (67, 16), (3, 40)])
def test_alignment_of_the_span(lphy, dem, first, offset8, T, D):
    """`first` odd or even on a 16- or an 8-byte aligned capture, with a span of
    an odd and an even count of samples: the head and the tail of the staging."""
    K = lphy.CHAN_TILE
    for n_out in (K + 2, K + 3) if D % 2 else (K + 2,):
        for T_ in (T, T + 1):
            x, taps, rot = inputs(900 + first, 3, T_, D, n_out, first, 5, extra=0)
            want = model.channelize(x, taps, rot, D, first, n_out, 3)
            got = device_call(lphy, dem, x, taps, rot, D, first, n_out, 3, offset8=offset8)
            assert_output(got, want, n_out, 0xA5, f"first={first} offset8={offset8} T={T_} D={D} outputs={n_out}")


@pytest.mark.parametrize("T, D", [(67, 16), (5, 1), (3, 40), (2, 7)])
def test_blocks_with_overlap_equal_one_call(lphy, dem, T, D):
    """One capture in one call, and in three calls on three pieces of it that
    overlap by T - D samples (lie D - T apart where D > T), with rot_first
    advanced: the same bytes."""
    K = lphy.CHAN_TILE
    counts = [K + 7, 2 * K - 1, 40]
    total = sum(counts)
    x, taps, rot = inputs(77, 3, T, D, total, 0, 7, extra=0)
    one = device_call(lphy, dem, x, taps, rot, D, 0, total, 5)[:, :total]
    np.testing.assert_array_equal(_u8(one), _u8(model.channelize(x, taps, rot, D, 0, total, 5)))
    parts, m0 = [], 0
    for n in counts:
        # as a streaming caller holds it: the block alone, from its first sample on
        a, b = m0 * D, (m0 + n - 1) * D + T
        parts.append(device_call(lphy, dem, x[a:b], taps, rot, D, 0, n, 5 + m0)[:, :n])
        m0 += n
    np.testing.assert_array_equal(_u8(np.concatenate(parts, axis=1)), _u8(one))
    # and with `first` advanced on the whole capture
    parts, m0 = [], 0
    for n in counts:
        parts.append(device_call(lphy, dem, x, taps, rot, D, m0 * D, n, 5 + m0)[:, :n])
        m0 += n
    np.testing.assert_array_equal(_u8(np.concatenate(parts, axis=1)), _u8(one))


SPECIALS = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-40, -1e-42, 3e38, -3e38, 1.17549435e-38], np.float32)


@pytest.mark.parametrize("T, D", [(5, 4), (3, 40)])
def test_special_values(lphy, dem, T, D):
    """+-inf, NaN, +-0, subnormals and 3e38 inside and at the edges of the tiles,
    in the samples and in the tables.  NaNs are compared by position (their
    payload is the machine's), everything else by its bytes: a device that
    flushed subnormals would fail here."""
    K = lphy.CHAN_TILE
    n_out, first, R = 2 * K + 3, 1, 5
    x, taps, rot = inputs(31, 3, T, D, n_out, first, R)
    xf = x.view(np.float32)
    # subnormal results need subnormal factors: scale a stretch of the capture down
    xf[2 * (first + 40 * D): 2 * (first + 60 * D)] *= np.float32(1e-39)
    spots = [first, first + 1, first + T - 1, first + (K - 1) * D, first + (K - 1) * D + T - 1, first + K * D,
             first + K * D + 1, first + (2 * K - 1) * D + T - 1, first + 2 * K * D, x.size - 3, first + 100 * D + 1,
             first + 130 * D, first + 50 * D, first + 55 * D + 1]
    for i, at in enumerate(spots):
        xf[2 * at + (i & 1)] = SPECIALS[i % SPECIALS.size]
        if i % 3 == 0:
            xf[2 * at + 1 - (i & 1)] = SPECIALS[(i + 4) % SPECIALS.size]
    taps.view(np.float32)[1, 2] = np.float32(1e-39)
    taps.view(np.float32)[2, 1] = np.float32(3e38)
    taps.view(np.float32)[2, 4] = np.float32(-0.0)
    rot.view(np.float32)[1, 3] = np.float32(1e-8)
    want = model.channelize(x, taps, rot, D, first, n_out, 2)
    got = device_call(lphy, dem, x, taps, rot, D, first, n_out, 2)
    w, g = want.view(np.float32), got[:, :n_out].copy().view(np.float32)
    nan = np.isnan(w)
    sub = (np.abs(w) > 0) & (np.abs(w) < np.float32(1.17549435e-38))
    assert nan.any() and np.isinf(w).any() and sub.any() and (~nan).sum() > nan.sum()  # (of the input)
    np.testing.assert_array_equal(np.isnan(g), nan)
    np.testing.assert_array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan])


def test_result_does_not_depend_on_the_output_buffer(lphy, dem):
    K = lphy.CHAN_TILE
    x, taps, rot = inputs(5, 8, 67, 16, K + 9, 1, 7)
    a = device_call(lphy, dem, x, taps, rot, 16, 1, K + 9, 3, fill=0x00)
    b = device_call(lphy, dem, x, taps, rot, 16, 1, K + 9, 3, fill=0xFF)
    np.testing.assert_array_equal(_u8(a[:, :K + 9]), _u8(b[:, :K + 9]))
    assert (_u8(a[:, K + 9:]) == 0x00).all() and (_u8(b[:, K + 9:]) == 0xFF).all()


@pytest.mark.parametrize("k", [4, 12, 21])
def test_host_form_equals_the_device_form(lphy, dem, k):
    C_, T, D, n_out, first, R, rf = cases(lphy)[k]
    x, taps, rot = inputs(500 + k, C_, T, D, n_out, first, R)
    got = device_call(lphy, dem, x, taps, rot, D, first, n_out, rf)[:, :n_out]
    out = np.full((C_, n_out + PAD), np.complex64(7 - 7j))
    host = dem.channelize_host(x, taps, rot, D, first=first, outputs=n_out, rot_first=rf, out=out)
    np.testing.assert_array_equal(_u8(host), _u8(got))
    assert (out[:, n_out:] == np.complex64(7 - 7j)).all()
    # and with the defaults: every output the capture holds
    all_out = dem.channelize_host(x, taps, rot, D, first=first, rot_first=rf)
    assert all_out.shape == (C_, lphy.channelize_outputs(x.size, first, T, D)) and all_out.shape[1] >= n_out
    np.testing.assert_array_equal(_u8(all_out[:, :n_out]), _u8(got))


def test_outputs_count(lphy):
    for n, first, T, D in [(1000, 3, 5, 4), (10, 0, 11, 1), (10, 0, 10, 3), (10, 11, 1, 1), (1 << 48, 0, 1, 65536),
                           (5, 0, 0, 1), (5, 0, 1, 0)]:
        assert lphy.channelize_outputs(n, first, T, D) == model.outputs(n, first, T, D)


def test_return_codes(lphy, dem):
    """Every documented return through the library's entry points, device and
    host form; nothing is written (the sentinel stays), no device call is made
    (the buffers are far smaller than the refused plans describe)."""
    import torch
    dev = torch.device("cuda", dem.device)
    L = dem.lib
    FILL = 0x5A
    t_x = torch.zeros(2 * 64, dtype=torch.float32, device=dev)
    t_taps = torch.zeros(2 * 64 * 8, dtype=torch.float32, device=dev)
    t_rot = torch.zeros(2 * 64 * 8, dtype=torch.float32, device=dev)
    t_out = torch.full((8 * 64,), FILL, dtype=torch.uint8, device=dev)
    h_x, h_taps, h_rot = np.zeros(64, np.complex64), np.zeros(512, np.complex64), np.zeros(512, np.complex64)
    h_out = np.full(64, np.complex64(3 + 4j))
    ok = dict(first=1, in_samples=64, outputs=8, out_stride=10, rot_first=0, channels=3, taps=5, decim=4, rot_period=7)
    k32, k48 = 1 << 32, 1 << 48

    def both(want, ctx=True, null=(), off=(), plan=True, **changes):
        p = lphy.chan_plan(**dict(ok, **changes))
        pp = p.ctypes.data if plan else None
        c = dem.ctx if ctx else None
        dptr = dict(x=t_x.data_ptr(), taps=t_taps.data_ptr(), rot=t_rot.data_ptr(), out=t_out.data_ptr())
        hptr = dict(x=h_x.ctypes.data, taps=h_taps.ctypes.data, rot=h_rot.ctypes.data, out=h_out.ctypes.data)
        for ptr in (dptr, hptr):
            for n in null:
                ptr[n] = None
            for n in off:
                ptr[n] += 4
        assert L.lphy_hip_channelize(c, dptr["x"], pp, dptr["taps"], dptr["rot"], dptr["out"], None) == want, changes
        assert L.lphy_hip_channelize_host(c, hptr["x"], pp, hptr["taps"], hptr["rot"], hptr["out"]) == want, changes

    both(EINVAL, ctx=False)
    both(EINVAL, plan=False)
    both(EINVAL, null=("taps",))
    both(EINVAL, null=("rot",))
    both(EINVAL, null=("x",))
    both(EINVAL, null=("out",))
    for n in ("x", "taps", "rot", "out"):
        both(EINVAL, off=(n,))
    both(EINVAL, reserved=(1, 0))
    both(EINVAL, reserved=(0, 1))
    for n in ("channels", "taps", "decim", "rot_period"):
        both(EINVAL, **{n: 0})
    # the order: -EINVAL in front of every -ERANGE, a null pointer in front of a bad plan
    both(EINVAL, channels=65, reserved=(0, 1))
    both(EINVAL, taps=5000, decim=0)
    both(EINVAL, off=("rot",), out_stride=1)
    both(EINVAL, null=("out",), in_samples=3)
    both(ERANGE, channels=65)
    both(ERANGE, taps=4097)
    both(ERANGE, decim=65537)
    both(ERANGE, rot_period=65537)
    both(ERANGE, outputs=k32, out_stride=k32)
    both(ERANGE, out_stride=7)
    both(ERANGE, in_samples=k48 + 1)
    both(ERANGE, in_samples=1 + 7 * 4 + 5 - 1)
    both(ERANGE, first=(1 << 64) - 30)
    both(ERANGE, first=65)
    both(ERANGE, out_stride=k48 // 3 + 1)
    both(ERANGE, out_stride=(1 << 64) - 1)
    torch.cuda.synchronize()
    assert (t_out.cpu().numpy() == FILL).all() and (h_out == np.complex64(3 + 4j)).all()
    # outputs == 0: returns 0, launches nothing, asks for neither the samples nor the output
    both(0, outputs=0, out_stride=0)
    both(0, outputs=0, null=("x", "out"), first=1000)
    both(ERANGE, outputs=0, channels=65)
    # and a legal call on these buffers goes through: exactly the plan's edge
    both(0, in_samples=1 + 7 * 4 + 5)
    torch.cuda.synchronize()
    assert (t_out.cpu().numpy()[8 * 30:] == FILL).all() and (t_out.cpu().numpy()[: 8 * 8] == 0).all()


def test_binding_checks_the_tensors(lphy, dem):
    import torch
    dev = torch.device("cuda", dem.device)
    z = lambda n: torch.zeros(2 * n, dtype=torch.float32, device=dev)  # noqa: E731
    p = lphy.chan_plan(0, 100, 24, 24, 0, 2, 5, 4, 3)
    dem.channelize(z(100), p, z(10), z(6), z(48))
    for bad in [(z(99), z(10), z(6), z(48)), (z(100), z(9), z(6), z(48)), (z(100), z(10), z(5), z(48)),
                (z(100), z(10), z(6), z(47)), (z(100).cpu(), z(10), z(6), z(48))]:
        with pytest.raises(ValueError):
            dem.channelize(bad[0], p, bad[1], bad[2], bad[3])
    torch.cuda.synchronize()
