"""lphy_hip_channelize_raw / lphy_hip_channelize_raw_host (csrc/lphy_chan.h with
the capture's format as a template parameter) against the definition: what
lphy_hip_channelize gives on the capture converted to float32
(tests/sample_formats.py to_float, tests/channelize_model.py).  The conversion
is exact and the arithmetic behind it is the float form's, so every comparison
is on the bytes.  SF 7; the call does not depend on it.

B = bytes of a sample (4: SC16, 2: SC8 and CU8), V = 16 / B samples of one
16-byte load of the staging.  K = lphy.CHAN_TILE outputs make a tile."""
import numpy as np
import pytest

import channelize_model as model
import sample_formats as sf
from resample_helpers import BIG, EINVAL, ERANGE, _u8, dem, guarded, rand_c64, unguarded  # noqa: F401 (dem: a fixture)
from test_gpu_channelize import PAD, assert_output, cases
from test_gpu_channelize import device_call as float_call

pytestmark = pytest.mark.gpu

INT_FORMATS = pytest.mark.parametrize("fmt", sf.INT_FORMATS, ids=[sf.NAMES[f] for f in sf.INT_FORMATS])


def torch_dtype(fmt):
    import torch
    return {sf.FMT_CF32: torch.float32, sf.FMT_SC16: torch.int16, sf.FMT_SC8: torch.int8, sf.FMT_CU8: torch.uint8}[fmt]


def capture_tensor(dev, x, fmt, offset=0):
    """The capture `x` ([n, 2] or flat, fmt's dtype) on the device, `offset`
    bytes into a 16-byte aligned allocation, as a tensor of fmt's type."""
    import torch
    raw = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    whole = torch.zeros(offset + raw.size, dtype=torch.uint8, device=dev)
    assert whole.data_ptr() % 16 == 0
    t = whole[offset:]
    t.copy_(torch.from_numpy(raw.copy()))
    t = t.view(torch_dtype(fmt))
    assert t.data_ptr() % 16 == offset % 16 and t.numel() == np.asarray(x).size
    return t


def device_call(lphy, d, x, fmt, taps, rot, D, first, n_out, rot_first, fill=0xA5, offset=0):
    """The device form on the capture `x` of format `fmt`, the output between
    guard samples and everything pre-filled with `fill`: the [C, out_stride]
    complex64 output as left."""
    import torch
    dev = torch.device("cuda", d.device)
    C_, T = taps.shape
    R = rot.shape[1]
    stride = n_out + PAD
    t_x = capture_tensor(dev, x, fmt, offset)
    t_taps = torch.from_numpy(taps.view(np.float32).copy()).to(dev)
    t_rot = torch.from_numpy(rot.view(np.float32).copy()).to(dev)
    t_all_out, t_out = guarded(dev, C_ * stride * 8, fill)
    plan = lphy.chan_plan(first, np.asarray(x).size // 2, n_out, stride, rot_first, C_, T, D, R)
    d.channelize_raw(t_x, fmt, plan, t_taps, t_rot, t_out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return unguarded(t_all_out, C_ * stride * 8, fill).view(np.complex64).reshape(C_, stride).copy()


def inputs(seed, fmt, C_, T, D, n_out, first, R, extra=2):
    """(capture [n, 2] of fmt over its whole range, taps, rot)"""
    rng = np.random.default_rng(seed)
    n = first + (n_out - 1) * D + T + extra if n_out else first + extra
    return sf.random_capture(rng, n, fmt), rand_c64(rng, C_, T), rand_c64(rng, C_, R)


@INT_FORMATS
def test_head_body_and_tail_of_the_staging(lphy, dem, fmt):
    """One output of one channel whose T taps are the whole span, n = T = 1 ..
    2V + 1 samples, at every offset of the capture within 16 bytes and `first`
    0 and 1: heads of 0 .. V - 1 samples, the spans shorter than their head
    among them, 0 .. 2 loads, tails of 0 .. V - 1."""
    B = sf.BYTES[fmt]
    V = 16 // B
    rng = np.random.default_rng(40 + fmt)
    x = sf.random_capture(rng, 2 * V + 2, fmt)
    xf = sf.to_float(x, fmt)
    rot = rand_c64(rng, 1, 1)
    short = 0
    for n in range(1, 2 * V + 2):
        taps = rand_c64(rng, 1, n)
        for first in (0, 1):
            want = model.channelize(xf, taps, rot, 1, first, 1, 0)
            for offset in range(0, 16, B):
                head = ((16 - (offset + first * B) % 16) % 16) // B
                short += n < head
                got = device_call(lphy, dem, x, fmt, taps, rot, 1, first, 1, 0, offset=offset)
                assert_output(got, want, 1, 0xA5, f"{sf.NAMES[fmt]} n={n} first={first} offset={offset} head={head}")
    assert short > 0  # the spans shorter than their head were among them


@INT_FORMATS
@pytest.mark.parametrize("k", [3, 4, 13, 17, 19, 23])
def test_tiles_against_the_model(lphy, dem, fmt, k):
    """Rows of test_gpu_channelize.cases(): full, partial and several tiles (3,
    4), a group of 8 with 5 channels (13), the global path (17, 19), the
    largest decimation (23).  D = 7 or 40 and `first` odd put every tile's span
    on another offset."""
    C_, T, D, n_out, first, R, rf = cases(lphy)[k]
    what = f"{sf.NAMES[fmt]} C={C_} T={T} D={D} outputs={n_out} first={first} R={R} rot_first={rf}"
    x, taps, rot = inputs(600 + k, fmt, C_, T, D, n_out, first, R)
    want = model.channelize(sf.to_float(x, fmt), taps, rot, D, first, n_out, rf)
    assert_output(device_call(lphy, dem, x, fmt, taps, rot, D, first, n_out, rf), want, n_out, 0xA5, what)


IDENTITY = np.ones((1, 1), np.complex64)


def as_converter(lphy, d, x, fmt, n_out, **kw):
    """The identity plan (T = D = C = R = 1, taps = rot = (1, 0)) and the same
    with taps = (2^-15, 0): the outputs, which must be to_float(x) and
    to_float(x) / 32768 on the bytes."""
    xf = sf.to_float(x, fmt)[:n_out]
    for g, want in [(1.0, xf), (2.0 ** -15, (xf.view(np.float32) / np.float32(32768)).view(np.complex64))]:
        got = device_call(lphy, d, x, fmt, IDENTITY * np.float32(g), IDENTITY, 1, 0, n_out, 0, **kw)
        assert want.dtype == np.complex64
        assert_output(got, want.reshape(1, -1), n_out, 0xA5, f"{sf.NAMES[fmt]} g={g}")


@pytest.mark.parametrize("fmt", [sf.FMT_SC8, sf.FMT_CU8], ids=["sc8", "cu8"])
def test_every_8_bit_value(lphy, dem, fmt):
    """All 256 bytes in I and, in another order, in Q."""
    b = np.arange(256, dtype=np.uint8)
    x = np.stack([b, (b * 37 + 11).astype(np.uint8)], axis=1).view(sf.DTYPES[fmt])
    assert np.unique(x[:, 0]).size == np.unique(x[:, 1]).size == 256
    for offset in (0, 6):
        as_converter(lphy, dem, x, fmt, 256, offset=offset)


def test_sc16_extremes_at_the_tile_edges(lphy, dem):
    """-32768, -32767, -1, 0, 1, 32766, 32767 at a tile's first sample, its
    last, and on both sides of the tile edges (output m is sample m here)."""
    K = lphy.CHAN_TILE
    n_out = 2 * K + 3
    v = np.array([-32768, -32767, -1, 0, 1, 32766, 32767], "<i2")
    spots = [0, 1, K - 2, K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 2]
    for r in range(v.size):
        x = sf.random_capture(np.random.default_rng(r), n_out, sf.FMT_SC16)
        for j, at in enumerate(spots):
            x[at] = (v[(j + r) % v.size], v[(j + r + 3) % v.size])
        as_converter(lphy, dem, x, sf.FMT_SC16, n_out, offset=4 * (r % 4))


@INT_FORMATS
@pytest.mark.parametrize("k", [4, 19])
def test_the_float_form_is_the_definition(lphy, dem, fmt, k):
    """An LDS-path and a global-path row: channelize_raw on the integers and
    channelize on to_float(x) uploaded as float32 leave the same bytes."""
    C_, T, D, n_out, first, R, rf = cases(lphy)[k]
    x, taps, rot = inputs(700 + k, fmt, C_, T, D, n_out, first, R)
    a = device_call(lphy, dem, x, fmt, taps, rot, D, first, n_out, rf)
    b = float_call(lphy, dem, sf.to_float(x, fmt), taps, rot, D, first, n_out, rf)
    np.testing.assert_array_equal(_u8(a), _u8(b))


@pytest.mark.parametrize("k", [4, 19])
@pytest.mark.parametrize("offset", [0, 8])
def test_cf32_is_channelize_itself(lphy, dem, k, offset):
    C_, T, D, n_out, first, R, rf = cases(lphy)[k]
    x, taps, rot = inputs(800 + k, sf.FMT_CF32, C_, T, D, n_out, first, R)
    a = device_call(lphy, dem, x, sf.FMT_CF32, taps, rot, D, first, n_out, rf, offset=offset)
    b = float_call(lphy, dem, sf.to_float(x, sf.FMT_CF32), taps, rot, D, first, n_out, rf, offset8=bool(offset))
    np.testing.assert_array_equal(_u8(a), _u8(b))
    assert_output(a, model.channelize(sf.to_float(x, sf.FMT_CF32), taps, rot, D, first, n_out, rf), n_out, 0xA5, "cf32")


@pytest.mark.parametrize("fmt", [sf.FMT_SC16, sf.FMT_CU8], ids=["sc16", "cu8"])
@pytest.mark.parametrize("T, D", [(67, 16), (2, 7)])
def test_blocks_equal_one_call(lphy, dem, fmt, T, D):
    """One capture in one call, and in three calls with `first` and rot_first
    advanced: the same bytes."""
    K = lphy.CHAN_TILE
    counts = [K + 7, 2 * K - 1, 40]
    total = sum(counts)
    x, taps, rot = inputs(77, fmt, 3, T, D, total, 0, 7, extra=0)
    one = device_call(lphy, dem, x, fmt, taps, rot, D, 0, total, 5)[:, :total]
    np.testing.assert_array_equal(_u8(one), _u8(model.channelize(sf.to_float(x, fmt), taps, rot, D, 0, total, 5)))
    parts, m0 = [], 0
    for n in counts:
        parts.append(device_call(lphy, dem, x, fmt, taps, rot, D, m0 * D, n, 5 + m0)[:, :n])
        m0 += n
    np.testing.assert_array_equal(_u8(np.concatenate(parts, axis=1)), _u8(one))


@pytest.mark.parametrize("fmt", [sf.FMT_SC16, sf.FMT_SC8], ids=["sc16", "sc8"])
def test_result_does_not_depend_on_the_output_buffer(lphy, dem, fmt):
    K = lphy.CHAN_TILE
    x, taps, rot = inputs(5, fmt, 8, 67, 16, K + 9, 1, 7)
    a = device_call(lphy, dem, x, fmt, taps, rot, 16, 1, K + 9, 3, fill=0x00)
    b = device_call(lphy, dem, x, fmt, taps, rot, 16, 1, K + 9, 3, fill=0xFF)
    np.testing.assert_array_equal(_u8(a[:, :K + 9]), _u8(b[:, :K + 9]))
    assert (_u8(a[:, K + 9:]) == 0x00).all() and (_u8(b[:, K + 9:]) == 0xFF).all()


@pytest.mark.parametrize("fmt, k", [(sf.FMT_SC16, 4), (sf.FMT_SC8, 12), (sf.FMT_CU8, 21), (sf.FMT_CF32, 12)],
                         ids=["sc16", "sc8", "cu8", "cf32"])
def test_host_form_equals_the_device_form(lphy, dem, fmt, k):
    C_, T, D, n_out, first, R, rf = cases(lphy)[k]
    x, taps, rot = inputs(500 + k, fmt, C_, T, D, n_out, first, R)
    got = device_call(lphy, dem, x, fmt, taps, rot, D, first, n_out, rf)[:, :n_out]
    out = np.full((C_, n_out + PAD), np.complex64(7 - 7j))
    host = dem.channelize_raw_host(x, fmt, taps, rot, D, first=first, outputs=n_out, rot_first=rf, out=out)
    np.testing.assert_array_equal(_u8(host), _u8(got))
    assert (out[:, n_out:] == np.complex64(7 - 7j)).all()
    # the defaults: every output the capture holds; and the flat layout
    n = x.shape[0]
    all_out = dem.channelize_raw_host(x, fmt, taps, rot, D, first=first, rot_first=rf)
    assert all_out.shape == (C_, lphy.channelize_outputs(n, first, T, D)) and all_out.shape[1] >= n_out
    np.testing.assert_array_equal(_u8(all_out[:, :n_out]), _u8(got))
    flat = dem.channelize_raw_host(x.reshape(-1), fmt, taps, rot, D, first=first, rot_first=rf)
    np.testing.assert_array_equal(_u8(flat), _u8(all_out))
    for bad in (x.reshape(-1)[:-1], x.astype(np.int32), x.reshape(-1, 2, 1)):
        with pytest.raises(ValueError):
            dem.channelize_raw_host(bad, fmt, taps, rot, D)


def test_sample_bytes(lphy):
    assert [lphy.sample_bytes(f) for f in (lphy.FMT_CF32, lphy.FMT_SC16, lphy.FMT_SC8, lphy.FMT_CU8)] == [8, 4, 2, 2]
    assert lphy.sample_bytes(-1) == 0 and lphy.sample_bytes(4) == 0


def test_return_codes(lphy, dem):
    """Every row of lphy_hip_channelize's table once with SC16, and the new
    rows (the format, d_in's alignment by format, their place in the order),
    through the device and the host entry point; nothing is written (the
    sentinel stays), no device call is made (the buffers are far smaller than
    the refused plans describe)."""
    import torch
    dev = torch.device("cuda", dem.device)
    L = dem.lib
    FILL = 0x5A
    t_x = torch.zeros(8 * 64, dtype=torch.uint8, device=dev)
    t_taps = torch.zeros(2 * 64 * 8, dtype=torch.float32, device=dev)
    t_rot = torch.zeros(2 * 64 * 8, dtype=torch.float32, device=dev)
    t_out = torch.full((8 * 64,), FILL, dtype=torch.uint8, device=dev)
    h_x, h_taps, h_rot = np.zeros(64, np.complex64), np.zeros(512, np.complex64), np.zeros(512, np.complex64)
    h_out = np.full(64, np.complex64(3 + 4j))
    assert t_x.data_ptr() % 16 == 0 and h_x.ctypes.data % 8 == 0
    ok = dict(first=1, in_samples=64, outputs=8, out_stride=10, rot_first=0, channels=3, taps=5, decim=4, rot_period=7)
    k32, k48 = 1 << 32, 1 << 48

    def both(want, fmt=sf.FMT_SC16, ctx=True, null=(), off=(), by=4, plan=True, **changes):
        p = lphy.chan_plan(**dict(ok, **changes))
        pp = p.ctypes.data if plan else None
        c = dem.ctx if ctx else None
        dptr = dict(x=t_x.data_ptr(), taps=t_taps.data_ptr(), rot=t_rot.data_ptr(), out=t_out.data_ptr())
        hptr = dict(x=h_x.ctypes.data, taps=h_taps.ctypes.data, rot=h_rot.ctypes.data, out=h_out.ctypes.data)
        for ptr in (dptr, hptr):
            for n in null:
                ptr[n] = None
            for n in off:
                ptr[n] += by
        what = (fmt, null, off, by, changes)
        rc = L.lphy_hip_channelize_raw(c, dptr["x"], fmt, pp, dptr["taps"], dptr["rot"], dptr["out"], None)
        assert rc == want, ("device form", rc, what)
        rc = L.lphy_hip_channelize_raw_host(c, hptr["x"], fmt, pp, hptr["taps"], hptr["rot"], hptr["out"])
        assert rc == want, ("host form", rc, what)

    # lphy_hip_channelize's table, with SC16
    both(EINVAL, ctx=False)
    both(EINVAL, plan=False)
    both(EINVAL, null=("taps",))
    both(EINVAL, null=("rot",))
    both(EINVAL, null=("x",))
    both(EINVAL, null=("out",))
    both(EINVAL, off=("x",), by=2)
    for n in ("taps", "rot", "out"):
        both(EINVAL, off=(n,))
    both(EINVAL, reserved=(1, 0))
    both(EINVAL, reserved=(0, 1))
    for n in ("channels", "taps", "decim", "rot_period"):
        both(EINVAL, **{n: 0})
    both(EINVAL, channels=65, reserved=(0, 1))
    both(EINVAL, taps=5000, decim=0)
    both(EINVAL, off=("rot",), out_stride=1)
    both(EINVAL, null=("out",), in_samples=3)
    ranges = [dict(channels=65), dict(taps=4097), dict(decim=65537), dict(rot_period=65537),
              dict(outputs=k32, out_stride=k32), dict(out_stride=7), dict(in_samples=k48 + 1),
              dict(in_samples=1 + 7 * 4 + 5 - 1), dict(first=(1 << 64) - 30), dict(first=65),
              dict(out_stride=k48 // 3 + 1), dict(out_stride=(1 << 64) - 1)]
    for ch in ranges:
        both(ERANGE, **ch)
    # the new rows.  A format that is none of the four: -EINVAL, in front of a misaligned pointer and of every -ERANGE
    for fmt in (-1, 4, 255):
        both(EINVAL, fmt=fmt)
        both(EINVAL, fmt=fmt, off=("x",), by=1)
        both(EINVAL, fmt=fmt, outputs=0, out_stride=0, null=("x", "out"))
        for ch in ranges:
            both(EINVAL, fmt=fmt, **ch)
    # d_in is asked for its sample's bytes, the other three for 8
    for fmt, legal in [(sf.FMT_CF32, (8,)), (sf.FMT_SC16, (4, 8, 12)), (sf.FMT_SC8, (2, 4, 6, 8, 12, 14)),
                       (sf.FMT_CU8, (2, 4, 6, 8, 12, 14))]:
        for by in (1, 2, 3, 4, 6, 8, 12, 14):
            both(0 if by in legal else EINVAL, fmt=fmt, off=("x",), by=by, outputs=0, out_stride=0)
            # in front of -ERANGE when it refuses, behind nothing that passes
            both(ERANGE if by in legal else EINVAL, fmt=fmt, off=("x",), by=by, channels=65)
        for n in ("taps", "rot", "out"):
            both(EINVAL, fmt=fmt, off=(n,), by=4)
            both(EINVAL, fmt=fmt, off=(n,), by=2)
    torch.cuda.synchronize()
    assert (t_out.cpu().numpy() == FILL).all() and (h_out == np.complex64(3 + 4j)).all()
    # outputs == 0: returns 0, launches nothing, asks for neither the samples nor the output
    both(0, outputs=0, out_stride=0)
    both(0, outputs=0, null=("x", "out"), first=1000)
    both(ERANGE, outputs=0, channels=65)
    # and a legal call on these buffers goes through, in every format, off a 16-byte boundary: the plan's edge
    for fmt in (sf.FMT_CF32, *sf.INT_FORMATS):
        t_out.fill_(FILL)
        both(0, fmt=fmt, in_samples=1 + 7 * 4 + 5, off=("x",), by=sf.BYTES[fmt])
        torch.cuda.synchronize()
        o = t_out.cpu().numpy()  # the tables are zeros, so every output is (+0, +0)
        assert (o[8 * 30:] == FILL).all() and (o[: 8 * 8] == 0).all()


def test_binding_checks_the_tensors(lphy, dem):
    import torch
    dev = torch.device("cuda", dem.device)
    z = lambda n, dt=torch.float32: torch.zeros(2 * n, dtype=dt, device=dev)  # noqa: E731
    p = lphy.chan_plan(0, 100, 24, 24, 0, 2, 5, 4, 3)
    for fmt in (sf.FMT_CF32, *sf.INT_FORMATS):
        dt = torch_dtype(fmt)
        dem.channelize_raw(z(100, dt), fmt, p, z(10), z(6), z(48))
        others = [torch_dtype(f) for f in (sf.FMT_CF32, *sf.INT_FORMATS) if f != fmt] + [torch.int32, torch.float16]
        bad = [(z(100, o), z(10), z(6), z(48)) for o in others]
        bad += [(z(99, dt), z(10), z(6), z(48)), (z(101, dt), z(10), z(6), z(48)), (z(100, dt), z(9), z(6), z(48)),
                (z(100, dt), z(10), z(5), z(48)), (z(100, dt), z(10), z(6), z(47)),
                (z(100, dt).cpu(), z(10), z(6), z(48))]
        for b in bad:
            with pytest.raises(ValueError):
                dem.channelize_raw(b[0], fmt, p, b[1], b[2], b[3])
    with pytest.raises(ValueError):
        dem.channelize_raw(z(100), 4, p, z(10), z(6), z(48))
    torch.cuda.synchronize()
