"""lphy_hip_synthesize / lphy_hip_synthesize_host (csrc/lphy_synth.h) against
the definition in plain numpy float32 (tests/synthesize_model.py, itself
checked by tests/test_synthesize_cpu.py).  The result is a pure function of the
inputs, every operation a float32 one in a fixed order, so every comparison is
on the bytes (where the model has a NaN, a NaN in the same place).  Any SF: the
call does not depend on it (SF 7 here).

K = lphy.SYNTH_TILE outputs make a tile.  A plan takes the LDS path when one
channel group's staged samples fit 64 KiB (lds_path below, the rule of
csrc/lphy_resample_plan.h; tests/cpp/synthesize_check.cpp pins its edge)."""
import numpy as np
import pytest

import synthesize_model as model
from resample_helpers import BIG, EINVAL, ERANGE, _u8, dem, guarded, rand_c64, unguarded  # noqa: F401 (dem: a fixture)

pytestmark = pytest.mark.gpu

PAD = 3        # in_stride = in_samples + PAD
FILL = 0xA5


def lds_bytes(lphy, C_, U, T):
    """synth_lds_bytes of csrc/lphy_resample_plan.h."""
    group = 1
    while group < 8 and group < C_:
        group *= 2
    slots = lphy.SYNTH_TILE // U + (T - 1) // U + 1 + 1
    return group * slots * 8


def lds_path(lphy, C_, U, T):
    """synth_lds_path of csrc/lphy_resample_plan.h."""
    return lds_bytes(lphy, C_, U, T) <= 64 * 1024


def inputs(seed, C_, T, U, n_in, R):
    rng = np.random.default_rng(seed)
    return rand_c64(rng, C_, n_in), rand_c64(rng, C_, T), rand_c64(rng, C_, R)


def covering(first, n_out, U):
    """Narrow samples enough for every output to have all its samples."""
    return (first + n_out - 1) // U + 1


def device_call(lphy, d, x, taps, rot, U, first, n_out, rot_first, fill=FILL, offset8=False, stream=None, skip=0):
    """The device form with the output between guard samples in a buffer
    pre-filled with `fill`, the streams in_samples + PAD apart with NaNs in the
    gaps: the n_out complex64 outputs.  Checks that the guards, the streams and
    the tables are as they were.  `skip`: the call sees the streams from narrow
    sample `skip` on (an advanced d_in)."""
    import torch
    dev = torch.device("cuda", d.device)
    C_, T = taps.shape
    R = rot.shape[1]
    n_in = x.shape[1]
    stride = n_in + PAD
    xs = np.full((C_, stride), np.complex64(np.nan + 1j * np.nan))
    xs[:, :n_in] = x
    xf = xs.view(np.float32).reshape(-1)
    lead = 2 if offset8 else 0  # floats: the samples start 8 bytes into the 16-byte aligned allocation
    t_all = torch.zeros(xf.size + lead, dtype=torch.float32, device=dev)
    t_x = t_all[lead:]
    t_x.copy_(torch.from_numpy(xf.copy()))
    t_taps = torch.from_numpy(taps.view(np.float32).copy()).to(dev)
    t_rot = torch.from_numpy(rot.view(np.float32).copy()).to(dev)
    t_out, o = guarded(dev, n_out * 8, fill, lead=8 if offset8 else 0)
    assert t_all.data_ptr() % 16 == 0 and t_out.data_ptr() % 16 == 0
    if offset8:
        assert t_x.data_ptr() % 16 == 8 and (o.data_ptr() % 16 == 8 or n_out == 0)
    plan = lphy.synth_plan(first, n_in - skip, stride, n_out, rot_first, C_, T, U, R)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    d.synthesize(t_x[2 * skip:], plan, t_taps, t_rot, o, stream=s)
    torch.cuda.synchronize()
    out = unguarded(t_out, n_out * 8, fill, lead=8 if offset8 else 0)
    assert t_x.cpu().numpy().tobytes() == xf.tobytes(), "streams written"
    assert t_taps.cpu().numpy().tobytes() == taps.tobytes() and t_rot.cpu().numpy().tobytes() == rot.tobytes()
    return out.view(np.complex64).copy()


def assert_equal(got, want, what):
    """Bytes, but for NaNs: a NaN where the model has one (its payload is the
    machine's), every other float by its bits."""
    g, w = got.view(np.float32), want.view(np.float32)
    nan = np.isnan(w)
    np.testing.assert_array_equal(np.isnan(g), nan, err_msg=what)
    np.testing.assert_array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan], err_msg=what)


def cases(lphy):
    K = lphy.SYNTH_TILE
    #        C   U    T     first      R  rot_first outputs     LDS path
    return [(1,  1,   1,    0,         1, 0,        2 * K + 37, True),
            (2,  3,   5,    1,         5, BIG,      2 * K + 37, True),    # groups of 2
            (3,  8,   129,  7,         7, BIG,      2 * K + 37, True),    # a group of 4 with 3 channels in it
            (8,  16,  257,  5 * 16 + 3, 5, BIG,     3 * K + 5,  True),
            (9,  16,  129,  0,         7, 6,        2 * K + 37, True),    # a full group and a partial one
            (64, 16,  129,  1,         5, BIG,      2 * K + 37, True),
            (3,  300, 5,    299,       7, BIG,      3 * K + 5,  True),    # U past the tile, T < U
            (8,  300, 257,  5 * 300 + 3, 1, 0,      2 * K + 37, True),
            (2,  300, 129,  0,         5, 4,        K + 1,      True),
            (1,  1,   257,  0,         7, BIG,      2 * K + 37, True),    # a plain FIR
            (8,  1,   129,  5 + 3,     5, BIG,      2 * K + 37, True),
            (9,  3,   257,  2,         7, 6,        2 * K + 37, True),    # T % U != 0
            (4,  8,   5,    0,         1, 0,        2 * K + 37, True),    # T < U: phases without taps
            (1,  16,  1,    15,        5, BIG,      2 * K + 37, True),
            (64, 3,   5,    5 * 3 + 3, 7, BIG,      K + 1,      True),
            (2,  8,   257,  1,         5, BIG,      3 * K + 5,  True),
            (1,  1,   4096, 1,         7, 6,        K + 1,      True),    # the longest filter, still in LDS
            (8,  1,   1025, 3,         7, BIG,      K + 37,     False),   # global path: eight channels' image cannot fit
            (9,  2,   2051, 1,         5, 4,        K + 1,      False),
            (2,  1,   4096, 0,         1, 0,        5,          False),
            (3,  1,   2049, 2,         7, BIG,      K + 1,      False),   # global path with a group of 4, 3 channels in it
            (4,  1,   2048, 0,         5, 4,        K + 1,      False),
            (8,  1,   767,  1,         5, BIG,      K + 1,      True)]    # the LDS path's limit: exactly 64 KiB of dynamic LDS


@pytest.mark.parametrize("k", range(23))
def test_shapes_against_the_model(lphy, dem, k):
    C_, U, T, first, R, rf, n_out, lds = cases(lphy)[k]
    what = f"C={C_} U={U} T={T} first={first} R={R} rot_first={rf} outputs={n_out}"
    assert lds_path(lphy, C_, U, T) == lds, what
    if T == 767:
        assert lds_bytes(lphy, C_, U, T) == 64 * 1024 and not lds_path(lphy, C_, U, T + 1)
    x, taps, rot = inputs(700 + k, C_, T, U, covering(first, n_out, U), R)
    want = model.synthesize(x, taps, rot, U, first, n_out, rf)
    assert_equal(device_call(lphy, dem, x, taps, rot, U, first, n_out, rf), want, what)


def edge_cases(lphy):
    K = lphy.SYNTH_TILE
    #        C  U   T    first n_in outputs
    return [(3, 8,  129, 0,    20,  2 * K + 37),    # past lphy_hip_synthesize_outputs (281): a +0 tail of whole tiles
            (3, 8,  129, 300,  20,  K),             # nothing but the tail
            (2, 16, 257, 0,    40,  K),             # the first outputs reach in front of the stream: j < 0
            (8, 1,  129, 0,    600, 2 * K),
            (3, 8,  129, 5,    1,   K + 1),         # in_samples = 1
            (1, 3,  5,   2,    1,   4),
            (3, 8,  129, 8 * 40 + 3, 100, 1),       # outputs = 1
            (9, 16, 129, 17,   60,  K),
            (9, 16, 129, 17,   60,  K - 1),
            (9, 16, 129, 17,   60,  K + 1),
            (8, 1,  1025, 900, 50,  K + 1),         # global path: j < 0 and a tail
            (3, 1,  1800, 1700, 50, K + 1)]         # the same with a group of 4


@pytest.mark.parametrize("k", range(12))
def test_edges_against_the_model(lphy, dem, k):
    C_, U, T, first, n_in, n_out = edge_cases(lphy)[k]
    what = f"C={C_} U={U} T={T} first={first} in_samples={n_in} outputs={n_out}"
    x, taps, rot = inputs(800 + k, C_, T, U, n_in, 7)
    want = model.synthesize(x, taps, rot, U, first, n_out, BIG)
    reach = lphy.synthesize_outputs(n_in, first, T, U)
    assert reach == model.outputs(n_in, first, T, U)
    if k in (0, 1, 10, 11):
        assert reach < n_out and want[reach:].tobytes() == bytes(8 * (n_out - reach))
    assert_equal(device_call(lphy, dem, x, taps, rot, U, first, n_out, BIG), want, what)


def test_no_input_sample_at_all(lphy, dem):
    """in_samples = 0: d_in is not asked for, every output is (+0, +0)."""
    import torch
    dev = torch.device("cuda", dem.device)
    K = lphy.SYNTH_TILE
    taps, rot = rand_c64(np.random.default_rng(1), 3, 5), rand_c64(np.random.default_rng(2), 3, 7)
    t_taps = torch.from_numpy(taps.view(np.float32).copy()).to(dev)
    t_rot = torch.from_numpy(rot.view(np.float32).copy()).to(dev)
    t_out, o = guarded(dev, (K + 1) * 8, FILL)
    dem.synthesize(None, lphy.synth_plan(3, 0, 0, K + 1, 0, 3, 5, 2, 7), t_taps, t_rot, o,
                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (unguarded(t_out, (K + 1) * 8, FILL) == 0).all()


@pytest.mark.parametrize("C_, U, T, first", [(3, 8, 129, 3), (8, 1, 5, 0), (2, 3, 5, 1), (8, 1, 1025, 2)])
def test_alignment_8_not_16(lphy, dem, C_, U, T, first):
    """d_in and d_out 8 bytes past a 16-byte boundary, for an odd and an even count."""
    K = lphy.SYNTH_TILE
    for n_out in (K + 2, K + 3):
        x, taps, rot = inputs(40 + n_out, C_, T, U, covering(first, n_out, U), 5)
        want = model.synthesize(x, taps, rot, U, first, n_out, 3)
        assert_equal(device_call(lphy, dem, x, taps, rot, U, first, n_out, 3, offset8=True), want,
                     f"C={C_} U={U} T={T} outputs={n_out}")


SPECIALS = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-40, -1e-42, 3e38, -3e38, 1.17549435e-38], np.float32)


@pytest.mark.parametrize("C_, U, T, first", [(3, 4, 9, 0), (2, 3, 5, 0), (5, 4, 4093, 0)])
def test_special_values(lphy, dem, C_, U, T, first):
    """+-inf, NaN, +-0, subnormals and 3e38 in the streams and in the tables,
    inside and at the edges of the tiles, and a NaN tap against the zero operand
    in front of the stream (the definition makes that a NaN).  NaNs are
    compared by position, everything else by its bits: a device that flushed
    subnormals would fail here.  The third plan takes the global path (five
    channels go as a group of eight); its chains are 1,024 samples long, so one infinite sample would leave no finite
    output: it gets the zeros and the subnormals alone, and the NaN tap."""
    K = lphy.SYNTH_TILE
    long_chain = not lds_path(lphy, C_, U, T)
    n_out, R = (K + 3 if long_chain else 2 * K + 3), 5
    assert long_chain == (T == 4093)
    n_in = covering(first, n_out, U)
    x, taps, rot = inputs(31, C_, T, U, n_in, R)
    xf = x.view(np.float32)
    # subnormal results need subnormal factors: scale a stretch of every stream down
    # (twice a chain's length; where the chain is longer than the stream, all of it)
    lo = 0 if long_chain else n_in // 3
    hi = n_in if long_chain else lo + max(6, 2 * ((T - 1) // U + 1))
    assert hi <= n_in
    xf[:, 2 * lo: 2 * hi] *= np.float32(1e-39)
    q0 = first // U
    spots = [q0, q0 + 1, q0 + (K - 1) // U, q0 + K // U, q0 + K // U + 1, q0 + (2 * K - 1) // U, q0 + 2 * K // U,
             n_in - 1, lo + 1, hi - 1]
    spots = sorted({at for at in spots if at < n_in})
    values = SPECIALS[np.isfinite(SPECIALS) & (np.abs(SPECIALS) < 1)] if long_chain else SPECIALS
    for i, at in enumerate(spots):
        c = i % C_
        xf[c, 2 * at + (i & 1)] = values[i % values.size]
        if i % 3 == 0:
            xf[c, 2 * at + 1 - (i & 1)] = values[(i + 4) % values.size]
    tf = taps.view(np.float32)
    tf[1, 2 * 2] = np.float32(1e-39)
    tf[0, 2 * 1 + 1] = np.float32(-0.0)
    # the last tap of channel 1 is NaN; with first = 0 output (T - 1) % U meets it at i = (T - 1) / U >= 1,
    # that is j < 0: a +0 operand
    tf[1, 2 * (T - 1)] = np.float32(np.nan)
    rot.view(np.float32)[1, 3] = np.float32(1e-8)
    want = model.synthesize(x, taps, rot, U, first, n_out, 2)
    w = want.view(np.float32)
    nan = np.isnan(w)
    sub = (np.abs(w) > 0) & (np.abs(w) < np.float32(1.17549435e-38))
    assert nan.any() and sub.any() and (~nan).sum() > nan.sum() // 8, "the inputs do not exercise what they should"
    if first == 0:
        assert T > U and np.isnan(w[2 * ((T - 1) % U)]), "NaN tap times the zero operand at the stream's start"
    assert_equal(device_call(lphy, dem, x, taps, rot, U, first, n_out, 2), want, f"C={C_} U={U} T={T}")


@pytest.mark.parametrize("C_, U, T", [(3, 8, 129), (8, 1, 5), (2, 300, 129), (8, 1, 1025), (3, 1, 2049)])
def test_two_blocks_equal_one_call(lphy, dem, C_, U, T):
    """One transmission in one call, and in two: the second with d_in advanced
    by J0 narrow samples, first = w0 - J0 * U and rot_first advanced by J0, for
    the J0 that suffices, w0 / U - (ceil(T / U) - 1), and for a smaller one."""
    K = lphy.SYNTH_TILE
    total, rf = 2 * K + 91, BIG
    n_in = covering(0, total, U)
    x, taps, rot = inputs(77, C_, T, U, n_in, 7)
    one = device_call(lphy, dem, x, taps, rot, U, 0, total, rf)
    assert_equal(one, model.synthesize(x, taps, rot, U, 0, total, rf), "one call")
    for w0 in (K + 7, K):
        head = device_call(lphy, dem, x, taps, rot, U, 0, w0, rf)
        j0 = max(0, w0 // U - ((T + U - 1) // U - 1))
        for J0 in sorted({j0, j0 // 2}):
            tail = device_call(lphy, dem, x, taps, rot, U, w0 - J0 * U, total - w0, rf + J0, skip=J0)
            np.testing.assert_array_equal(_u8(np.concatenate([head, tail])), _u8(one), err_msg=f"w0={w0} J0={J0}")


def test_second_run_host_form_and_side_stream(lphy, dem):
    import torch
    K = lphy.SYNTH_TILE
    for C_, U, T, first, n_out in [(9, 16, 129, 5, 2 * K + 37), (8, 1, 1025, 1, K + 5)]:
        n_in = covering(first, n_out, U) - 3       # and a short tail
        x, taps, rot = inputs(5, C_, T, U, n_in, 7)
        a = device_call(lphy, dem, x, taps, rot, U, first, n_out, 3, fill=0x00)
        b = device_call(lphy, dem, x, taps, rot, U, first, n_out, 3, fill=0xFF)
        np.testing.assert_array_equal(_u8(a), _u8(b))
        assert_equal(a, model.synthesize(x, taps, rot, U, first, n_out, 3), "device form")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            c = device_call(lphy, dem, x, taps, rot, U, first, n_out, 3, stream=side.cuda_stream)
        np.testing.assert_array_equal(_u8(c), _u8(a))
        host = dem.synthesize_host(x, taps, rot, U, first=first, rot_first=3, outputs=n_out)
        np.testing.assert_array_equal(_u8(host), _u8(a))
        # and with the defaults: every output an input sample reaches
        reach = lphy.synthesize_outputs(n_in, first, T, U)
        all_out = dem.synthesize_host(x, taps, rot, U, first=first, rot_first=3)
        assert all_out.shape == (reach,)
        m = min(reach, n_out)
        np.testing.assert_array_equal(_u8(all_out[:m]), _u8(a[:m]))


def test_outputs_count(lphy):
    for n, first, T, U in [(100, 3, 5, 4), (1, 0, 11, 1), (1, 11, 11, 1), (10, 1000, 3, 3), (1 << 48, 0, 4096, 65536),
                           (0, 0, 5, 1), (5, 0, 0, 1), (5, 0, 1, 0)]:
        assert lphy.synthesize_outputs(n, first, T, U) == model.outputs(n, first, T, U)


def test_return_codes(lphy, dem):
    """Every documented return through the library's entry points, device and
    host form; nothing is written (the sentinel stays), no device call is made
    (the buffers are far smaller than the refused plans describe)."""
    import torch
    dev = torch.device("cuda", dem.device)
    L = dem.lib
    fill = 0x5A
    t_x = torch.zeros(2 * 64, dtype=torch.float32, device=dev)
    t_taps = torch.zeros(2 * 64 * 8, dtype=torch.float32, device=dev)
    t_rot = torch.zeros(2 * 64 * 8, dtype=torch.float32, device=dev)
    t_out = torch.full((8 * 64,), fill, dtype=torch.uint8, device=dev)
    h_x, h_taps, h_rot = np.zeros(64, np.complex64), np.zeros(512, np.complex64), np.zeros(512, np.complex64)
    h_out = np.full(64, np.complex64(3 + 4j))
    ok = dict(first=1, in_samples=10, in_stride=12, outputs=30, rot_first=0, channels=3, taps=5, interp=4,
              rot_period=7)
    k32, k48 = 1 << 32, 1 << 48

    def both(want, ctx=True, null=(), off=(), plan=True, **changes):
        p = lphy.synth_plan(**dict(ok, **changes))
        pp = p.ctypes.data if plan else None
        c = dem.ctx if ctx else None
        dptr = dict(x=t_x.data_ptr(), taps=t_taps.data_ptr(), rot=t_rot.data_ptr(), out=t_out.data_ptr())
        hptr = dict(x=h_x.ctypes.data, taps=h_taps.ctypes.data, rot=h_rot.ctypes.data, out=h_out.ctypes.data)
        for ptr in (dptr, hptr):
            for n in null:
                ptr[n] = None
            for n in off:
                ptr[n] += 4
        assert L.lphy_hip_synthesize(c, dptr["x"], pp, dptr["taps"], dptr["rot"], dptr["out"], None) == want, changes
        assert L.lphy_hip_synthesize_host(c, hptr["x"], pp, hptr["taps"], hptr["rot"], hptr["out"]) == want, changes

    both(EINVAL, ctx=False)
    both(EINVAL, plan=False)
    both(EINVAL, null=("taps",))
    both(EINVAL, null=("rot",))
    both(EINVAL, null=("out",))
    both(EINVAL, null=("x",))
    for n in ("x", "taps", "rot", "out"):
        both(EINVAL, off=(n,))
    both(EINVAL, reserved=(1, 0))
    both(EINVAL, reserved=(0, 1))
    for n in ("channels", "taps", "interp", "rot_period"):
        both(EINVAL, **{n: 0})
    # the order: -EINVAL in front of every -ERANGE, a null pointer in front of a bad plan
    both(EINVAL, channels=65, reserved=(0, 1))
    both(EINVAL, taps=5000, interp=0)
    both(EINVAL, off=("rot",), in_stride=1)
    both(EINVAL, null=("out",), outputs=k32)
    both(ERANGE, channels=65)
    both(ERANGE, taps=4097)
    both(ERANGE, interp=65537)
    both(ERANGE, rot_period=65537)
    both(ERANGE, outputs=k32)
    both(ERANGE, in_stride=9)
    both(ERANGE, in_samples=k48 + 1, in_stride=k48 + 1)
    both(ERANGE, in_stride=k48 // 3 + 1)
    both(ERANGE, in_stride=(1 << 64) - 1)
    both(ERANGE, first=k48 - 29)
    both(ERANGE, first=(1 << 64) - 30)
    torch.cuda.synchronize()
    assert (t_out.cpu().numpy() == fill).all() and (h_out == np.complex64(3 + 4j)).all()
    # outputs == 0: returns 0, launches nothing, asks for neither the samples nor the output
    both(0, outputs=0)
    both(0, outputs=0, null=("x", "out"), first=k48)
    both(ERANGE, outputs=0, channels=65)
    # in_samples == 0: the samples are not asked for
    both(0, in_samples=0, null=("x",))
    # and a legal call on these buffers goes through, at the limits' edge for first
    both(0)
    both(0, first=k48 - 30)
    torch.cuda.synchronize()
    assert (t_out.cpu().numpy()[8 * 30:] == fill).all() and (t_out.cpu().numpy()[: 8 * 30] == 0).all()
    assert (h_out[30:] == np.complex64(3 + 4j)).all() and (h_out[:30] == 0).all()


def test_binding_checks_the_tensors(lphy, dem):
    import torch
    dev = torch.device("cuda", dem.device)
    z = lambda n: torch.zeros(2 * n, dtype=torch.float32, device=dev)  # noqa: E731
    p = lphy.synth_plan(0, 10, 12, 24, 0, 2, 5, 4, 3)
    dem.synthesize(z(22), p, z(10), z(6), z(24))     # the last stream may stop at in_samples
    for bad in [(z(21), z(10), z(6), z(24)), (z(22), z(9), z(6), z(24)), (z(22), z(10), z(5), z(24)),
                (z(22), z(10), z(6), z(23)), (z(22).cpu(), z(10), z(6), z(24)), (None, z(10), z(6), z(24))]:
        with pytest.raises(ValueError):
            dem.synthesize(bad[0], p, bad[1], bad[2], bad[3])
    torch.cuda.synchronize()
