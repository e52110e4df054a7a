"""GPU batch forms of the LoRaCodes.hpp helpers (csrc/lphy_codes.hip, SURVEY
8f rank 3) against the CPU oracle (pinned to the reference header by
test_oracle_vs_reference.py): Gray mapping over every 16-bit value, every
Hamming / parity op over every byte with its flags, the diagonal
(de)interleaver for the SX127x geometries (ppm 5..12, rdd 0..4) on batches
of frames with strides, the three whitening generators at several bit
offsets, and the checksums — bit for bit, row by row.  The second half of the
file covers what the header admits beyond that: every ppm 1..16 and rdd 0..4
on full-width input, whitening across and far past the generators' periods
(bit_ofs up to INT_MAX), lora_encode_batch on its own, element and thread
counts around the workgroup size, untouched tails, every documented return
code, and the calls in stream order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def test_gpu_gray_all_values(oracle, lphy, torch_dev):
    torch, dev = torch_dev
    v = np.arange(65536, dtype=np.uint16)
    for tb in (0, 1):
        t = torch.from_numpy(v.view(np.int16).copy()).to(dev)
        lphy.gray_batch(t, tb)
        got = t.cpu().numpy().view(np.uint16)
        want = np.array([oracle.gray(int(x), tb) for x in v[::1]], np.uint16)
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("op", range(8))
def test_gpu_hamming_all_bytes(oracle, lphy, torch_dev, op):
    torch, dev = torch_dev
    x = np.tile(np.arange(256, dtype=np.uint8), 37)
    t = torch.from_numpy(x.copy()).to(dev)
    fl = torch.zeros(x.size, dtype=torch.uint8, device=dev)
    lphy.hamming_batch(t, op, fl)
    got, gfl = t.cpu().numpy(), fl.cpu().numpy()
    for i in range(256):
        o, f = oracle.hamming(i, op)
        assert got[i] == o and gfl[i] == f, (i, op)
    np.testing.assert_array_equal(got.reshape(37, 256), np.tile(got[:256], (37, 1)))


@pytest.mark.parametrize("ppm,rdd", [(p, r) for p in (5, 7, 8, 10, 12) for r in (0, 1, 2, 4)])
def test_gpu_interleaver_batch(oracle, lphy, torch_dev, ppm, rdd):
    torch, dev = torch_dev
    rng = np.random.default_rng(ppm * 10 + rdd)
    frames, ncw = 301, 5 * ppm + 3
    cw_stride, sym_stride = ncw + 5, (ncw // ppm) * (4 + rdd) + 3
    cw = rng.integers(0, 1 << (4 + rdd), (frames, cw_stride), dtype=np.uint8)
    tcw = torch.from_numpy(cw.copy()).to(dev)
    tsy = torch.full((frames, sym_stride), -1, dtype=torch.int16, device=dev)
    lphy.interleave_batch(tcw, frames, cw_stride, ncw, tsy, sym_stride, ppm, rdd)
    sy = tsy.cpu().numpy().view(np.uint16)
    nsy = (ncw // ppm) * (4 + rdd)
    for f in range(frames):
        np.testing.assert_array_equal(sy[f, :nsy], oracle.interleave(cw[f, :ncw], ppm, rdd))
        assert (sy[f, nsy:] == 0xFFFF).all()  # past the row's blocks: untouched
    # deinterleave random symbols (and back to the codewords above)
    rs = rng.integers(0, 1 << ppm, (frames, sym_stride), dtype=np.uint16)
    trs = torch.from_numpy(rs.view(np.int16).copy()).to(dev)
    tout = torch.full((frames, cw_stride), 0xAB, dtype=torch.uint8, device=dev)
    lphy.deinterleave_batch(trs, frames, sym_stride, nsy, tout, cw_stride, ppm, rdd)
    out = tout.cpu().numpy()
    for f in range(frames):
        np.testing.assert_array_equal(out[f, : (nsy // (4 + rdd)) * ppm], oracle.deinterleave(rs[f, :nsy], ppm, rdd))
    lphy.deinterleave_batch(tsy, frames, sym_stride, nsy, tout, cw_stride, ppm, rdd)
    np.testing.assert_array_equal(tout.cpu().numpy()[:, : (ncw // ppm) * ppm], cw[:, : (ncw // ppm) * ppm])


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_gpu_whitening_and_checksums(oracle, lphy, torch_dev, kind):
    torch, dev = torch_dev
    rng = np.random.default_rng(60 + kind)
    frames, length, stride = 513, 200, 211
    buf = rng.integers(0, 256, (frames, stride), dtype=np.uint8)
    for rdd in (0, 1, 4):
        for bit_ofs in (0, 3, 100):
            t = torch.from_numpy(buf.copy()).to(dev)
            lphy.whiten_batch(t, frames, stride, length, kind, bit_ofs, rdd)
            got = t.cpu().numpy()
            for f in range(0, frames, 37):
                np.testing.assert_array_equal(got[f, :length], oracle.whiten(buf[f, :length], kind, bit_ofs, rdd))
            np.testing.assert_array_equal(got[:, length:], buf[:, length:])
            lphy.whiten_batch(t, frames, stride, length, kind, bit_ofs, rdd)  # involution
            np.testing.assert_array_equal(t.cpu().numpy(), buf)
    out = torch.zeros(frames, dtype=torch.int16, device=dev)
    t = torch.from_numpy(buf.copy()).to(dev)
    lphy.checksum_batch(t, frames, stride, length, kind, out)
    got = out.cpu().numpy().view(np.uint16)
    for f in range(frames):
        assert got[f] == oracle.checksum(buf[f, :length] if kind != 1 else buf[f, :2], kind), f


# --------------------------------------------------------------------------
# The whole parameter space the header admits.  Every row of every call is
# compared with the oracle, byte for byte; outputs start from a sentinel and
# everything outside what the call documents as written must keep it.
W = 256                                     # the kernels' workgroup size
BOUNDARY = (1, W - 1, W, W + 1, 3 * W + 5)  # element / thread totals around it
EINVAL, ERANGE = -22, -34
INT_MAX = (1 << 31) - 1
S8, S16 = 0xAB, 0xA5C3                      # sentinels


def _dev8(torch, dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8).copy()).to(dev)


def _dev16(torch, dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16).copy()).to(dev)


def _host16(t):
    return t.cpu().numpy().view(np.uint16)


def _whiten_rows(oracle, buf, length, kind, bit_ofs, rdd):
    """The oracle on the first `length` bytes of every row; the tail as it was."""
    want = buf.copy()
    for f in range(buf.shape[0]):
        want[f, :length] = oracle.whiten(buf[f, :length], kind, bit_ofs, rdd)
    return want


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("kind", [1, 2])
def test_gpu_whiten_across_periods(oracle, lphy, torch_dev, kind, frames):
    """Rows of 600 bytes cross the 510-position period of both SX1272
    generators at every offset; offsets at, around and several times past it."""
    torch, dev = torch_dev
    length, stride = 600, 605
    buf = np.random.default_rng(700 + 10 * kind + frames).integers(0, 256, (frames, stride), dtype=np.uint8)
    for rdd in range(5):
        for bit_ofs in (0, 1, 3, 100, 503, 504, 509, 510, 511, 1019, 1020, 1021, 5103):
            t = _dev8(torch, dev, buf)
            lphy.whiten_batch(t, frames, stride, length, kind, bit_ofs, rdd)
            got = t.cpu().numpy()
            want = _whiten_rows(oracle, buf, length, kind, bit_ofs, rdd)
            np.testing.assert_array_equal(got, want, str((rdd, bit_ofs)))   # the tails too: untouched
            # only the 4 + rdd codeword bits are whitened, the data's high bits stay
            assert not ((got ^ buf) & (0xFF ^ (0xFF >> (4 - rdd)))).any()
            lphy.whiten_batch(t, frames, stride, length, kind, bit_ofs, rdd)  # involution
            np.testing.assert_array_equal(t.cpu().numpy(), buf)


def test_gpu_whiten_sx1232_ignores_offset_and_rdd(oracle, lphy, torch_dev):
    torch, dev = torch_dev
    frames, length, stride = 3, 600, 605
    buf = np.random.default_rng(711).integers(0, 256, (frames, stride), dtype=np.uint8)
    want = _whiten_rows(oracle, buf, length, 0, 0, 0)
    for bit_ofs, rdd in ((0, 0), (777, 3), (5103, 4), (1, 200)):   # rdd is not even range-checked here
        t = _dev8(torch, dev, buf)
        lphy.whiten_batch(t, frames, stride, length, 0, bit_ofs, rdd)
        np.testing.assert_array_equal(t.cpu().numpy(), want, str((bit_ofs, rdd)))
        lphy.whiten_batch(t, frames, stride, length, 0, bit_ofs, rdd)
        np.testing.assert_array_equal(t.cpu().numpy(), buf)


def test_gpu_whiten_sx1232_longest_row(oracle, lphy, torch_dev):
    """len 65,535, the longest the call admits: byte j is 8 * j steps of the
    9-bit LFSR from its seed, reduced by the period of 511 in the kernel."""
    torch, dev = torch_dev
    length, stride = 65535, 65535 + 5
    buf = np.random.default_rng(712).integers(0, 256, (1, stride), dtype=np.uint8)
    t = _dev8(torch, dev, buf)
    lphy.whiten_batch(t, 1, stride, length, 0, 9, 2)
    np.testing.assert_array_equal(t.cpu().numpy(), _whiten_rows(oracle, buf, length, 0, 0, 0))


@pytest.mark.parametrize("kind", [1, 2])
def test_gpu_whiten_large_offsets(oracle, lphy, torch_dev, kind):
    """bit_ofs up to INT_MAX: the bytes of the same call at bit_ofs % 510, which
    are the oracle's there (the oracle's own int arithmetic does not reach the
    large values, so it is never given them)."""
    torch, dev = torch_dev
    frames, length, stride = 2, 1024, 1024 + 5
    buf = np.random.default_rng(720 + kind).integers(0, 256, (frames, stride), dtype=np.uint8)
    for rdd in (1, 4):
        for bit_ofs in (INT_MAX, INT_MAX - 509, INT_MAX - 65535, 1 << 30):
            small = bit_ofs % 510
            t, u = _dev8(torch, dev, buf), _dev8(torch, dev, buf)
            lphy.whiten_batch(t, frames, stride, length, kind, bit_ofs, rdd)
            lphy.whiten_batch(u, frames, stride, length, kind, small, rdd)
            got = t.cpu().numpy()
            np.testing.assert_array_equal(got, u.cpu().numpy(), str((rdd, bit_ofs)))
            np.testing.assert_array_equal(got, _whiten_rows(oracle, buf, length, kind, small, rdd), str((rdd, bit_ofs)))


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_gpu_whiten_shortest_rows_and_full_stride(oracle, lphy, torch_dev, kind):
    torch, dev = torch_dev
    rng = np.random.default_rng(730 + kind)
    for frames, length, stride in ((3, 0, 4), (3, 1, 4), (W + 1, 1, 1), (3, 7, 7), (1, W, W), (W - 1, 1, 2)):
        buf = rng.integers(0, 256, (frames, stride), dtype=np.uint8)
        t = _dev8(torch, dev, buf)
        lphy.whiten_batch(t, frames, stride, length, kind, 5, 3)
        np.testing.assert_array_equal(t.cpu().numpy(), _whiten_rows(oracle, buf, length, kind, 5, 3),
                                      str((frames, length, stride)))


def _interleave_case(oracle, lphy, torch, dev, rng, frames, blocks, ppm, rdd):
    """One interleave and one deinterleave call on full-width random input with
    a partial block at the end of every row and strides beyond the rows."""
    nb = 4 + rdd
    tag = str((frames, blocks, ppm, rdd))
    ncw, nsy = blocks * ppm + (ppm - 1), blocks * nb + (nb - 1)   # rows as the caller counts them
    cw_stride, sym_stride = ncw + 5, nsy + 3
    cw = rng.integers(0, 256, (frames, cw_stride), dtype=np.uint8)
    tsy = torch.full((frames, sym_stride), S16 - 65536, dtype=torch.int16, device=dev)
    lphy.interleave_batch(_dev8(torch, dev, cw), frames, cw_stride, ncw, tsy, sym_stride, ppm, rdd)
    sy = _host16(tsy)
    # the oracle block by block over the rows' whole blocks (it has no state across blocks)
    want = oracle.interleave(cw[:, : blocks * ppm].reshape(-1), ppm, rdd).reshape(frames, blocks * nb)
    np.testing.assert_array_equal(sy[:, : blocks * nb], want, tag)
    assert (sy[:, blocks * nb:] == S16).all(), tag
    assert (want < (1 << ppm)).all()

    rs = rng.integers(0, 65536, (frames, sym_stride), dtype=np.uint16)
    tcw = torch.full((frames, cw_stride), S8, dtype=torch.uint8, device=dev)
    lphy.deinterleave_batch(_dev16(torch, dev, rs), frames, sym_stride, nsy, tcw, cw_stride, ppm, rdd)
    out = tcw.cpu().numpy()
    wantc = oracle.deinterleave(rs[:, : blocks * nb].reshape(-1), ppm, rdd).reshape(frames, blocks * ppm)
    np.testing.assert_array_equal(out[:, : blocks * ppm], wantc, tag)
    assert (out[:, blocks * ppm:] == S8).all(), tag

    # round trip of the whole blocks: the codeword bits below 4 + rdd come back, the others are dropped
    tcw.fill_(S8)
    lphy.deinterleave_batch(tsy, frames, sym_stride, nsy, tcw, cw_stride, ppm, rdd)
    out = tcw.cpu().numpy()
    np.testing.assert_array_equal(out[:, : blocks * ppm], cw[:, : blocks * ppm] & ((1 << nb) - 1), tag)
    assert (out[:, blocks * ppm:] == S8).all(), tag


@pytest.mark.parametrize("rdd", range(5))
def test_gpu_interleaver_every_geometry(oracle, lphy, torch_dev, rdd):
    """ppm 1..16 with this rdd, those with ppm < 4 + rdd (where the diagonal
    wraps more than once) among them: 3 whole blocks and a partial one a row."""
    torch, dev = torch_dev
    rng = np.random.default_rng(800 + rdd)
    for ppm in range(1, 17):
        _interleave_case(oracle, lphy, torch, dev, rng, 3, 3, ppm, rdd)


@pytest.mark.parametrize("ppm", [1, 3, 8, 16])
def test_gpu_interleaver_thread_totals(oracle, lphy, torch_dev, ppm):
    """One block a row, so k_interleave runs frames * (4 + rdd) threads and
    k_deinterleave frames * ppm: for every boundary count B the totals are the
    multiples of those units next to B on both sides (B itself where it is a
    multiple: every B at ppm 1, W at rdd 0, W - 1 at rdd 1)."""
    torch, dev = torch_dev
    rng = np.random.default_rng(820 + ppm)
    for rdd in (0, 1):
        counts = set()
        for unit in (ppm, 4 + rdd):
            for b in BOUNDARY:
                counts |= {b // unit, -(-b // unit)}
        for frames in sorted(counts - {0}):
            _interleave_case(oracle, lphy, torch, dev, rng, frames, 1, ppm, rdd)


def test_gpu_interleaver_less_than_a_block(lphy, torch_dev):
    torch, dev = torch_dev
    for ppm, rdd in ((1, 0), (5, 0), (8, 4), (16, 2), (2, 4)):
        nb = 4 + rdd
        tcw = torch.full((3, 20), S8, dtype=torch.uint8, device=dev)
        tsy = torch.full((3, 20), S16 - 65536, dtype=torch.int16, device=dev)
        lphy.interleave_batch(tcw, 3, 20, ppm - 1, tsy, 20, ppm, rdd)
        lphy.deinterleave_batch(tsy, 3, 20, nb - 1, tcw, 20, ppm, rdd)
        assert (tcw.cpu().numpy() == S8).all() and (_host16(tsy) == S16).all()


def _encode_case(oracle, lphy, torch, dev, data, length, sym_stride):
    frames, stride = data.shape
    tsy = torch.full((frames, sym_stride), S16 - 65536, dtype=torch.int16, device=dev)
    lphy.lora_encode_batch(_dev8(torch, dev, data), frames, stride, length, tsy, sym_stride)
    sy = _host16(tsy)
    tag = str((frames, stride, length, sym_stride))
    for f in range(frames):
        np.testing.assert_array_equal(sy[f, : 2 * length], oracle.encode(data[f, :length].tobytes()), tag)
    assert (sy[:, 2 * length:] == S16).all(), tag


def test_gpu_lora_encode_every_byte(oracle, lphy, torch_dev):
    torch, dev = torch_dev
    data = (np.arange(256)[None, :] + 37 * np.arange(3)[:, None]).astype(np.uint8)   # every value in every row
    _encode_case(oracle, lphy, torch, dev, np.ascontiguousarray(data), 256, 512)
    wide = np.concatenate([data, np.full((3, 4), 0xEE, np.uint8)], axis=1)
    _encode_case(oracle, lphy, torch, dev, np.ascontiguousarray(wide), 256, 512 + 7)


@pytest.mark.parametrize("b", BOUNDARY)
def test_gpu_lora_encode_boundary_counts(oracle, lphy, torch_dev, b):
    torch, dev = torch_dev
    rng = np.random.default_rng(840 + b)
    for frames, length in ((b, 1), (1, b), (b, 3), (2, b)):
        data = rng.integers(0, 256, (frames, length + 3), dtype=np.uint8)
        _encode_case(oracle, lphy, torch, dev, data, length, 2 * length + 5)
        _encode_case(oracle, lphy, torch, dev, np.ascontiguousarray(data[:, :length]), length, 2 * length)


def test_gpu_lora_encode_no_work(lphy, torch_dev):
    torch, dev = torch_dev
    data = torch.full((4, 8), S8, dtype=torch.uint8, device=dev)
    tsy = torch.full((4, 16), S16 - 65536, dtype=torch.int16, device=dev)
    lphy.lora_encode_batch(data, 4, 8, 0, tsy, 16)
    lphy.lora_encode_batch(data, 0, 8, 8, tsy, 16)
    assert (_host16(tsy) == S16).all() and (data.cpu().numpy() == S8).all()


@pytest.mark.parametrize("count", BOUNDARY)
def test_gpu_gray_and_hamming_boundary_counts(oracle, lphy, torch_dev, count):
    """`count` elements of a longer buffer: the element after them stays."""
    torch, dev = torch_dev
    rng = np.random.default_rng(860 + count)
    v = rng.integers(0, 65536, count + 1, dtype=np.uint16)
    for tb in (0, 1):
        t = _dev16(torch, dev, v)
        lphy.gray_batch(t[:count], tb)
        got = _host16(t)
        assert got[count] == v[count]
        np.testing.assert_array_equal(got[:count], [oracle.gray(int(x), tb) for x in v[:count]])
    x = rng.integers(0, 256, count + 1, dtype=np.uint8)
    for op in range(8):
        t = _dev8(torch, dev, x)
        fl = torch.full((count + 1,), S8, dtype=torch.uint8, device=dev)
        lphy.hamming_batch(t[:count], op, fl[:count])
        got, gfl = t.cpu().numpy(), fl.cpu().numpy()
        assert got[count] == x[count] and gfl[count] == S8
        want = [oracle.hamming(int(b), op) for b in x[:count]]
        np.testing.assert_array_equal(got[:count], [w[0] for w in want])
        np.testing.assert_array_equal(gfl[:count], [w[1] for w in want])


@pytest.mark.parametrize("op", range(8))
def test_gpu_hamming_without_flags(oracle, lphy, torch_dev, op):
    torch, dev = torch_dev
    x = np.concatenate([np.arange(256, dtype=np.uint8), np.arange(255, -1, -1, dtype=np.uint8)[: W + 1]])
    t = _dev8(torch, dev, x)
    lphy.hamming_batch(t, op, None)
    np.testing.assert_array_equal(t.cpu().numpy(), [oracle.hamming(int(b), op)[0] for b in x])


@pytest.mark.parametrize("frames", [1, W, W + 1])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_gpu_checksum_short_rows(oracle, lphy, torch_dev, kind, frames):
    torch, dev = torch_dev
    rng = np.random.default_rng(880 + 10 * kind + frames)
    for length in (0, 1, 2, 3, 255):
        stride = max(length, 2) + 3
        buf = rng.integers(0, 256, (frames, stride), dtype=np.uint8)
        out = torch.full((frames + 1,), S16 - 65536, dtype=torch.int16, device=dev)
        lphy.checksum_batch(_dev8(torch, dev, buf), frames, stride, length, kind, out)
        got = _host16(out)
        assert got[frames] == S16
        want = [oracle.checksum(buf[f, :length] if kind != 1 else buf[f, :2], kind) for f in range(frames)]
        np.testing.assert_array_equal(got[:frames], want, str(length))


def test_gpu_header_checksum_ignores_len(oracle, lphy, torch_dev):
    """LPHY_SUM_HEADER reads two bytes a row whatever `len` says: rows of
    stride 2 with len 0 and len 200, which must not trip len > stride."""
    torch, dev = torch_dev
    frames = W + 1
    buf = np.random.default_rng(899).integers(0, 256, (frames, 2), dtype=np.uint8)
    want = [oracle.checksum(buf[f], 1) for f in range(frames)]
    for length in (0, 200):
        out = torch.full((frames + 1,), S16 - 65536, dtype=torch.int16, device=dev)
        lphy.checksum_batch(_dev8(torch, dev, buf), frames, 2, length, 1, out)
        got = _host16(out)
        np.testing.assert_array_equal(got[:frames], want)
        assert got[frames] == S16


def test_gpu_codes_return_codes(lphy, torch_dev):
    """Every return include/lphy_hip.h documents for the seven calls, through
    the C entry points.  The buffers are far smaller than the refused calls
    describe, and keep their sentinel: nothing is launched."""
    torch, dev = torch_dev
    L = lphy.load()
    t8 = torch.full((64,), S8, dtype=torch.uint8, device=dev)
    u8 = torch.full((64,), S8, dtype=torch.uint8, device=dev)
    t16 = torch.full((64,), S16 - 65536, dtype=torch.int16, device=dev)
    b, c, s = t8.data_ptr(), u8.data_ptr(), t16.data_ptr()
    big = 1 << 20
    cases = [
        # lora_encode_batch(bytes, frames, stride, len, syms, sym_stride, stream)
        (L.lphy_hip_lora_encode_batch, (None, big, big, big, s, 2 * big, None), EINVAL),
        (L.lphy_hip_lora_encode_batch, (b, big, big, big, None, 2 * big, None), EINVAL),
        (L.lphy_hip_lora_encode_batch, (b, big, big, big + 1, s, 4 * big, None), EINVAL),      # len > stride
        (L.lphy_hip_lora_encode_batch, (b, big, 1 << 40, 1 << 31, s, 1 << 40, None), EINVAL),  # len > INT_MAX
        (L.lphy_hip_lora_encode_batch, (b, big, big, big, s, 2 * big - 1, None), ERANGE),      # 2 * len > sym_stride
        (L.lphy_hip_lora_encode_batch, (None, 0, 8, 4, None, 8, None), 0),
        (L.lphy_hip_lora_encode_batch, (None, big, 8, 0, None, 0, None), 0),
        # gray_batch(syms, count, to_binary, stream)
        (L.lphy_hip_gray_batch, (None, big, 0, None), EINVAL),
        (L.lphy_hip_gray_batch, (None, 0, 1, None), 0),
        # interleave_batch(cw, frames, cw_stride, cw_per_frame, syms, sym_stride, ppm, rdd, stream)
        (L.lphy_hip_interleave_batch, (b, big, big, big, s, big, 0, 4, None), EINVAL),
        (L.lphy_hip_interleave_batch, (b, big, big, big, s, big, 17, 4, None), EINVAL),
        (L.lphy_hip_interleave_batch, (b, big, big, big, s, big, 8, 5, None), EINVAL),
        (L.lphy_hip_interleave_batch, (None, big, big, big, s, big, 8, 4, None), EINVAL),
        (L.lphy_hip_interleave_batch, (b, big, big, big, None, big, 8, 4, None), EINVAL),
        (L.lphy_hip_interleave_batch, (b, big, big, 8 * 1000, s, 8 * 1000 - 1, 8, 4, None), ERANGE),  # symbols > sym_stride
        (L.lphy_hip_interleave_batch, (b, big, big, big + 1, s, 2 * big, 8, 4, None), ERANGE),        # row > cw_stride
        (L.lphy_hip_interleave_batch, (None, 0, 16, 16, None, 16, 8, 4, None), 0),
        # deinterleave_batch(syms, frames, sym_stride, syms_per_frame, cw, cw_stride, ppm, rdd, stream)
        (L.lphy_hip_deinterleave_batch, (s, big, big, big, b, big, 0, 4, None), EINVAL),
        (L.lphy_hip_deinterleave_batch, (s, big, big, big, b, big, 17, 4, None), EINVAL),
        (L.lphy_hip_deinterleave_batch, (s, big, big, big, b, big, 8, 5, None), EINVAL),
        (L.lphy_hip_deinterleave_batch, (None, big, big, big, b, big, 8, 4, None), EINVAL),
        (L.lphy_hip_deinterleave_batch, (s, big, big, big, None, big, 8, 4, None), EINVAL),
        (L.lphy_hip_deinterleave_batch, (s, big, big, 4 * 1000, b, 16 * 1000 - 1, 16, 0, None), ERANGE),  # codewords > cw_stride
        (L.lphy_hip_deinterleave_batch, (s, big, big, big + 1, b, 4 * big, 8, 4, None), ERANGE),          # row > sym_stride
        (L.lphy_hip_deinterleave_batch, (None, 0, 16, 16, None, 16, 8, 4, None), 0),
        # whiten_batch(bytes, frames, stride, len, kind, bit_ofs, rdd, stream)
        (L.lphy_hip_whiten_batch, (b, big, 4096, 4096, 3, 0, 4, None), EINVAL),
        (L.lphy_hip_whiten_batch, (b, big, 4096, 4096, -1, 0, 4, None), EINVAL),
        (L.lphy_hip_whiten_batch, (b, big, 4096, 4096, 1, 0, 5, None), EINVAL),
        (L.lphy_hip_whiten_batch, (b, big, 4096, 4096, 2, 0, 5, None), EINVAL),
        (L.lphy_hip_whiten_batch, (b, big, 4096, 4096, 0, -1, 4, None), EINVAL),
        (L.lphy_hip_whiten_batch, (b, big, 4096, 4096, 1, -1, 4, None), EINVAL),
        (L.lphy_hip_whiten_batch, (b, big, 4096, 4096, 2, -INT_MAX - 1, 4, None), EINVAL),
        (L.lphy_hip_whiten_batch, (b, big, 4096, 4097, 2, 0, 4, None), EINVAL),           # len > stride
        (L.lphy_hip_whiten_batch, (b, big, 1 << 17, 65536, 0, 0, 4, None), EINVAL),       # len > 65535
        (L.lphy_hip_whiten_batch, (None, big, 4096, 4096, 1, 0, 4, None), EINVAL),
        (L.lphy_hip_whiten_batch, (None, 0, 4096, 4096, 1, INT_MAX, 4, None), 0),
        (L.lphy_hip_whiten_batch, (None, big, 4096, 0, 2, INT_MAX, 0, None), 0),
        # hamming_batch(bytes, count, op, flags, stream)
        (L.lphy_hip_hamming_batch, (b, big, -1, c, None), EINVAL),
        (L.lphy_hip_hamming_batch, (b, big, 8, c, None), EINVAL),
        (L.lphy_hip_hamming_batch, (None, big, 0, c, None), EINVAL),
        (L.lphy_hip_hamming_batch, (None, 0, 7, None, None), 0),
        # checksum_batch(bytes, frames, stride, len, kind, out, stream)
        (L.lphy_hip_checksum_batch, (b, big, 4096, 4096, 3, s, None), EINVAL),
        (L.lphy_hip_checksum_batch, (b, big, 4096, 4096, -1, s, None), EINVAL),
        (L.lphy_hip_checksum_batch, (b, big, 4096, 4097, 0, s, None), EINVAL),            # len > stride
        (L.lphy_hip_checksum_batch, (b, big, 4096, 4097, 2, s, None), EINVAL),
        (L.lphy_hip_checksum_batch, (b, big, 1, 0, 1, s, None), EINVAL),                  # a header is 2 bytes
        (L.lphy_hip_checksum_batch, (None, big, 4096, 16, 0, s, None), EINVAL),
        (L.lphy_hip_checksum_batch, (b, big, 4096, 16, 2, None, None), EINVAL),
        (L.lphy_hip_checksum_batch, (None, 0, 4096, 16, 0, None, None), 0),
    ]
    for i, (fn, args, want) in enumerate(cases):
        assert fn(*args) == want, (i, fn.__name__, args)
    torch.cuda.synchronize()
    assert (t8.cpu().numpy() == S8).all() and (u8.cpu().numpy() == S8).all() and (_host16(t16) == S16).all()


def test_gpu_codes_in_stream_order(oracle, lphy, torch_dev):
    """encode -> whiten -> checksum on a fresh stream with no host
    synchronisation between them.  The whitening overwrites what the encoder
    reads and the checksum reads what the whitening writes, so either order
    going wrong shows; the uploads are on that stream too."""
    torch, dev = torch_dev
    frames, length, stride, sym_stride = W + 1, 255, 260, 2 * 255 + 3
    data = np.random.default_rng(900).integers(0, 256, (frames, stride), dtype=np.uint8)

    def chain(stream):
        t = _dev8(torch, dev, data)
        tsy = torch.full((frames, sym_stride), S16 - 65536, dtype=torch.int16, device=dev)
        out = torch.full((frames,), S16 - 65536, dtype=torch.int16, device=dev)
        lphy.lora_encode_batch(t, frames, stride, length, tsy, sym_stride, stream=stream)
        lphy.whiten_batch(t, frames, stride, length, 2, 511, 4, stream=stream)
        lphy.checksum_batch(t, frames, stride, length, 0, out, stream=stream)
        return t, tsy, out

    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(s):
        on_s = chain(s.cuda_stream)
        s.synchronize()
    on_default = chain(None)
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in on_s]
    for a, b in zip(got, on_default):
        np.testing.assert_array_equal(a, b.cpu().numpy())
    white = _whiten_rows(oracle, data, length, 2, 511, 4)
    np.testing.assert_array_equal(got[0], white)
    for f in range(frames):
        np.testing.assert_array_equal(got[1].view(np.uint16)[f, : 2 * length], oracle.encode(data[f, :length].tobytes()))
        assert got[2].view(np.uint16)[f] == oracle.checksum(white[f, :length], 0)
