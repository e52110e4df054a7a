"""What tests/test_gpu_channelize*.py and tests/test_gpu_synthesize*.py share,
beside the models (channelize_model.py, synthesize_model.py)."""
import numpy as np
import pytest

EINVAL, ERANGE = -22, -34
GUARD = 4      # samples in front of and behind the output, which the call must leave alone
BIG = (1 << 40) + 3
PAYLOAD_LENS = [[1, 5, 2], [3, 1, 4], [5, 2, 3]]   # the chains' frames, per channel


@pytest.fixture(scope="module")
def dem(lphy):
    d = lphy.Demodulator(7)
    yield d
    d.close()


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def rand_c64(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def guarded(dev, nbytes, fill, lead=0):
    """A device buffer of `nbytes` between GUARD samples (`lead` more bytes in
    front), all of it `fill`: the whole allocation and the buffer in it."""
    import torch
    g0 = GUARD * 8 + lead
    whole = torch.full((g0 + nbytes + GUARD * 8,), fill, dtype=torch.uint8, device=dev)
    return whole, whole[g0: g0 + nbytes]


def unguarded(whole, nbytes, fill, lead=0):
    """The buffer's bytes as the call left them, once the guards are seen untouched."""
    out, g0 = whole.cpu().numpy(), GUARD * 8 + lead
    assert (out[:g0] == fill).all() and (out[g0 + nbytes:] == fill).all(), "guards written"
    return out[g0: g0 + nbytes]


def frames_of(oracle, ch):
    """Channel ch's frames: header, payload, checksum."""
    rng = np.random.default_rng(7000 + ch)
    out = []
    for n in PAYLOAD_LENS[ch]:
        body = rng.integers(0, 256, n, dtype=np.uint8)
        crc = int(oracle.sx_checksum(body))
        out.append(np.concatenate([rng.integers(0, 256, 2, dtype=np.uint8), body,
                                   np.array([crc & 0xFF, crc >> 8], np.uint8)]))
    return out


def rx_buffers(d, dev, windows, n_sym, max_frames, fill):
    """One channel's device buffers behind the channeliser in the chains: detector records, the found table
    and its info, the search's workspace, symbols, bytes and metadata, all pre-filled."""
    import torch
    u8 = lambda n: torch.full((n,), fill, dtype=torch.uint8, device=dev)  # noqa: E731
    return dict(rec=u8(windows * 16), desc=u8((max_frames + 1) * 32), info=u8(32), work=u8(d.find_frames_workspace(windows)),
                syms=torch.full((n_sym,), -1, dtype=torch.int16, device=dev), data=u8(n_sym // 2 + 1),
                meta=u8(max_frames * 32))
