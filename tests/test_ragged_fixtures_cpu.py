"""The fixtures of tests/test_gpu_ragged.py hold what that file relies on,
with the CPU oracle alone (no GPU):

* the SF 12 frames: uncut, each packet's payload comes back from the oracle's
  chain with a good CRC, so the -8 dB noise leaves the symbols decidable;
* the isolation case: frame A's estimate gives t_off > 0 in every mode, so
  its last symbol's shifted window would pass the frame's end and the clamp
  keeps it in place; read with the buffer's end instead of the frame's (A with
  the loud frame B behind it), that symbol's window moves into B: the oracle's
  symbol for it differs, and A would be normalised by B's amplitude.  A and C
  alone need no normalisation, B alone does;
* a frame without a whole symbol leaves x86-64's default NaN in the oracle's
  cfo and time_offset (what the kernels write for it)."""
import numpy as np

from test_gpu_ragged import MIXED, isolation_frames, mode_input


def test_sf12_frames_decode_with_the_oracle(oracle):
    from test_gpu_osr import _frames
    sf, N = 12, 4096
    for k, s in enumerate(MIXED[12]):
        plen = max(1, (s + 1) // 2)
        # the packet mixed_frames cuts to s symbols, and its payload
        x = _frames(oracle, sf, 1, 1, plen, seed=1000 * sf + 31 * k, snr=-8.0, cfo=0.3 if k & 1 else 0.0)[0]
        want = np.random.default_rng(1000 * sf + 31 * k).integers(0, 256, plen, dtype=np.uint8)
        r, syms, sync, met = oracle.lora_demodulate(oracle.dechirp(x, sf), sf)
        assert r == 2 * plen
        r, pay, crc = oracle.decode(syms)
        np.testing.assert_array_equal(pay, want)
        assert x.size >= s * N + 37


def test_isolation_case_depends_on_the_clamp(oracle):
    sf, N = 7, 128
    a, b, c = isolation_frames(oracle, sf)
    for x, loud in ((a, False), (b, True), (c, False)):
        assert (max(np.abs(x.real).max(), np.abs(x.imag).max()) > 1.0) == loud
    for mode in (0, 1, 2):
        fa, fb = mode_input(oracle, sf, a, mode), mode_input(oracle, sf, b, mode)

        def run(x):
            if mode == 0:
                return oracle.demodulate(x, sf)
            return oracle.lora_demodulate(oracle.dechirp(x, sf) if mode == 2 else x, sf)
        r, syms, sync, met = run(fa)
        assert r == fa.size // N - 2
        t_off = int(np.round(met[1]))
        assert 0 < t_off < N, (mode, met)
        # the same samples with B's first symbol inside the buffer: the last
        # symbol's window shifts by t_off and the symbol changes
        r2, syms2, _, met2 = run(np.concatenate([fa, fb[:N]]))
        assert syms2[r - 1] != syms[r - 1], mode


def test_frame_without_a_symbol_leaves_the_host_nan(oracle):
    x = np.full(37, 0.25 + 0.5j, np.complex64)
    r, syms, sync, met = oracle.lora_demodulate(x, 7)
    assert r == 0 and sync == 0
    assert list(met.view(np.uint32)) == [0xFFC00000, 0xFFC00000]
    r, syms, sync, met = oracle.lora_demodulate(np.zeros(0, np.complex64), 7)
    assert r == 0
    assert list(met.view(np.uint32)) == [0xFFC00000, 0xFFC00000]
