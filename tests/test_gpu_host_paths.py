"""The two copy paths of the *_host entry points (csrc/lphy_host.h).  demod,
decode and modulate go through the context's pinned mirror when the call
fits it and copy slice by slice from the caller's memory otherwise; the other
five always copy slice by slice.  The pageable path of the first three needs
a call above 32 MiB, so the test build caps the mirror instead
(lphy_hip_test_pinned_max).

Every entry point runs once with the mirror and once with the cap at 0; both
results are byte-equal to each other and to the device-buffer entry point on
the same inputs (which the other GPU tests pin to the oracle).  Then: staging
that grows between calls of one context, and a call after one that its
*_impl refused with the uploads already enqueued."""
import errno

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _iq(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(DEV)


def _back(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.fixture(scope="module")
def dems(lphy):
    made = {}

    def get(sf):
        if sf not in made:
            made[sf] = lphy.Demodulator(sf, test_build=True)
        return made[sf]
    yield get
    for d in made.values():
        d.close()


def _both_paths(d, host_call):
    """host_call() through the mirror (where the entry point uses it) and
    with every copy pageable; the two results, each a tuple of arrays."""
    try:
        with_mirror = host_call()
        d.pinned_max(0)
        pageable = host_call()
    finally:
        d.pinned_max(32 << 20)
    return with_mirror, pageable


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g).reshape(-1).view(np.uint8), np.ascontiguousarray(w).reshape(-1).view(np.uint8)
        assert g.size == w.size and np.array_equal(g, w), f"{what}: output {i} differs"


def _check(d, host_call, device_call):
    want = device_call()
    with_mirror, pageable = _both_paths(d, host_call)
    _same(with_mirror, want, "mirror vs device entry point")
    _same(pageable, want, "pageable vs device entry point")


def _demod_device(lphy, d, iq, frames, fs, mode, flags):
    per = d.syms_per_frame(fs, mode)
    syms = torch.zeros(max(frames * per, 1), dtype=torch.int16, device=DEV)
    pay = torch.zeros(max(frames * (per // 2), 1), dtype=torch.uint8, device=DEV)
    meta = torch.zeros(frames * 32, dtype=torch.uint8, device=DEV)
    d.demod_batch(_t(iq), frames, fs, syms, meta, mode, flags, payload=pay)
    torch.cuda.synchronize()
    return (_back(syms, np.uint16)[: frames * per], _back(pay, np.uint8)[: frames * (per // 2)],
            _back(meta, lphy.META_DTYPE))


@pytest.mark.parametrize("sf,frames,mode,fused_min", [(7, 3, 0, 0), (7, 3, 2, 0), (11, 2, 2, -1)])
def test_demod(lphy, dems, sf, frames, mode, fused_min):
    """(SF 11 with the library's own launch choice: two frames take the
    separate launches, whose speculation records are the staging's lent slice)"""
    d = dems(sf)
    d.set_fused_min_frames(fused_min)
    fs = 4 * d.N
    iq = _iq(sf * 10 + mode, frames * fs)
    try:
        _check(d, lambda: d.demod_host(iq, frames, fs, mode, lphy.F_DECODE),
               lambda: _demod_device(lphy, d, iq, frames, fs, mode, lphy.F_DECODE))
    finally:
        d.set_fused_min_frames(0)


def test_ragged(lphy, dems):
    d = dems(7)
    lengths = [0, 3 * 128, 5 * 128 + 7]
    mode, flags, fill = lphy.MODE_DECHIRP_LORA_DEMODULATE, lphy.F_DECODE, 0xBEEF
    iq = _iq(3, sum(lengths))
    desc = d.ragged_layout(lengths, mode)
    n_iq, n_out = d._ragged_extent(desc, mode)

    def device():
        syms = _t(np.full(max(n_out, 1), fill, np.uint16)).view(torch.int16)
        pay = _t(np.full(max((n_out + 1) // 2, 1), fill & 0xFF, np.uint8))
        meta = torch.zeros(len(lengths) * 32, dtype=torch.uint8, device=DEV)
        d.demod_ragged(_t(iq), _t(desc), len(lengths), syms, meta, mode, flags, payload=pay, iq_samples=n_iq,
                       out_syms=n_out)
        torch.cuda.synchronize()
        return _back(syms, np.uint16), _back(pay, np.uint8), _back(meta, lphy.META_DTYPE)

    _check(d, lambda: d.demod_ragged_host(iq, lengths, mode, flags, fill=fill)[:3], device)


def test_detect(lphy, dems):
    d = dems(7)
    first, hop, windows = 5, 64, 3
    iq = _iq(4, first + (windows - 1) * hop + d.N + 3)

    def device():
        out = torch.zeros(windows * 16, dtype=torch.uint8, device=DEV)
        d.detect_batch(_t(iq), iq.size, first, hop, 1, windows, out, lphy.DET_DECHIRP)
        torch.cuda.synchronize()
        return (_back(out, lphy.DETECT_DTYPE),)

    _check(d, lambda: (d.detect_host(iq, first, hop, 1, windows, lphy.DET_DECHIRP),), device)


@pytest.mark.parametrize("count", [8, 0])
def test_decode(lphy, dems, count):
    d = dems(7)
    syms = lphy.encode_payloads(np.random.default_rng(5).integers(0, 256, count // 2, dtype=np.uint8))

    def host():
        rc, out, meta = d.decode_host(syms)
        assert rc == 0
        return out, meta

    def device():
        pay = torch.zeros(max(count // 2, 1), dtype=torch.uint8, device=DEV)
        meta = torch.zeros(32, dtype=torch.uint8, device=DEV)
        t_syms = _t(syms).view(torch.int16) if count else torch.zeros(1, dtype=torch.int16, device=DEV)
        d.decode_batch(t_syms, 1, count, pay, meta)
        torch.cuda.synchronize()
        return _back(pay, np.uint8)[: count // 2], _back(meta, lphy.META_DTYPE)

    _check(d, host, device)


@pytest.mark.parametrize("nsyms", [2, 0])
def test_modulate(lphy, dems, nsyms):
    d = dems(7)
    syms = np.array([5, 100][:nsyms], np.uint16)

    def device():
        iq = torch.zeros((nsyms + 2) * d.N * 2, dtype=torch.float32, device=DEV)
        d.modulate_batch(_t(syms).view(torch.int16) if nsyms else None, 1, nsyms, iq)
        torch.cuda.synchronize()
        return (_back(iq, np.float32),)

    _check(d, lambda: (d.modulate_host(syms),), device)


def test_estimate(lphy, dems):
    d = dems(7)
    iq = _iq(6, 2 * d.N)

    def device():
        meta = torch.zeros(32, dtype=torch.uint8, device=DEV)
        d.estimate_batch(_t(iq), 1, iq.size, iq.size, meta)
        torch.cuda.synchronize()
        return (_back(meta, lphy.META_DTYPE),)

    _check(d, lambda: (np.array([d.estimate_host(iq)]),), device)


def test_compensate(lphy, dems):
    """(a non-zero time shift: the rotation goes through the staging's lent shift buffer)"""
    d = dems(7)
    iq = _iq(7, 2 * d.N)
    cfo, shift = 0.3, 3.0

    def device():
        t = _t(iq)
        rc = d.lib.lphy_hip_compensate(d.ctx, t.data_ptr(), iq.size, cfo, shift, None)
        assert rc == 0
        torch.cuda.synchronize()
        return (_back(t, np.complex64),)

    _check(d, lambda: (d.compensate_host(iq, cfo, shift),), device)


def test_compensate_batch(lphy, dems):
    d = dems(7)
    frames, fs = 3, 2 * d.N + 1
    iq = _iq(8, frames * fs)
    meta = np.zeros(frames, lphy.META_DTYPE)
    meta["cfo"], meta["time_offset"] = [0.3, -0.2, 0.0], [3.0, -2.0, 0.0]

    def device():
        t = _t(iq)
        d.compensate_batch(t, t, frames, fs, _t(meta))
        torch.cuda.synchronize()
        return (_back(t, np.complex64),)

    _check(d, lambda: (d.compensate_batch_host(iq, frames, fs, meta),), device)


def test_staging_grows_between_calls(lphy, dems):
    """A context nothing was reserved on: a small call, one four times as
    large (the staging and its mirror are replaced), the small one again."""
    mode, flags = lphy.MODE_DECHIRP_LORA_DEMODULATE, lphy.F_DECODE
    fs = 4 * 128
    small, large = _iq(9, fs), _iq(10, 4 * fs)
    want_small = _demod_device(lphy, dems(7), small, 1, fs, mode, flags)
    want_large = _demod_device(lphy, dems(7), large, 4, fs, mode, flags)
    d = lphy.Demodulator(7, test_build=True)
    try:
        _same(d.demod_host(small, 1, fs, mode, flags), want_small, "first call")
        _same(d.demod_host(large, 4, fs, mode, flags), want_large, "larger call")
        _same(d.demod_host(small, 1, fs, mode, flags), want_small, "small call again")
    finally:
        d.close()


def test_call_after_a_refused_one(lphy, dems):
    """demod_batch refuses mode 0 on a frame that is no whole number of
    symbols, after demod_host enqueued its uploads; the stream is waited for
    and the next call on the context is right."""
    d = dems(7)
    fs = 4 * 128
    d.bounds_violations(reset=True)
    with pytest.raises(lphy.LphyError) as e:
        d.demod_host(_iq(11, 2 * (fs + 1)), 2, fs + 1, lphy.MODE_DEMODULATE)
    assert e.value.rc == -errno.EINVAL
    iq = _iq(12, 2 * fs)
    mode, flags = lphy.MODE_DECHIRP_LORA_DEMODULATE, lphy.F_DECODE
    _same(d.demod_host(iq, 2, fs, mode, flags), _demod_device(lphy, d, iq, 2, fs, mode, flags), "after -EINVAL")
    assert d.bounds_violations() == 0
