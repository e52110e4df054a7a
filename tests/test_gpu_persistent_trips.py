"""The later trips of the persistent grids of k_rg_demod (csrc/lphy_ragged.h),
k_detect (csrc/lphy_detect.h) and k_tx_samples (csrc/lphy_tx.h).

Each of them is launched with min(resident grid, tiles of the call)
workgroups, so its loop `for (t0 = blockIdx.x * T; t0 < units; t0 += stride)`
takes a second trip only in a call with more tiles than the device holds
workgroups - larger than any other test's.  The test build's
lphy_hip_test_grid_cap (Demodulator.grid_cap, csrc/lphy_testing.h) caps the
grid instead: under a cap of 1 one workgroup walks every tile of a small call,
under a cap of 2 or 3 the workgroups make unequal numbers of trips.  What runs
only then: the barrier / team_sync in front of the restaging, the reuse of
red[], dstp[] and the LDS rows, the `continue` of a wave of tail units in
k_tx_samples, the early exit of the workgroups with one trip fewer, and the
parked phases of units read in a later trip.

Every output is compared bit for bit with the CPU oracle on each frame or
window alone and byte for byte with the same call without the cap, and the
test build's device index checks stay at zero.  The grid size itself cannot
be seen in any output (that is what these tests assert), so the tests do not
depend on the resident grid of the device.

Beside the cap: ragged calls at SF 9 and SF 11 (kernels no other ragged test
instantiates; at SF 11 a tile holds two symbols of two wavefronts each), 601
frames in one ragged call (k_rg_final's third block, a partly filled last
workgroup of k_rg_prologue, unit_frame over 602 records with runs of frames
without units), and the ragged kernels' in-place re-runs for non-finite
samples (k_rg_prologue's cmul_x rescan, k_rg_demod's restaging of a wave's or
a workgroup's symbols) against the oracle.

One figure of the receive cases cannot hold as a partial tile: at SF 12 a tile
is one symbol (T = 1), so `units % T != 0` is asserted where T > 1, and SF 12
also runs under a cap of 2, where 9 tiles give trips of 5 and 4."""
import copy
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc
from test_gpu_nonfinite import VALUES, _nan_bits_equal
from test_gpu_ragged import MIXED, SENTINEL, check_batch, expect, mixed_frames, mode_input
from test_gpu_tx_ragged import (CYCLE, HAND_SPECS, Run, check_iq, check_syms, extent, hand_written,
                                payloads_of)

pytestmark = pytest.mark.gpu

COUNTS = dict(MIXED)
COUNTS[9] = [0, 1, 2, 3, 5, 10, 18, 2, 6]   # 47 symbols, T = 8
COUNTS[11] = [2, 3, 1, 5]                   # 11 symbols, T = 2
MANY = [0, 0, 0, 1, 2, 3, 4, 5]


def tile_of(sf):
    """Geo<SF>::T: symbols (windows) per tile of 256 threads, N / 16 lanes each."""
    return 256 // max(1, (1 << sf) // 16)


def caps_of(sf):
    return (1, 2, 3) if tile_of(sf) == 1 else (1, 3)


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_outputs(a, b, what):
    """Symbols, bytes and meta records of two ragged calls, byte for byte."""
    for x, y, name in zip(a[:3], b[:3], ("symbols", "bytes", "meta")):
        np.testing.assert_array_equal(_u8(x), _u8(y), err_msg=f"{what}: {name}")


def _demod(lphy, sf, hann=False, **kw):
    return lphy.Demodulator(sf, window=lphy.WINDOW_HANN if hann else lphy.WINDOW_NONE, test_build=True, **kw)


@pytest.fixture(scope="module")
def frames_of(oracle):
    """The mixed-length frames per (sf, extra counts, tail) and their per-mode inputs, built once."""
    cache = {}

    def get(sf, mode, extra=(), tail=0):
        key = (sf, mode, tuple(extra), tail)
        if key not in cache:
            raw = cache.setdefault((sf, "raw", tuple(extra), tail),
                                   mixed_frames(oracle, sf, COUNTS[sf] + list(extra), tail))
            cache[key] = [mode_input(oracle, sf, x, mode) for x in raw]
        return cache[key]
    return get


# ---- ragged receive under a cap ---------------------------------------------
RX_CASES = [(sf, mode, 0) for sf in (7, 8, 9, 10, 11, 12) for mode in (0, 1, 2)] + \
           [(8, mode, 2) for mode in (0, 1, 2)]   # 2 = LPHY_F_NO_SCRATCH


@pytest.mark.parametrize("sf,mode,extra_flags", RX_CASES)
def test_ragged_receive_capped(oracle, lphy, frames_of, sf, mode, extra_flags):
    hann = mode == sf % 3   # one mode per SF through the Hann window
    frames = frames_of(sf, mode)
    lens = [x.size for x in frames]
    flat = np.concatenate(frames)
    flags = lphy.F_DECODE | extra_flags
    d = _demod(lphy, sf, hann)
    d.bounds_violations(reset=True)
    ref = d.demod_ragged_host(flat, lens, mode, flags, fill=SENTINEL)
    T, units = tile_of(sf), int(ref[3]["unit_offset"][-1])
    assert units == sum(COUNTS[sf]) and -(-units // T) >= 3
    assert T == 1 or units % T != 0   # a partial last tile
    what = f"SF{sf} mode {mode} hann {hann} flags {flags}"
    check_batch(oracle, sf, frames, mode, hann, *ref, f"{what} uncapped", scratch=not extra_flags)
    for cap in caps_of(sf):
        d.grid_cap(cap)
        got = d.demod_ragged_host(flat, lens, mode, flags, fill=SENTINEL)
        check_batch(oracle, sf, frames, mode, hann, *got, f"{what} cap {cap}", scratch=not extra_flags)
        same_outputs(got, ref, f"{what} cap {cap} against the uncapped call")
    assert d.bounds_violations() == 0
    d.close()


# ---- ragged receive, non-finite samples --------------------------------------
# Three frames more than the capped cases have: without them no tile of T = 4
# or T = 2 symbols holds a poisoned data symbol beside a finite frame's.
NF_EXTRA = (1, 3, 1)
# per SF: (frame, estimate symbol), (frame, data symbol index in the frame), frame of the poisoned tail
NF_SITES = {7: ((4, 1), (8, 3), 6), 10: ((1, 1), (2, 4), 4), 11: ((2, 0), (3, 4), 5)}


def ref_scale(src):
    """lora_demodulate's normalisation (LoRaDemod.cpp:60-78): max over the
    samples of std::max(|re|, |im|) by `if (m > max)`, which never takes a NaN."""
    re, im = np.abs(src.real.astype(np.float32)), np.abs(src.imag.astype(np.float32))
    m = np.where(re < im, im, re)
    m = m[~np.isnan(m)]
    mx = np.float32(m.max()) if m.size else np.float32(0.0)
    if not mx > 1.0:
        return 0, np.float32(1.0)
    with np.errstate(all="ignore"):
        return 1, np.float32(1.0) / mx


def check_nonfinite(oracle, sf, frames, mode, out, what):
    syms, pay, meta, desc = out
    for f, x in enumerate(frames):
        with np.errstate(all="ignore"):
            e = expect(oracle, sf, x, mode, False)
        w = f"{what} frame {f}"
        m = meta[f]
        assert m["status"] == e["status"], w
        if "normalised" in e:
            src = oracle.dechirp(x, sf) if mode == 2 and x.size else x
            norm, scale = ref_scale(src)
            assert m["normalised"] == norm, w
            assert np.float32(m["scale"]).view(np.uint32) == scale.view(np.uint32), w
        if e["syms"] is None:
            continue
        so, n = int(desc["sym_offset"][f]), len(e["syms"])
        np.testing.assert_array_equal(syms[so: so + n], e["syms"], err_msg=w)
        assert m["sync_word"] == e["sync"] and m["have_sync"] == e["have_sync"], w
        _nan_bits_equal([m["cfo"], m["time_offset"]], [e["cfo"], e["toff"]])
        if "bytes" in e:
            np.testing.assert_array_equal(pay[so // 2: so // 2 + n // 2], e["bytes"], err_msg=w)
            assert m["crc_ok"] == e["crc"], w


@pytest.mark.parametrize("sf", [7, 10, 11])
@pytest.mark.parametrize("mode", [1, 2])
def test_ragged_receive_nonfinite(oracle, lphy, frames_of, sf, mode):
    """A value of VALUES in an estimate symbol of one frame, in a data symbol
    of another that a single workgroup reaches in its second trip or later,
    and (mode 1) in the trailing partial symbol of a third; every poisoned
    symbol shares its tile with a symbol of a finite frame, which the re-run
    restages with it.  With and without the cap."""
    N, T = 1 << sf, tile_of(sf)
    tail = 37 if mode == 1 else 0
    clean = frames_of(sf, mode, NF_EXTRA, tail)
    counts = COUNTS[sf] + list(NF_EXTRA)
    first = np.concatenate([[0], np.cumsum(counts)])
    (fe, se), (fd, sd), ft = NF_SITES[sf]
    poisoned = {fe, fd} | ({ft} if mode == 1 else set())
    assert len(poisoned) == (3 if mode == 1 else 2)
    assert se < min(counts[fe], 2) and 2 <= sd < counts[fd]
    assert (first[fd] + sd) // T >= 1   # trip 2 or later under a cap of 1
    owner = np.repeat(np.arange(len(counts)), counts)   # unit -> frame

    def beside_finite(u):
        return any(f not in poisoned for f in owner[u // T * T: u // T * T + T])
    assert beside_finite(first[fe] + se) and beside_finite(first[fd] + sd)
    assert mode != 1 or any(beside_finite(u) for u in range(first[ft], first[ft + 1]))

    lens = [x.size for x in clean]
    d = _demod(lphy, sf)
    d.bounds_violations(reset=True)
    for k in range(len(VALUES)):
        frames = [x.copy() for x in clean]
        frames[fe][se * N + 7] = VALUES[k]
        frames[fd][sd * N + N // 2 + 1] = VALUES[(k + 3) % len(VALUES)]
        if mode == 1:
            frames[ft][counts[ft] * N + 5] = VALUES[(k + 5) % len(VALUES)]
        flat = np.concatenate(frames)
        outs = {}
        for cap in (0, 1):
            d.grid_cap(cap)
            outs[cap] = d.demod_ragged_host(flat, lens, mode, lphy.F_DECODE, fill=SENTINEL)
            check_nonfinite(oracle, sf, frames, mode, outs[cap], f"SF{sf} mode {mode} values {k} cap {cap}")
        same_outputs(outs[1], outs[0], f"SF{sf} mode {mode} values {k}")
    assert d.bounds_violations() == 0
    d.close()


# ---- ragged receive, many frames ---------------------------------------------
@pytest.fixture(scope="module")
def many(oracle):
    """601 frames of 0, 0, 0, 1, 2, 3, 4, 5 symbols in turn per (sf, mode), built once."""
    cache = {}

    def get(sf, mode):
        if (sf, mode) not in cache:
            counts = [MANY[f % len(MANY)] for f in range(601)]
            raw = cache.setdefault((sf, "raw"), mixed_frames(oracle, sf, counts, seed=5))
            cache[sf, mode] = [mode_input(oracle, sf, x, mode) for x in raw]
        return cache[sf, mode]
    return get


@pytest.mark.parametrize("sf", [7, 9])
@pytest.mark.parametrize("mode", [0, 2])
def test_ragged_receive_many_frames(oracle, lphy, many, sf, mode):
    frames = many(sf, mode)
    lens = [x.size for x in frames]
    flat = np.concatenate(frames)
    d = _demod(lphy, sf)
    d.bounds_violations(reset=True)
    ref = d.demod_ragged_host(flat, lens, mode, lphy.F_DECODE, fill=SENTINEL)
    assert ref[3].size == 602 and int(ref[3]["unit_offset"][-1]) == 75 * sum(MANY)
    check_batch(oracle, sf, frames, mode, False, *ref, f"SF{sf} mode {mode} 601 frames")
    d.grid_cap(2)
    got = d.demod_ragged_host(flat, lens, mode, lphy.F_DECODE, fill=SENTINEL)
    check_batch(oracle, sf, frames, mode, False, *got, f"SF{sf} mode {mode} 601 frames cap 2")
    same_outputs(got, ref, f"SF{sf} mode {mode} 601 frames cap 2")
    assert d.bounds_violations() == 0
    d.close()


# ---- the detector under a cap ------------------------------------------------
@pytest.fixture(scope="module")
def detect_sets(oracle):
    cache = {}

    def get(sf, noisy, dechirp, hann, lphy, first, hop, windows):
        key = (sf, noisy, dechirp, hann)
        if key not in cache:
            pk = cache.setdefault((sf, noisy), dc.packets(oracle, sf, noisy)[: 3 << sf])
            iq = dc.detector_feed(oracle, pk, sf, dechirp)
            cache[key] = (iq, dc.expected(oracle, lphy, iq, sf, first, hop, 1, windows, dechirp, hann))
        return cache[key]
    return get


# (sf, first, hop, windows): 8 tiles of 32, 511 tiles of 4 (both with a partial
# last tile), 128 tiles of 1.  Windows 123, 1019 and 0 / 64 are whole symbols:
# in the clean set a single tone, which no certificate of the sum holds for.
DETECT_CASES = [(7, 5, 1, 251), (10, 5, 1, 2043), (12, 0, 64, 128)]


@pytest.mark.parametrize("sf,first,hop,windows", DETECT_CASES)
@pytest.mark.parametrize("noisy", [True, False])
@pytest.mark.parametrize("hann,dechirp", [(False, True), (True, False)])
def test_detect_capped(oracle, lphy, detect_sets, sf, first, hop, windows, noisy, hann, dechirp):
    """The device form, every call into records pre-filled with a sentinel (the
    host form's staging would still hold the previous call's records where a
    call left a window out), with three guard records behind them."""
    import torch
    T = tile_of(sf)
    assert -(-windows // T) >= 3 and (T == 1 or windows % T != 0)
    iq, want = detect_sets(sf, noisy, dechirp, hann, lphy, first, hop, windows)
    fl = lphy.DET_DECHIRP if dechirp else 0
    dev = torch.device("cuda:0")
    t_iq = torch.from_numpy(iq.view(np.float32).copy()).to(dev)
    d = _demod(lphy, sf, hann)
    d.bounds_violations(reset=True)
    d.detect_serial_count(reset=True)

    def call():
        t_out = torch.full(((windows + 3) * 16,), 0xAB, dtype=torch.uint8, device=dev)
        d.detect_batch(t_iq, iq.size, first, hop, 1, windows, t_out, fl, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = t_out.cpu().numpy()
        assert (out[windows * 16:] == 0xAB).all()
        return out[: windows * 16].view(lphy.DETECT_DTYPE), d.detect_serial_count()
    ref, walked = call()
    what = f"SF{sf} hop {hop} noisy {noisy} hann {hann}"
    dc.assert_records_equal(ref, want, f"{what} uncapped")
    print(f"{what}: {walked} of {windows} windows walked in order")
    if not noisy and not hann:
        assert walked >= 1   # the clean set's whole symbols take the serial bin walk
    for cap in caps_of(sf):
        d.grid_cap(cap)
        got, n = call()
        dc.assert_records_equal(got, want, f"{what} cap {cap}")
        np.testing.assert_array_equal(_u8(got), _u8(ref), err_msg=f"{what} cap {cap} against the uncapped call")
        assert n == walked, f"{what} cap {cap}"
    assert d.bounds_violations() == 0
    d.close()


# ---- ragged transmit under a cap ---------------------------------------------
TX_CAPS = (1, 2)
LONG_SPECS = HAND_SPECS + [(33, None, 0), (16, None, 0), (33, None, 0), (9, None, 3), (33, None, 0), (0, None, 0),
                           (33, None, 0), (33, None, 0), (5, None, 0), (33, None, 0), (33, None, 0)]


@pytest.fixture(scope="module")
def modulated(oracle):
    """oracle.modulate(oracle.encode(payload) or symbols, ...) per frame, once per argument set."""
    cache = {}

    def get(src, sf, osr=1, ampl=1.0, sync=0x12, symbols=False):
        syms = np.asarray(src, np.uint16) if symbols else oracle.encode(bytes(src))
        key = (syms.tobytes(), sf, osr, ampl, sync)
        if key not in cache:
            iq = oracle.modulate(syms, sf, osr, 125000, ampl, sync)
            iq.setflags(write=False)
            cache[key] = (syms, iq)
        return cache[key]
    return get


def _iq_bits(x):
    return np.ascontiguousarray(x).reshape(-1).view(np.uint32)


def cycle_batch(sf=7, frames=70):
    lens = [CYCLE[f % len(CYCLE)] for f in range(frames)]
    return lens, payloads_of(lens, 100 + sf)


@pytest.mark.parametrize("osr", [1, 2])
def test_tx_byte_form_capped(lphy, modulated, osr):
    sf = 7
    lens, pl = cycle_batch()
    d = lphy.Demodulator(sf, osr=osr, test_build=True)
    d.bounds_violations(reset=True)
    desc = d.tx_layout(lens)
    n_iq, n_sym = extent(d, lphy, desc)
    assert -(-int(desc["unit_offset"][-1]) // 256) >= 3 and int(desc["unit_offset"][-1]) % 256
    want = [modulated(p, sf, osr) for p in pl]
    ref_iq, ref_sy = Run(lphy, d, desc, n_iq, n_sym).tx(b"".join(pl))
    check_iq(ref_iq, desc, [w[1] for w in want], f"osr {osr} uncapped")
    for cap in TX_CAPS:
        d.grid_cap(cap)
        iq, syms = Run(lphy, d, desc, n_iq, n_sym).tx(b"".join(pl))
        check_iq(iq, desc, [w[1] for w in want], f"osr {osr} cap {cap}")
        check_syms(syms, desc, [w[0] for w in want], f"osr {osr} cap {cap}")   # d_syms_out equals encode()
        np.testing.assert_array_equal(_iq_bits(iq), _iq_bits(ref_iq))
        np.testing.assert_array_equal(syms, ref_sy)
    assert d.bounds_violations() == 0
    d.close()


@pytest.mark.parametrize("osr", [1, 2])
def test_tx_symbol_form_capped(lphy, modulated, osr):
    """The same batch through lphy_hip_modulate_ragged, with one frame of an
    odd symbol count among them."""
    sf, step = 7, 128 * osr
    lens, pl = cycle_batch()
    frames_syms = [modulated(p, sf, osr)[0] for p in pl]
    frames_syms.insert(2, modulated(payloads_of([4], 7)[0], sf, osr)[0][:7])
    d = lphy.Demodulator(sf, osr=osr, test_build=True)
    d.bounds_violations(reset=True)
    desc = d.ragged_layout([(s.size + 2) * step for s in frames_syms], lphy.MODE_LORA_DEMODULATE)
    n_iq, n_sym = extent(d, lphy, desc)
    assert -(-int(desc["unit_offset"][-1]) // 256) >= 3
    flat = np.zeros(n_sym, np.uint16)
    for f, s in enumerate(frames_syms):
        at = int(desc["sym_offset"][f])
        flat[at: at + s.size] = s
    want = [modulated(s, sf, osr, symbols=True)[1] for s in frames_syms]
    ref_iq, _ = Run(lphy, d, desc, n_iq, n_sym).modulate(flat)
    check_iq(ref_iq, desc, want, f"symbol form osr {osr} uncapped")
    for cap in TX_CAPS:
        d.grid_cap(cap)
        iq, _ = Run(lphy, d, desc, n_iq, n_sym).modulate(flat)
        check_iq(iq, desc, want, f"symbol form osr {osr} cap {cap}")
        np.testing.assert_array_equal(_iq_bits(iq), _iq_bits(ref_iq))
    assert d.bounds_violations() == 0
    d.close()


def test_tx_hand_written_descriptors_capped(lphy, modulated):
    """test_hand_written_descriptors' table (odd iq_offsets: lead rows; a frame
    below two symbols; gaps), with frames added up to three tiles of 256 units."""
    sf, osr, step = 7, 1, 128
    desc = hand_written(sf, osr, LONG_SPECS)
    d = lphy.Demodulator(sf, osr=osr, test_build=True)
    d.bounds_violations(reset=True)
    nf = len(LONG_SPECS)
    assert -(-int(desc["unit_offset"][-1]) // 256) >= 3 and int(desc["unit_offset"][-1]) % 256
    # a lead row (a modulated symbol at an odd sample offset) in a tile behind the first
    total = desc["samples"][:-1] // np.uint64(step)
    nsym = np.where(total >= 2, 2 + ((total - np.minimum(total, 2)) & ~np.uint64(1)), 0)
    last_unit = desc["unit_offset"][:-1] + nsym
    assert np.any((desc["iq_offset"][:-1] & 1 == 1) & (nsym > 0) & (last_unit > 256))
    assert np.any((desc["iq_offset"][:-1] & 1 == 1) & (nsym > 0) & (last_unit <= 256))
    n_iq = int((desc["iq_offset"][:-1] + desc["samples"][:-1]).max())
    n_sym = int(desc["sym_offset"][-1])
    pl = payloads_of([s[0] for s in LONG_SPECS], 40 + sf)
    data = np.full(n_sym // 2 + 1, 0xEE, np.uint8)
    for f, p in enumerate(pl):
        at = int(desc["sym_offset"][f]) // 2
        data[at: at + len(p)] = np.frombuffer(p, np.uint8)
    want = [modulated(p, sf, osr, 0.75, 0x34) for p in pl]
    none = [f for f in range(nf) if total[f] < 2]
    assert none == [3, 8]   # fewer than two symbols: nothing written
    want_iq = [np.zeros(0, np.complex64) if f in none else w[1] for f, w in enumerate(want)]
    want_sy = [np.zeros(0, np.uint16) if f in none else w[0] for f, w in enumerate(want)]
    ref_iq, ref_sy = Run(lphy, d, desc, n_iq, n_sym).tx(data.tobytes(), 0.75, 0x34)
    check_iq(ref_iq, desc, want_iq, "hand-written uncapped")
    for cap in TX_CAPS:
        d.grid_cap(cap)
        iq, syms = Run(lphy, d, desc, n_iq, n_sym).tx(data.tobytes(), 0.75, 0x34)
        check_iq(iq, desc, want_iq, f"hand-written cap {cap}")
        check_syms(syms, desc, want_sy, f"hand-written cap {cap}")
        np.testing.assert_array_equal(_iq_bits(iq), _iq_bits(ref_iq))
        np.testing.assert_array_equal(syms, ref_sy)
    assert d.bounds_violations() == 0
    d.close()


@pytest.mark.parametrize("cap", TX_CAPS)
def test_tx_repeat_capped(lphy, modulated, cap):
    """Two capped calls back to back into one buffer: the second parks its
    phases in the first's samples, also those of units read in a later trip."""
    sf = 7
    lens, pl = cycle_batch()
    d = lphy.Demodulator(sf, test_build=True)
    d.bounds_violations(reset=True)
    desc = d.tx_layout(lens)
    n_iq, n_sym = extent(d, lphy, desc)
    once, _ = Run(lphy, d, desc, n_iq, n_sym).tx(b"".join(pl))
    d.grid_cap(cap)
    run = Run(lphy, d, desc, n_iq, n_sym)
    t_data = run.torch.from_numpy(np.frombuffer(b"".join(pl), np.uint8).copy()).to(run.dev)
    for _ in range(2):
        d.tx_ragged(t_data, run.t_desc, run.frames, run.t_iq, run.t_syms, 1.0, 0x12, stream=run.stream,
                    iq_samples=n_iq, out_syms=n_sym)
    twice, _ = run.fetch()
    np.testing.assert_array_equal(_iq_bits(twice), _iq_bits(once))
    check_iq(twice, desc, [modulated(p, sf)[1] for p in pl], f"repeat cap {cap}")
    assert d.bounds_violations() == 0
    d.close()


@pytest.mark.parametrize("cap", TX_CAPS)
def test_tx_round_trip_capped(lphy, oracle, cap):
    """A capped transmit through a capped lphy_hip_demod_ragged (mode 2, decode) on the same table."""
    import torch
    sf = 7
    lens, pl = cycle_batch()
    d = lphy.Demodulator(sf, test_build=True)
    d.bounds_violations(reset=True)
    desc = d.tx_layout(lens)
    n_iq, n_sym = extent(d, lphy, desc)

    def round_trip():
        run = Run(lphy, d, desc, n_iq, n_sym)
        run.tx(b"".join(pl))
        t_syms = torch.zeros(max(n_sym, 1), dtype=torch.int16, device=run.dev)
        t_pay = torch.full(((n_sym + 1) // 2 + 1,), 0xEE, dtype=torch.uint8, device=run.dev)
        t_meta = torch.zeros(len(lens) * 32, dtype=torch.uint8, device=run.dev)
        d.demod_ragged(run.t_iq, run.t_desc, len(lens), t_syms, t_meta, lphy.MODE_DECHIRP_LORA_DEMODULATE,
                       lphy.F_DECODE, payload=t_pay, stream=run.stream, iq_samples=n_iq, out_syms=n_sym)
        torch.cuda.synchronize()
        return t_syms.cpu().numpy(), t_pay.cpu().numpy(), t_meta.cpu().numpy()
    ref = round_trip()
    d.grid_cap(cap)
    got = round_trip()
    same_outputs(got, ref, f"round trip cap {cap}")
    meta = got[2].view(lphy.META_DTYPE)
    assert np.all(meta["status"] == 0)
    for f, p in enumerate(pl):
        at = int(desc["sym_offset"][f]) // 2
        assert got[1][at: at + len(p)].tobytes() == p, f"frame {f}"
        # ... which is what the oracle's own chain gives for the frame alone
        r, osyms, _, _ = oracle.lora_demodulate(oracle.dechirp(oracle.modulate(oracle.encode(p), sf), sf), sf)
        assert r == 2 * len(p)
        so = int(desc["sym_offset"][f])
        np.testing.assert_array_equal(got[0].view(np.uint16)[so: so + r], osyms)
    assert got[1][sum(lens):].tobytes() == b"\xee" * (got[1].size - sum(lens))
    assert d.bounds_violations() == 0
    d.close()


# ---- the hook itself ---------------------------------------------------------
def test_cap_restores_and_large_cap_changes_nothing(oracle, lphy, frames_of):
    sf, mode = 9, 2
    frames = frames_of(sf, mode)
    lens, flat = [x.size for x in frames], np.concatenate(frames)
    d = _demod(lphy, sf)
    d.bounds_violations(reset=True)

    def call():
        return d.demod_ragged_host(flat, lens, mode, lphy.F_DECODE, fill=SENTINEL)
    ref = call()
    check_batch(oracle, sf, frames, mode, False, *ref, "default")
    tiles = -(-sum(COUNTS[sf]) // tile_of(sf))
    for cap in (1, 0, tiles + 1, 1 << 20, 0xFFFFFFFF, 0):   # 0 after a cap: the default again
        d.grid_cap(cap)
        same_outputs(call(), ref, f"cap {cap}")
    assert d.bounds_violations() == 0
    d.close()


def test_cap_is_per_context(oracle, lphy, frames_of):
    """A context made by lphy_hip_ctx_share from a capped one has no cap of its
    own: it takes and drops one independently, and both give the same bytes."""
    sf, mode = 9, 0
    frames = frames_of(sf, mode)
    lens, flat = [x.size for x in frames], np.concatenate(frames)
    base = _demod(lphy, sf)
    base.bounds_violations(reset=True)
    base.grid_cap(1)
    h = C.c_void_p()
    assert base.lib.lphy_hip_ctx_share(C.byref(h), base.ctx, 0) == 0
    other = copy.copy(base)
    other.ctx = h
    a = base.demod_ragged_host(flat, lens, mode, lphy.F_DECODE, fill=SENTINEL)
    b = other.demod_ragged_host(flat, lens, mode, lphy.F_DECODE, fill=SENTINEL)
    check_batch(oracle, sf, frames, mode, False, *a, "capped context")
    same_outputs(b, a, "shared context")
    other.grid_cap(3)
    base.grid_cap(0)
    same_outputs(other.demod_ragged_host(flat, lens, mode, lphy.F_DECODE, fill=SENTINEL), a, "shared context, cap 3")
    same_outputs(base.demod_ragged_host(flat, lens, mode, lphy.F_DECODE, fill=SENTINEL), a, "base, cap dropped")
    assert base.lib.lphy_hip_test_grid_cap(None, 1) == -22   # -EINVAL
    assert base.bounds_violations() == 0
    other.close()
    base.close()


def test_product_library_has_no_cap(lphy):
    d = lphy.Demodulator(7, lib_path=lphy.HIP_SO)
    with pytest.raises(AttributeError):
        d.grid_cap(1)
    d.close()
