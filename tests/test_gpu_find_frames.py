"""lphy_hip_find_frames / lphy_hip_find_frames_host (csrc/lphy_find.h): the
ragged table of the frames found in a capture, from hand-made detector records
(no IQ is read).  Both entry points are compared record for record, d_info
included, with the definition in plain numpy (tests/find_frames_model.py,
itself checked by tests/test_find_frames_cpu.py).

SF 7 (S = 128) throughout: the search has no transform, the SF only sets S."""
import numpy as np
import pytest

import find_frames_model as model

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -22, -34
SF, S = 7, 128
GUARD = 3  # records in front of and behind the table, which the call must leave alone


@pytest.fixture(scope="module")
def dem(lphy):
    d = lphy.Demodulator(SF)
    yield d
    d.close()


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _params(lphy, p):
    return lphy.find_params(p["first"], p["hop"], p["lead"], p["total_samples"], p["threshold_db"], p["max_gap"],
                            p["min_symbols"])


def device_call(lphy, d, rec, p, mode, max_frames, fill=0xA5):
    """The device form with the table between guard records, and the table, the
    info and the workspace pre-filled with `fill`: (desc, info)."""
    import torch
    dev = torch.device("cuda", d.device)
    windows = rec.size
    t_rec = torch.from_numpy(_u8(rec).copy() if windows else np.zeros(16, np.uint8)).to(dev)
    t_desc = torch.full(((max_frames + 1 + 2 * GUARD) * 32,), fill, dtype=torch.uint8, device=dev)
    t_info = torch.full((3 * 32,), fill, dtype=torch.uint8, device=dev)
    nwork = d.find_frames_workspace(windows)
    assert nwork > 0 and nwork % 16 == 0
    t_work = torch.full((nwork + 64,), fill, dtype=torch.uint8, device=dev)
    d.find_frames(t_rec if windows else None, windows, _params(lphy, p), mode, max_frames,
                  t_desc[GUARD * 32: (GUARD + max_frames + 1) * 32], t_info[32:64], t_work[:nwork],
                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    desc, info, work = t_desc.cpu().numpy(), t_info.cpu().numpy(), t_work.cpu().numpy()
    assert (desc[: GUARD * 32] == fill).all() and (desc[(GUARD + max_frames + 1) * 32:] == fill).all()
    assert (info[:32] == fill).all() and (info[64:] == fill).all() and (work[nwork:] == fill).all()
    return (desc[GUARD * 32: (GUARD + max_frames + 1) * 32].view(lphy.RAGGED_DESC_DTYPE).copy(),
            info[32:64].view(lphy.FIND_INFO).copy()[0])


def assert_same(lphy, got, want, what):
    (desc, info), (wdesc, winfo) = got, want
    np.testing.assert_array_equal(_u8(desc), _u8(wdesc.astype(lphy.RAGGED_DESC_DTYPE)), err_msg=f"{what}: table")
    assert {k: int(info[k]) for k in model.INFO_FIELDS} == winfo, what
    assert not info["reserved"].any(), what


def check(lphy, d, rec, p, mode, max_frames, what, forms=("device", "host")):
    want = model.find_frames(rec, p, S, mode, max_frames)
    if "device" in forms:
        assert_same(lphy, device_call(lphy, d, rec, p, mode, max_frames), want, f"{what}, device form")
    if "host" in forms:
        assert_same(lphy, d.find_frames_host(rec, _params(lphy, p), mode, max_frames), want, f"{what}, host form")
    return want


def pattern(name, n):
    rng = np.random.default_rng(1000 + n)
    if name == "none":
        return np.zeros(n, bool)
    if name == "all":
        return np.ones(n, bool)
    if name == "alternating":
        return np.arange(n) % 2 == 0
    return rng.random(n) < {"p05": 0.05, "p50": 0.5, "p95": 0.95}[name]


# ---- 1. sizes x patterns ---------------------------------------------------------
def sizes(lphy):
    T = lphy.FIND_TILE
    return [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, 40000]


@pytest.mark.parametrize("k", range(11))
def test_sizes_and_patterns(lphy, dem, k):
    n = sizes(lphy)[k]
    for name in ("none", "all", "alternating", "p05", "p50", "p95"):
        act = pattern(name, n)
        for max_gap in (0, 2):
            p = model.params(hop=S, total_samples=n * S, max_gap=max_gap)
            nb = len(model.bursts(act, max_gap))
            want = check(lphy, dem, model.records(act), p, 2, max(nb, 1) + 2, f"{n} windows, {name}, max_gap {max_gap}")
            assert want[1]["bursts"] == nb


# ---- 2. gaps and bursts against the tile, chunk and wavefront edges ----------------
@pytest.mark.parametrize("edge", ["tile", "two_tiles", "chunk", "wave"])
@pytest.mark.parametrize("extra", [0, 1])
def test_gap_of_max_gap_straddles_an_edge(lphy, dem, edge, extra):
    T = lphy.FIND_TILE
    at = {"tile": T, "two_tiles": 2 * T, "chunk": 256 + T, "wave": 64}[edge]
    max_gap = 5
    n = 3 * T
    for left in range(1, max_gap + 2):      # the gap's position across the edge
        act = np.zeros(n, bool)
        a = at - left                       # the last active window in front of the gap
        b = a + max_gap + extra + 1         # the first one behind it
        act[[a - 2, a, b, b + 3]] = True
        p = model.params(hop=S, total_samples=n * S, max_gap=max_gap)
        want = check(lphy, dem, model.records(act), p, 2, 4, f"{edge} edge, gap {max_gap + extra}, {left} in front",
                     forms=("device",))
        assert want[1]["bursts"] == 1 + extra


def test_bursts_over_whole_tiles_and_a_bridge_longer_than_a_tile(lphy, dem):
    T = lphy.FIND_TILE
    n = 8 * T + 17
    act = np.zeros(n, bool)
    act[T - 10: 3 * T + 10] = True           # covers tiles 1 and 2 whole
    act[5 * T: 6 * T] = True                 # exactly tile 5
    p = model.params(hop=S, total_samples=n * S, max_gap=3)
    want = check(lphy, dem, model.records(act), p, 2, 5, "bursts over whole tiles")
    assert want[1]["bursts"] == 2 and want[1]["frames"] == 2
    # max_gap = 5000: active windows 3999 and 5000 inactive ones apart are one burst
    # (tiles with no active window lie inside it), 5001 apart are two
    n = 16 * T
    act = np.zeros(n, bool)
    act[[100, 4100, 4100 + 5001, 4100 + 5001 + 5002]] = True
    p = model.params(hop=S, total_samples=n * S, max_gap=5000)
    assert 4100 + 5001 + 5002 < n
    want = check(lphy, dem, model.records(act), p, 2, 5, "a bridge longer than a tile")
    assert want[1]["bursts"] == 2 and [int(x) for x in want[0]["samples"][:2]] == [(9101 - 100 + 1) * S, S]
    # the last window of the capture active, and only it
    act = np.zeros(n, bool)
    act[-1] = True
    check(lphy, dem, model.records(act), p, 2, 2, "only the last window")


# ---- 3. values ----------------------------------------------------------------------
def test_values(lphy, dem):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    power = [-inf, inf, nan, 5.0, 12.5, 12.4999, inf, -3.0, 0.0]
    avg = [-inf, 0.0, 0.0, nan, 2.5, 2.5, inf, -inf, -10.0]
    rec = np.zeros(len(power) * 40, model.DETECT_DTYPE)   # the values 40 windows apart, all-zero windows between
    rec["power"], rec["power_avg"] = -inf, -inf
    rec["power"][::40], rec["power_avg"][::40] = power, avg
    rec["findex"], rec["index"] = nan, 0xFFFF              # fields the search does not read
    for thr, flags in ((10.0, [0, 1, 0, 0, 1, 0, 0, 1, 1]), (-np.inf, [0, 1, 0, 0, 1, 1, 0, 1, 1]),
                       (np.inf, [0, 1, 0, 0, 0, 0, 0, 1, 0])):
        assert list(model.active_flags(rec, thr)[::40]) == [bool(f) for f in flags], thr
        assert model.active_flags(rec, thr).sum() == sum(flags)
        p = model.params(hop=S, total_samples=rec.size * S, threshold_db=thr)
        want = check(lphy, dem, rec, p, 1, 12, f"threshold {thr}")
        assert want[1]["frames"] == sum(flags) == want[1]["active"]


# ---- 4. geometry -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("min_symbols", [1, 4])
def test_geometry(lphy, dem, mode, min_symbols):
    T = lphy.FIND_TILE
    n = 2 * T + 300
    rng = np.random.default_rng(5)
    act = np.zeros(n, bool)
    at = 3
    while at < n - 40:                      # bursts of 1 .. 30 windows, gaps of 1 .. 40
        ln = int(rng.integers(1, 31))
        act[at: at + ln] = True
        at += ln + int(rng.integers(1, 41))
    act[-9:] = True                         # the last burst reaches the last window
    rec = model.records(act)
    for what, hop, lead, first, total in (("hop = S", S, 0, 0, n * S),
                                          ("hop = S / 4, lead = S / 2", S // 4, S // 2, 640, 640 + n * S // 4 + S),
                                          ("hop = 3", 3, 0, 7, 7 + 3 * n),
                                          ("hop = 3, min over the clip", 3, 1, 7, 7 + 3 * n - 20),
                                          ("the last burst clipped", S, 0, 0, n * S - 5 * S - 1),
                                          ("the last burst clipped away", S, 0, 4096, 4096 + (n - 9) * S - 1),
                                          ("capture shorter than first", S, 0, 4096, 100)):
        p = model.params(first=first, hop=hop, lead=lead, total_samples=total, max_gap=1, min_symbols=min_symbols)
        want = check(lphy, dem, rec, p, mode, 200, f"{what}, mode {mode}, min_symbols {min_symbols}")
        d = want[0][: want[1]["frames"]]
        assert ((d["iq_offset"] + d["samples"]) <= total).all() and (d["samples"] % S == 0).all()
        assert (d["iq_offset"][1:] >= (d["iq_offset"] + d["samples"])[:-1]).all()


def test_dropped_long(lphy, dem):
    # hop = 2^24: 127 windows are below 2^31 samples, 128 are not
    n = 700
    act = np.zeros(n, bool)
    act[10:210] = True      # 200 windows: dropped_long
    act[300:427] = True     # 127: kept
    act[450:578] = True     # 128: exactly 2^31, dropped_long
    act[600] = True
    p = model.params(hop=1 << 24, total_samples=n << 24)
    want = check(lphy, dem, model.records(act), p, 2, 4, "hop = 2^24")
    assert want[1]["dropped_long"] == 2 and want[1]["frames"] == 2
    assert int(want[0]["samples"][0]) == 127 << 24


# ---- 5. capacity ----------------------------------------------------------------------------
def test_capacity(lphy, dem):
    T = lphy.FIND_TILE
    act = pattern("p05", 3 * T + 5)
    rec = model.records(act)
    p = model.params(hop=S, total_samples=rec.size * S, max_gap=2, min_symbols=2)
    count = model.find_frames(rec, p, S, 2, 10 ** 6)[1]["frames"]
    assert count > 8
    for max_frames in (1, count, count - 1, count + 7):
        want = check(lphy, dem, rec, p, 2, max_frames, f"max_frames {max_frames} of {count}")
        assert want[1]["frames"] == min(count, max_frames) and want[1]["overflow"] == max(0, count - max_frames)


# ---- 6. what the call does not touch, and that it repeats ---------------------------------------
@pytest.mark.parametrize("k", [8, 10])
def test_untouched_memory_and_repeat(lphy, dem, k):
    n = sizes(lphy)[k]
    rec = model.records(pattern("p50", n))
    p = model.params(hop=S, total_samples=n * S, max_gap=1)
    a = device_call(lphy, dem, rec, p, 2, 300, fill=0xA5)   # (the guards are checked in there)
    b = device_call(lphy, dem, rec, p, 2, 300, fill=0x5A)
    np.testing.assert_array_equal(_u8(a[0]), _u8(b[0]))
    assert a[1].tobytes() == b[1].tobytes()
    assert_same(lphy, a, model.find_frames(rec, p, S, 2, 300), "pre-filled with 0xA5")


# ---- 7. return codes ------------------------------------------------------------------------------
def test_return_codes(lphy, dem):
    import torch
    dev = torch.device("cuda", dem.device)
    L = dem.lib
    t = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    base = t.data_ptr()
    assert base % 16 == 0
    rec, desc, info, work = base, base + 4096, base + 8192, base + 16384
    h_rec = np.zeros(4, lphy.DETECT_DTYPE)
    h_desc = np.zeros(9, lphy.RAGGED_DESC_DTYPE)
    h_info = np.zeros(1, lphy.FIND_INFO)
    ok = dict(first=0, hop=S, lead=0, total_samples=4 * S, threshold_db=10.0, max_gap=0, min_symbols=1)

    def both(want, ctx=True, prm=ok, windows=4, mode=2, max_frames=8, null=(), work_at=work, reserved=0):
        pp = None if prm is None else lphy.find_params(reserved=reserved, **prm)
        p_prm = None if pp is None else pp.ctypes.data
        c = dem.ctx if ctx else None
        got = L.lphy_hip_find_frames(c, None if "rec" in null else rec, windows, p_prm, mode, max_frames,
                                     None if "desc" in null else desc, None if "info" in null else info,
                                     None if "work" in null else work_at, None)
        assert got == want, f"device form: {got}"
        if "work" in null or work_at != work:
            return                                  # the host form has no workspace argument
        got = L.lphy_hip_find_frames_host(c, None if "rec" in null else h_rec.ctypes.data, windows, p_prm, mode,
                                          max_frames, None if "desc" in null else h_desc.ctypes.data,
                                          None if "info" in null else h_info.ctypes.data)
        assert got == want, f"host form: {got}"

    both(0)
    both(EINVAL, ctx=False)
    both(EINVAL, prm=None)
    both(EINVAL, null=("desc",))
    both(EINVAL, null=("info",))
    both(EINVAL, null=("rec",))
    both(0, null=("rec",), windows=0)
    both(EINVAL, null=("work",))
    both(EINVAL, work_at=work + 8)
    both(EINVAL, prm=dict(ok, hop=0))
    both(EINVAL, prm=dict(ok, min_symbols=0))
    both(EINVAL, max_frames=0)
    both(EINVAL, prm=dict(ok, threshold_db=float("nan")))
    both(EINVAL, reserved=1)
    both(EINVAL, mode=-1)
    both(EINVAL, mode=3)
    # -EINVAL comes first; all -ERANGE cases are refused before any device call, so the small buffers do
    both(EINVAL, windows=1 << 32, mode=3)
    both(ERANGE, windows=1 << 32, prm=dict(ok, hop=1))
    both(ERANGE, max_frames=1 << 31)
    both(ERANGE, prm=dict(ok, first=(1 << 48) - 4 * S + 1))
    both(0, prm=dict(ok, first=(1 << 48) - 4 * S, total_samples=1 << 48))
    both(ERANGE, prm=dict(ok, lead=(1 << 64) - 1))
    both(ERANGE, prm=dict(ok, hop=(1 << 64) - 1))
    both(ERANGE, windows=1 << 31, prm=dict(ok, hop=2 * S))
    torch.cuda.synchronize()


# ---- 8. later trips of the persistent grids ----------------------------------------------------------
def test_grid_cap(lphy):
    d = lphy.Demodulator(SF, test_build=True)
    d.bounds_violations(reset=True)
    n = 40000
    rec = model.records(pattern("p50", n))
    p = model.params(hop=S, total_samples=n * S, max_gap=1)
    want = model.find_frames(rec, p, S, 2, 9000)
    assert want[1]["frames"] > 4000
    for cap in (0, 2, 1):
        d.grid_cap(cap)
        assert_same(lphy, device_call(lphy, d, rec, p, 2, 9000), want, f"cap {cap}, device form")
        assert_same(lphy, d.find_frames_host(rec, _params(lphy, p), 2, 9000), want, f"cap {cap}, host form")
    assert d.bounds_violations() == 0
    d.close()
