"""lphy_hip_find_frames's definition (include/lphy_hip.h, "Frame search") in
plain numpy: a loop over the active indices.  The expectation of
tests/test_find_frames_cpu.py, test_gpu_find_frames.py and
test_gpu_find_frames_chain.py."""
import numpy as np

DETECT_DTYPE = np.dtype([("power", "<f4"), ("power_avg", "<f4"), ("findex", "<f4"), ("index", "<u2"),
                         ("reserved", "<u2")])
DESC_DTYPE = np.dtype([("iq_offset", "<u8"), ("samples", "<u8"), ("sym_offset", "<u8"), ("unit_offset", "<u8")])
INFO_FIELDS = ("frames", "bursts", "dropped_short", "dropped_long", "overflow", "active")


def params(first=0, hop=128, lead=0, total_samples=0, threshold_db=10.0, max_gap=0, min_symbols=1):
    return dict(first=first, hop=hop, lead=lead, total_samples=total_samples, threshold_db=threshold_db,
                max_gap=max_gap, min_symbols=min_symbols)


def records(active, hi=30.0, lo=0.0):
    """Detector records whose power - power_avg is `hi` where `active`, else `lo`."""
    a = np.asarray(active, bool)
    rec = np.zeros(a.size, DETECT_DTYPE)
    rec["power"] = np.where(a, np.float32(hi), np.float32(lo))
    return rec


def active_flags(rec, threshold_db):
    """1: the float32 difference compared in float32; a NaN difference is inactive."""
    with np.errstate(invalid="ignore"):
        diff = (rec["power"].astype(np.float32) - rec["power_avg"].astype(np.float32)).astype(np.float32)
        return diff >= np.float32(threshold_db)


def out_syms(total, mode):
    """lphy_hip_syms_per_frame for `total` whole symbols."""
    return total - 2 if total >= 2 else (0 if mode == 0 else total)


def bursts(active, max_gap):
    """2: [(a, b)] of the active flags."""
    out = []
    for w in np.flatnonzero(active):
        w = int(w)
        if out and w - out[-1][1] - 1 <= max_gap:
            out[-1][1] = w
        else:
            out.append([w, w])
    return [(a, b) for a, b in out]


def find_frames(rec, p, step, mode, max_frames):
    """(desc[max_frames + 1], info dict) for the records `rec`, params `p`
    (see params()), step = S = N * osr."""
    act = active_flags(rec, p["threshold_db"])
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["active"] = int(act.sum())
    desc = np.zeros(max_frames + 1, DESC_DTYPE)
    end = sym = unit = 0
    for a, b in bursts(act, p["max_gap"]):
        info["bursts"] += 1
        start = p["first"] + p["lead"] + a * p["hop"]                                              # 3
        extent = 0 if start >= p["total_samples"] else min((b - a + 1) * p["hop"], p["total_samples"] - start)
        total = extent // step
        if total < p["min_symbols"]:                                                               # 4
            info["dropped_short"] += 1
            continue
        if total * step >= 1 << 31:
            info["dropped_long"] += 1
            continue
        if info["frames"] == max_frames:                                                           # 5
            info["overflow"] += 1
            continue
        desc[info["frames"]] = (start, total * step, sym, unit)                                    # 6
        info["frames"] += 1
        end = start + total * step
        sym += (out_syms(total, mode) + 1) & ~1
        unit += total
    desc[info["frames"]:] = (end, 0, sym, unit)                                                    # 7
    return desc, info
