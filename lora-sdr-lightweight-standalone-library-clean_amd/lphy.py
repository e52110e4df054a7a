"""Python binding of the MI355X LoRa PHY C ABI (include/lphy_hip.h).

Thin ctypes layer used by tests/, bench.py and __graft_entry__: it loads
lib/liblphy_hip.so (built in-tree by the package Makefile) and exposes the
batch entry points on device pointers (torch tensors) plus the host-buffer
conveniences.  There is no fallback: when the library or a HIP device is
missing, calls raise.

lib/test/liblphy_hip.so is the test-only build (Makefile `test`): the same
kernels with device index checks (-DLPHY_DEBUG_BOUNDS, counted in
bounds_violations()) and the comparison flags F_EXACT_ROTATION /
F_SCAN_FIRST / F_DEBUG_RECHECK (csrc/lphy_testing.h), which the product
library rejects.  Demodulator(..., test_build=True) uses it; LPHY_LIB=test
makes it the default (a whole test run under the index checks).
"""
from __future__ import annotations

import ctypes as C
import errno
import os
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
LIB_DIR = PKG / "lib"
HIP_SO = LIB_DIR / "liblphy_hip.so"
TEST_SO = LIB_DIR / "test" / "liblphy_hip.so"
# LPHY_LIB=test: the test build; LPHY_LIB=<path>: another build of the
# library (timing experiments, tools/ubench/variants.py)
_ENV_LIB = os.environ.get("LPHY_LIB", "")
DEFAULT_SO = TEST_SO if _ENV_LIB == "test" else (Path(_ENV_LIB) if _ENV_LIB else HIP_SO)
SHIM_SO = LIB_DIR / "liblora_phy_amd.so"

MODE_DEMODULATE = 0
MODE_LORA_DEMODULATE = 1
MODE_DECHIRP_LORA_DEMODULATE = 2
F_DECODE = 1
F_NO_SCRATCH = 2
F_STAGE_PROLOGUE = 4
F_STAGE_SYMBOLS = 8
F_STAGE_FINAL = 16
F_UNFUSED = 32  # separate prologue / symbol launches (lphy_hip.h)
# test-only build (csrc/lphy_testing.h; the product library returns -EINVAL):
F_EXACT_ROTATION = 64  # every symbol with the reference's per-sample rotation
F_SCAN_FIRST = 256  # modes 1/2: whole-frame max-abs pre-scan (no speculation)
F_DEBUG_RECHECK = 512  # every symbol / estimated frame left to the exact re-run
F_FRAMES_KERNEL = 1024  # SF 7-10: k_frames where k_wave would run (test build; the certificate tests on k_frames)
# lphy_hip_test_libm's ops (test build; csrc/lphy_testing.h lphy_test_libm_op)
(LIBM_SINCOS_EXACT, LIBM_SINCOS_SPLIT, LIBM_SINCOS_LARGE, LIBM_ATAN2, LIBM_CABS, LIBM_LOGF, LIBM_LOG10F,
 LIBM_SQRTF, LIBM_DETECTOR_POWER) = range(9)
WINDOW_NONE = 0
WINDOW_HANN = 1
# Smallest batch new Demodulators send to the fused kernels
# (lphy_hip_ctx_set_fused_min_frames); None keeps the library's measured
# per-SF crossover.  The test suite sets 0 (tests/conftest.py) so that its
# small batches run the fused kernels.
FUSED_MIN_FRAMES = None


class FrameMeta(C.Structure):
    _fields_ = [
        ("cfo", C.c_float), ("time_offset", C.c_float), ("rate", C.c_float),
        ("scale", C.c_float), ("t_off", C.c_int32), ("status", C.c_int32),
        ("sw0", C.c_uint16), ("sw1", C.c_uint16), ("sync_word", C.c_uint8),
        ("crc_ok", C.c_uint8), ("normalised", C.c_uint8), ("have_sync", C.c_uint8),
    ]


assert C.sizeof(FrameMeta) == 32

META_DTYPE = np.dtype([
    ("cfo", "<f4"), ("time_offset", "<f4"), ("rate", "<f4"), ("scale", "<f4"),
    ("t_off", "<i4"), ("status", "<i4"), ("sw0", "<u2"), ("sw1", "<u2"),
    ("sync_word", "u1"), ("crc_ok", "u1"), ("normalised", "u1"), ("have_sync", "u1"),
])
assert META_DTYPE.itemsize == 32

# lphy_ragged_desc (include/lphy_hip.h): frames + 1 records per ragged call
RAGGED_DESC_DTYPE = np.dtype([("iq_offset", "<u8"), ("samples", "<u8"), ("sym_offset", "<u8"),
                              ("unit_offset", "<u8")])
assert RAGGED_DESC_DTYPE.itemsize == 32


# lphy_detect_rec (include/lphy_hip.h): one record per detector window
class DetectRec(C.Structure):
    _fields_ = [("power", C.c_float), ("power_avg", C.c_float), ("findex", C.c_float),
                ("index", C.c_uint16), ("reserved", C.c_uint16)]


assert C.sizeof(DetectRec) == 16
DETECT_DTYPE = np.dtype([("power", "<f4"), ("power_avg", "<f4"), ("findex", "<f4"), ("index", "<u2"),
                         ("reserved", "<u2")])
assert DETECT_DTYPE.itemsize == 16
DET_DECHIRP = 1  # lphy_hip_detect_*: the context's down-chirp on every window first

# lphy_find_params / lphy_find_info (include/lphy_hip.h): the frame search
FIND_PARAMS = np.dtype([("first", "<u8"), ("hop", "<u8"), ("lead", "<u8"), ("total_samples", "<u8"),
                        ("threshold_db", "<f4"), ("max_gap", "<u4"), ("min_symbols", "<u4"), ("reserved", "<u4")])
assert FIND_PARAMS.itemsize == 48
FIND_INFO = np.dtype([("frames", "<u4"), ("bursts", "<u4"), ("dropped_short", "<u4"), ("dropped_long", "<u4"),
                      ("overflow", "<u4"), ("active", "<u4"), ("reserved", "<u4", (2,))])
assert FIND_INFO.itemsize == 32
FIND_TILE = 1024  # windows per tile of the search's passes (csrc/lphy_find_scan.h kFindTile)


def find_params(first=0, hop=0, lead=0, total_samples=0, threshold_db=0.0, max_gap=0, min_symbols=1,
                reserved=0) -> np.ndarray:
    """One FIND_PARAMS record."""
    p = np.zeros(1, FIND_PARAMS)
    p[0] = (first, hop, lead, total_samples, threshold_db, max_gap, min_symbols, reserved)
    return p

# lphy_chan_plan (include/lphy_hip.h): the channeliser
CHAN_PLAN = np.dtype([("first", "<u8"), ("in_samples", "<u8"), ("outputs", "<u8"), ("out_stride", "<u8"),
                      ("rot_first", "<u8"), ("channels", "<u4"), ("taps", "<u4"), ("decim", "<u4"),
                      ("rot_period", "<u4"), ("reserved", "<u4", (2,))])
assert CHAN_PLAN.itemsize == 64
CHAN_TILE = 256  # outputs of every channel per workgroup (csrc/lphy_resample_plan.h kResTile)


def chan_plan(first=0, in_samples=0, outputs=0, out_stride=0, rot_first=0, channels=0, taps=0, decim=0,
              rot_period=0, reserved=(0, 0)) -> np.ndarray:
    """One CHAN_PLAN record."""
    p = np.zeros(1, CHAN_PLAN)
    p[0] = (first, in_samples, outputs, out_stride, rot_first, channels, taps, decim, rot_period, reserved)
    return p


def channelize_outputs(in_samples: int, first: int, taps: int, decim: int) -> int:
    """The largest `outputs` for which every tap lies inside a capture of
    in_samples (lphy_hip_channelize_outputs); 0 when there is none."""
    return int(load().lphy_hip_channelize_outputs(in_samples, first, taps, decim))


# enum lphy_sample_format (include/lphy_hip.h): what a capture's I/Q pairs are made of
FMT_CF32, FMT_SC16, FMT_SC8, FMT_CU8 = 0, 1, 2, 3
_FMT_DTYPE = {FMT_CF32: np.dtype(np.float32), FMT_SC16: np.dtype("<i2"), FMT_SC8: np.dtype(np.int8),
              FMT_CU8: np.dtype(np.uint8)}


def sample_bytes(fmt: int) -> int:
    """Bytes of one I/Q pair of format `fmt` (lphy_hip_sample_bytes): 8, 4, 2,
    2; 0 for anything else."""
    return int(load().lphy_hip_sample_bytes(fmt))


def _fmt_dtype(fmt: int) -> np.dtype:
    if fmt not in _FMT_DTYPE:
        raise ValueError(f"fmt: one of FMT_CF32, FMT_SC16, FMT_SC8, FMT_CU8 expected, got {fmt!r}")
    return _FMT_DTYPE[fmt]


def _design_tables(who: str, centres, step: int, taps: int, cutoff: float, beta: float, synth: bool):
    """What chan_design and synth_design share: the Kaiser(beta)-windowed sinc
    with unit gain at DC, the exact (Fraction) phase reduction, the period R of
    centre * step and its limit.  synth: the mixer turns forward, exp(+i ...),
    and the prototype is scaled by `step`; else backward, unscaled."""
    import math
    from fractions import Fraction
    cs = [Fraction(c) for c in centres]
    if not cs or taps < 1 or step < 1:
        raise ValueError(f"{who}: at least one centre, one tap and a step >= 1")
    R = 1
    for c in cs:
        R = math.lcm(R, (c * step).denominator)
    if R > 65536:
        raise ValueError(f"{who}: rotation period {R} exceeds 65536")
    k = np.arange(taps, dtype=np.float64)
    h = 2.0 * cutoff * np.sinc(2.0 * cutoff * (k - (taps - 1) / 2.0)) * np.kaiser(taps, beta)
    h = h / h.sum()
    if synth:
        h = h * float(step)
    t = np.empty((len(cs), taps), np.complex128)
    r = np.empty((len(cs), R), np.complex128)
    for i, c in enumerate(cs):
        pt = 2.0 * np.pi * np.array([float((c * n) % 1) for n in range(taps)])
        pr = 2.0 * np.pi * np.array([float((c * step * n) % 1) for n in range(R)])
        if synth:
            t[i] = h * (np.cos(pt) + 1j * np.sin(pt))
            r[i] = np.cos(pr) + 1j * np.sin(pr)
        else:
            t[i] = h * (np.cos(pt) - 1j * np.sin(pt))
            r[i] = np.cos(pr) - 1j * np.sin(pr)
    return t.astype(np.complex64), r.astype(np.complex64), R, (taps - 1) / 2.0


def chan_design(centres, decim: int, taps: int, cutoff: float, beta: float):
    """Tables for lphy_hip_channelize from channel centres: `centres` are
    fractions.Fraction cycles per input sample, `cutoff` the low-pass edge in
    cycles per input sample.  Returns (taps complex64 [C, T], rot complex64
    [C, R], R, delay): channel c is the input times exp(-2 pi i centre n),
    through a Kaiser(beta)-windowed sinc of `taps` coefficients with unit gain
    at DC, every `decim`-th sample; delay = (taps - 1) / 2 input samples.  The
    phases are reduced exactly (Fraction arithmetic), everything else is
    float64, rounded to float32 once.  R is the least common period of
    centre * decim; ValueError when it exceeds 65536."""
    return _design_tables("chan_design", centres, decim, taps, cutoff, beta, synth=False)


# lphy_synth_plan (include/lphy_hip.h): the synthesiser
SYNTH_PLAN = np.dtype([("first", "<u8"), ("in_samples", "<u8"), ("in_stride", "<u8"), ("outputs", "<u8"),
                       ("rot_first", "<u8"), ("channels", "<u4"), ("taps", "<u4"), ("interp", "<u4"),
                       ("rot_period", "<u4"), ("reserved", "<u4", (2,))])
assert SYNTH_PLAN.itemsize == 64
SYNTH_TILE = 256  # wideband outputs per workgroup (csrc/lphy_resample_plan.h kResTile)


def synth_plan(first=0, in_samples=0, in_stride=0, outputs=0, rot_first=0, channels=0, taps=0, interp=0,
               rot_period=0, reserved=(0, 0)) -> np.ndarray:
    """One SYNTH_PLAN record."""
    p = np.zeros(1, SYNTH_PLAN)
    p[0] = (first, in_samples, in_stride, outputs, rot_first, channels, taps, interp, rot_period, reserved)
    return p


def synthesize_outputs(in_samples: int, first: int, taps: int, interp: int) -> int:
    """The outputs from `first` up to the last one an input sample reaches
    (lphy_hip_synthesize_outputs): (in_samples - 1) * interp + taps - first, 0
    when that is not positive."""
    return int(load().lphy_hip_synthesize_outputs(in_samples, first, taps, interp))


def synth_design(centres, interp: int, taps: int, cutoff: float, beta: float):
    """Tables for lphy_hip_synthesize from channel centres, the mirror of
    chan_design: `centres` are fractions.Fraction cycles per wideband sample,
    `cutoff` the low-pass edge in cycles per wideband sample.  Returns (taps
    complex64 [C, T], rot complex64 [C, R], R, delay): channel c's stream is
    zero-stuffed by `interp`, passed through `interp` times a
    Kaiser(beta)-windowed sinc of `taps` coefficients with unit gain at DC
    (unit gain for the stream, that is) and multiplied by exp(+2 pi i centre
    w); narrow sample j is centred at wideband sample j * interp + delay,
    delay = (taps - 1) / 2.  taps[c, k] = interp * h[k] * exp(+2 pi i centre
    k), rot[c, j] = exp(+2 pi i centre interp j): the conjugates of
    chan_design's for decim = interp, the taps times interp.  The phases are
    reduced exactly (Fraction arithmetic), everything else is float64, rounded
    to float32 once.  R is the least common period of centre * interp;
    ValueError when it exceeds 65536."""
    return _design_tables("synth_design", centres, interp, taps, cutoff, beta, synth=True)


_vp = C.c_void_p
_sz = C.c_size_t

EXPORTS = (
    "lphy_hip_ctx_create", "lphy_hip_ctx_destroy", "lphy_hip_ctx_share", "lphy_hip_ctx_reserve",
    "lphy_hip_ctx_set_fused_min_frames",
    "lphy_hip_syms_per_frame", "lphy_hip_recheck_count", "lphy_hip_bounds_violations",
    "lphy_hip_demod_batch", "lphy_hip_decode_batch", "lphy_hip_estimate_batch",
    "lphy_hip_compensate", "lphy_hip_modulate_batch", "lphy_hip_demod_host",
    "lphy_hip_decode_host", "lphy_hip_estimate_host", "lphy_hip_compensate_host",
    "lphy_hip_modulate_host", "lphy_hip_demod_stream", "lphy_hip_sync", "lphy_hip_version",
    "lphy_hip_gray_batch", "lphy_hip_interleave_batch", "lphy_hip_deinterleave_batch",
    "lphy_hip_whiten_batch", "lphy_hip_hamming_batch", "lphy_hip_checksum_batch",
    "lphy_hip_lora_encode_batch", "lphy_hip_lorawan_mic_batch", "lphy_hip_lorawan_parse_batch",
    "lphy_hip_lorawan_mic_host",
    "lphy_hip_ragged_layout", "lphy_hip_demod_ragged", "lphy_hip_demod_ragged_host",
    "lphy_hip_detect_batch", "lphy_hip_detect_host", "lphy_hip_detect_serial_count",
    "lphy_hip_compensate_batch", "lphy_hip_compensate_ragged", "lphy_hip_compensate_batch_host",
    "lphy_hip_modulate_ragged", "lphy_hip_tx_ragged", "lphy_hip_tx_ragged_host", "lphy_hip_tx_layout",
    "lphy_hip_estimate_ragged", "lphy_hip_estimate_ragged_host",
    "lphy_hip_detect_ragged", "lphy_hip_detect_ragged_host",
    "lphy_hip_find_frames_workspace", "lphy_hip_find_frames", "lphy_hip_find_frames_host",
    "lphy_hip_channelize_outputs", "lphy_hip_channelize", "lphy_hip_channelize_host",
    "lphy_hip_sample_bytes", "lphy_hip_channelize_raw", "lphy_hip_channelize_raw_host",
    "lphy_hip_synthesize_outputs", "lphy_hip_synthesize", "lphy_hip_synthesize_host",
    "lphy_hip_symbol_samples", "lphy_hip_lorawan_build_ragged", "lphy_hip_lorawan_tx_layout",
    "lphy_hip_lorawan_parse_ragged", "lphy_hip_lorawan_sessions_check",
    "lphy_hip_lorawan_crypt_batch", "lphy_hip_lorawan_crypt_tx_ragged", "lphy_hip_lorawan_crypt_rx_ragged",
    "lphy_hip_lorawan_crypt_host",
)

WHITEN_SX1232, WHITEN_SX1272, WHITEN_SX1272_LFSR = 0, 1, 2
CODE_ENC84, CODE_DEC84, CODE_ENC74, CODE_DEC74 = 0, 1, 2, 3
CODE_ENCP54, CODE_CHKP54, CODE_ENCP64, CODE_CHKP64 = 4, 5, 6, 7
SUM_SX1272_CRC, SUM_HEADER, SUM_CHECKSUM8 = 0, 1, 2

_LIBS: dict = {}


class LphyError(RuntimeError):
    def __init__(self, rc: int, what: str):
        name = errno.errorcode.get(-rc, str(rc))
        super().__init__(f"{what} failed: -{name} ({rc})")
        self.rc = rc


def use(path) -> C.CDLL:
    """Make the library at `path` the default of later load() / Demodulator
    calls (experiment builds: tools/ubench) and load it."""
    global DEFAULT_SO
    DEFAULT_SO = Path(path)
    return load(DEFAULT_SO)


def load(path: Path | None = None) -> C.CDLL:
    """Load liblphy_hip.so (raises if it was not built); `path` picks another
    build (TEST_SO), default DEFAULT_SO."""
    path = Path(path or DEFAULT_SO)
    if str(path) in _LIBS:
        return _LIBS[str(path)]
    if not path.exists():
        raise FileNotFoundError(f"{path} missing: build with __graft_entry__.build()")
    # One HIP runtime per process: torch ships its own libamdhip64 (SONAME
    # libamdhip64.so.7) and asks for it by the unversioned name.  Loaded
    # first, it also satisfies our NEEDED libamdhip64.so.7; loaded after
    # /opt/rocm's copy, a second runtime instance appears and torch then
    # sees no device.  So bring torch's in before ours when torch exists.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(str(path))
    L.lphy_hip_ctx_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_int]
    L.lphy_hip_ctx_destroy.argtypes = [_vp]
    L.lphy_hip_ctx_destroy.restype = None
    L.lphy_hip_ctx_share.argtypes = [C.POINTER(_vp), _vp, C.c_uint]
    L.lphy_hip_ctx_reserve.argtypes = [_vp, _sz, _sz]
    L.lphy_hip_ctx_set_fused_min_frames.argtypes = [_vp, C.c_long]
    L.lphy_hip_bounds_violations.argtypes = [_vp, C.POINTER(C.c_ulonglong), C.c_int]
    L.lphy_hip_syms_per_frame.argtypes = [_vp, _sz, C.c_int]
    L.lphy_hip_syms_per_frame.restype = _sz
    L.lphy_hip_demod_batch.argtypes = [_vp, _vp, _sz, _sz, _vp, _vp, _vp, C.c_int, C.c_uint, _vp]
    L.lphy_hip_ragged_layout.argtypes = [_vp, _vp, _sz, C.c_int, _vp]
    L.lphy_hip_demod_ragged.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, _vp, C.c_int, C.c_uint, _vp]
    L.lphy_hip_demod_ragged_host.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, _vp, C.c_int, C.c_uint]
    L.lphy_hip_detect_batch.argtypes = [_vp, _vp, _sz, _sz, _sz, _sz, _sz, _vp, C.c_uint, _vp]
    L.lphy_hip_detect_host.argtypes = [_vp, _vp, _sz, _sz, _sz, _sz, _sz, _vp, C.c_uint]
    L.lphy_hip_detect_serial_count.argtypes = [_vp, C.POINTER(C.c_ulonglong), C.c_int]
    L.lphy_hip_detect_ragged.argtypes = [_vp, _vp, _vp, _sz, C.c_uint, _vp, C.c_uint, _vp]
    L.lphy_hip_detect_ragged_host.argtypes = [_vp, _vp, _vp, _sz, C.c_uint, _vp, C.c_uint]
    L.lphy_hip_find_frames_workspace.argtypes = [_sz]
    L.lphy_hip_find_frames_workspace.restype = _sz
    L.lphy_hip_find_frames.argtypes = [_vp, _vp, _sz, _vp, C.c_int, _sz, _vp, _vp, _vp, _vp]
    L.lphy_hip_find_frames_host.argtypes = [_vp, _vp, _sz, _vp, C.c_int, _sz, _vp, _vp]
    L.lphy_hip_channelize_outputs.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    L.lphy_hip_channelize_outputs.restype = C.c_uint64
    L.lphy_hip_channelize.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp]
    L.lphy_hip_channelize_host.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp]
    L.lphy_hip_sample_bytes.argtypes = [C.c_int]
    L.lphy_hip_sample_bytes.restype = _sz
    L.lphy_hip_channelize_raw.argtypes = [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]
    L.lphy_hip_channelize_raw_host.argtypes = [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp]
    L.lphy_hip_synthesize_outputs.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    L.lphy_hip_synthesize_outputs.restype = C.c_uint64
    L.lphy_hip_synthesize.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp]
    L.lphy_hip_synthesize_host.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp]
    L.lphy_hip_decode_batch.argtypes = [_vp, _vp, _sz, _sz, _vp, _vp, _vp]
    L.lphy_hip_estimate_batch.argtypes = [_vp, _vp, _sz, _sz, _sz, _vp, _vp]
    L.lphy_hip_estimate_ragged.argtypes = [_vp, _vp, _vp, _sz, _sz, _vp, _vp]
    L.lphy_hip_estimate_ragged_host.argtypes = [_vp, _vp, _vp, _sz, _sz, _vp]
    L.lphy_hip_compensate.argtypes = [_vp, _vp, _sz, C.c_float, C.c_float, _vp]
    L.lphy_hip_compensate_batch.argtypes = [_vp, _vp, _vp, _sz, _sz, _vp, _vp]
    L.lphy_hip_compensate_ragged.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _vp]
    L.lphy_hip_compensate_batch_host.argtypes = [_vp, _vp, _sz, _sz, _vp]
    L.lphy_hip_modulate_batch.argtypes = [_vp, _vp, _sz, _sz, _vp, C.c_float, C.c_uint8, _vp]
    L.lphy_hip_modulate_ragged.argtypes = [_vp, _vp, _vp, _sz, _vp, C.c_float, C.c_uint8, _vp]
    L.lphy_hip_tx_ragged.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, C.c_float, C.c_uint8, _vp]
    L.lphy_hip_tx_ragged_host.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, C.c_float, C.c_uint8]
    L.lphy_hip_tx_layout.argtypes = [_vp, _vp, _sz, _vp]
    L.lphy_hip_demod_host.argtypes = [_vp, _vp, _sz, _sz, _vp, _vp, _vp, C.c_int, C.c_uint]
    L.lphy_hip_decode_host.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.lphy_hip_estimate_host.argtypes = [_vp, _vp, _sz, _vp]
    L.lphy_hip_compensate_host.argtypes = [_vp, _vp, _sz, C.c_float, C.c_float]
    L.lphy_hip_modulate_host.argtypes = [_vp, _vp, _sz, _vp, C.c_float, C.c_uint8]
    L.lphy_hip_demod_stream.argtypes = [_vp, C.c_int, _sz, _sz, C.c_int, C.c_uint, _sz, _vp, _vp,
                                        _vp, C.POINTER(_sz), C.POINTER(_sz)]
    L.lphy_hip_sync.argtypes = [_vp]
    L.lphy_hip_recheck_count.argtypes = [_vp, C.POINTER(C.c_ulonglong), C.c_int]
    L.lphy_hip_version.restype = C.c_char_p
    L.lphy_hip_gray_batch.argtypes = [_vp, _sz, C.c_int, _vp]
    L.lphy_hip_interleave_batch.argtypes = [_vp, _sz, _sz, _sz, _vp, _sz, C.c_uint, C.c_uint, _vp]
    L.lphy_hip_deinterleave_batch.argtypes = [_vp, _sz, _sz, _sz, _vp, _sz, C.c_uint, C.c_uint, _vp]
    L.lphy_hip_whiten_batch.argtypes = [_vp, _sz, _sz, _sz, C.c_int, C.c_int, C.c_uint, _vp]
    L.lphy_hip_hamming_batch.argtypes = [_vp, _sz, C.c_int, _vp, _vp]
    L.lphy_hip_checksum_batch.argtypes = [_vp, _sz, _sz, _sz, C.c_int, _vp, _vp]
    L.lphy_hip_lora_encode_batch.argtypes = [_vp, _sz, _sz, _sz, _vp, _sz, _vp]
    L.lphy_hip_lorawan_mic_batch.argtypes = [_vp, _vp, _sz, _vp, _sz, _vp, C.c_uint, _vp]
    L.lphy_hip_lorawan_parse_batch.argtypes = [_vp, _sz, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp]
    L.lphy_hip_lorawan_mic_host.argtypes = [C.c_int, _vp, C.c_int, C.c_uint32, C.c_uint32, _vp, _sz,
                                            C.POINTER(C.c_uint32)]
    L.lphy_hip_symbol_samples.argtypes = [_vp]
    L.lphy_hip_symbol_samples.restype = _sz
    L.lphy_hip_lorawan_build_ragged.argtypes = [_vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp, _vp]
    L.lphy_hip_lorawan_tx_layout.argtypes = [_vp, _vp, _sz, _vp]
    L.lphy_hip_lorawan_parse_ragged.argtypes = [_vp, _vp, _sz, _sz, C.c_int, _vp, _vp, _sz, _vp, _vp, _sz, _vp,
                                                _vp, _vp]
    L.lphy_hip_lorawan_sessions_check.argtypes = [_vp, _sz]
    L.lphy_hip_lorawan_crypt_batch.argtypes = [_vp, _vp, _sz, _vp, _sz, _vp, _vp]
    L.lphy_hip_lorawan_crypt_tx_ragged.argtypes = [_vp, _vp, _sz, _vp, _sz, C.c_uint, _vp, _vp]
    L.lphy_hip_lorawan_crypt_rx_ragged.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, C.c_int, _vp, _sz, C.c_uint, _vp,
                                                   _vp]
    L.lphy_hip_lorawan_crypt_host.argtypes = [C.c_int, _vp, C.c_int, C.c_uint32, C.c_uint32, _vp, _sz]
    _LIBS[str(path)] = L
    return L


def _chk(rc: int, what: str) -> None:
    if rc != 0:
        raise LphyError(rc, what)


def _ptr(a) -> int | None:
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()  # torch tensor


def _dev_buf(t, name: str, device: int, nbytes: int, itemsize: int | None = None) -> int:
    """Pointer of a device tensor after checking what the C ABI cannot: it
    lives on the context's HIP device, is contiguous, has the element size
    the kernels write (when given) and holds at least `nbytes`.  A wrong
    buffer would otherwise become a silent out-of-bounds device access."""
    if t is None or isinstance(t, np.ndarray) or not hasattr(t, "data_ptr"):
        raise ValueError(f"{name}: expected a device tensor, got {type(t).__name__}")
    if t.device.type != "cuda" or (t.device.index or 0) != device:
        raise ValueError(f"{name}: tensor on {t.device}, context on cuda:{device}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    if itemsize is not None and t.element_size() != itemsize:
        raise ValueError(f"{name}: {itemsize}-byte elements expected, got {t.dtype}")
    have = t.numel() * t.element_size()
    if have < nbytes:
        raise ValueError(f"{name}: {have} bytes, the call writes/reads {nbytes}")
    return t.data_ptr()


# what channelize / synthesize and their *_host forms share
def _one_plan(plan, dtype, name: str):
    p = np.ascontiguousarray(plan, dtype).reshape(-1)
    if p.size != 1:
        raise ValueError(f"plan: one {name} record expected, got {p.size}")
    return p, p[0]


def _tables_bufs(taps, rot, device: int, q):
    ch = int(q["channels"])
    return (_dev_buf(taps, "taps", device, ch * int(q["taps"]) * 8, None),
            _dev_buf(rot, "rot", device, ch * int(q["rot_period"]) * 8, None))


_PAD = np.zeros(1, np.complex64)  # an empty array's stand-in: never read, never written


def _host_ptrs(*arrays):
    return [(a if a.size else _PAD).ctypes.data for a in arrays]


class Demodulator:
    """One (sf, bw, osr, window) configuration on one HIP device."""

    def __init__(self, sf: int, bw_hz: int = 125000, osr: int = 1,
                 window: int = WINDOW_NONE, device: int = 0, test_build: bool = False,
                 lib_path=None):
        self.lib = load(lib_path or (TEST_SO if test_build else None))
        self.sf, self.N, self.bw_hz, self.osr = sf, 1 << sf, bw_hz, osr
        self.window, self.device = window, device
        h = _vp()
        _chk(self.lib.lphy_hip_ctx_create(C.byref(h), device, sf, bw_hz, osr, window),
             "lphy_hip_ctx_create")
        self.ctx = h
        if FUSED_MIN_FRAMES is not None:
            self.set_fused_min_frames(FUSED_MIN_FRAMES)

    def set_fused_min_frames(self, frames: int) -> None:
        """Smallest batch that takes the fused kernels on this context
        (< 0: the library's measured per-SF crossover)."""
        _chk(self.lib.lphy_hip_ctx_set_fused_min_frames(self.ctx, int(frames)),
             "lphy_hip_ctx_set_fused_min_frames")

    def close(self):
        if self.ctx:
            self.lib.lphy_hip_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def syms_per_frame(self, frame_samples: int, mode: int) -> int:
        return self.lib.lphy_hip_syms_per_frame(self.ctx, frame_samples, mode)

    def symbol_samples(self) -> int:
        """N * osr: the samples of one symbol (lphy_hip_symbol_samples), what
        lorawan_build_ragged / lorawan_parse_ragged take for this context."""
        return int(self.lib.lphy_hip_symbol_samples(self.ctx))

    def lorawan_tx_layout(self, tx) -> np.ndarray:
        """Descriptors (RAGGED_DESC_DTYPE, len(tx) + 1 records) of the LoRaWAN
        frames of `tx` (LORAWAN_TX_DTYPE), packed back to back: tx_layout on
        12 + fopts_len + payload_len bytes each (lphy_hip_lorawan_tx_layout)."""
        t = np.ascontiguousarray(tx, LORAWAN_TX_DTYPE).reshape(-1)
        desc = np.zeros(t.size + 1, RAGGED_DESC_DTYPE)
        _chk(self.lib.lphy_hip_lorawan_tx_layout(self.ctx, t.ctypes.data if t.size else None, t.size,
                                                 desc.ctypes.data), "lphy_hip_lorawan_tx_layout")
        return desc

    # --- device batch API (torch tensors) --------------------------------
    def demod_batch(self, iq, frames, frame_samples, syms, meta, mode, flags=0,
                    payload=None, stream=None):
        per = self.syms_per_frame(frame_samples, mode)
        dv = self.device
        p_iq = _dev_buf(iq, "iq", dv, frames * frame_samples * 8, None)
        p_syms = _dev_buf(syms, "syms", dv, frames * per * 2, 2)
        p_meta = _dev_buf(meta, "meta", dv, frames * 32, None)
        p_pay = None
        if flags & F_DECODE:
            p_pay = _dev_buf(payload, "payload", dv, frames * (per // 2), 1)
        _chk(self.lib.lphy_hip_demod_batch(self.ctx, p_iq, frames, frame_samples,
                                           p_syms, p_pay, p_meta, mode, flags, stream),
             "lphy_hip_demod_batch")

    # --- ragged batches: frames of different lengths in one call ---------
    def ragged_layout(self, lengths, mode: int) -> np.ndarray:
        """Descriptors (RAGGED_DESC_DTYPE, len(lengths) + 1 records) of frames
        of `lengths` samples packed back to back; record [-1] holds the
        totals (lphy_hip_ragged_layout)."""
        n = np.ascontiguousarray(lengths, np.uint64).reshape(-1)
        desc = np.zeros(n.size + 1, RAGGED_DESC_DTYPE)
        _chk(self.lib.lphy_hip_ragged_layout(self.ctx, n.ctypes.data if n.size else None, n.size, mode,
                                             desc.ctypes.data), "lphy_hip_ragged_layout")
        return desc

    def _ragged_extents(self, desc: np.ndarray, mode: int):
        """(IQ samples, output symbols, whole symbols, bytes a transmit call
        reads) the descriptors span."""
        d = desc[:-1]
        total = d["samples"] // np.uint64(self.N * self.osr)
        data = total - np.minimum(total, 2)  # behind the two sync symbols
        per = np.where(total >= 2, data, 0 if mode == MODE_DEMODULATE else total).astype(np.uint64)

        def top(a):
            return int(a.max()) if a.size else 0
        return (top(d["iq_offset"] + d["samples"]), top(d["sym_offset"] + per), int(desc["unit_offset"][-1]),
                top(d["sym_offset"] // np.uint64(2) + data // np.uint64(2)))

    def _ragged_extent(self, desc: np.ndarray, mode: int):
        """(IQ samples, output symbols) the descriptors span: for callers that
        size device buffers themselves."""
        return self._ragged_extents(desc, mode)[:2]

    def demod_ragged(self, iq, desc, frames, syms, meta, mode, flags=0, payload=None, stream=None,
                     iq_samples=None, out_syms=None):
        """lphy_hip_demod_ragged on device tensors; `desc` is a device tensor
        holding frames + 1 RAGGED_DESC_DTYPE records.  iq_samples / out_syms:
        the extents the descriptors span (checked against the tensors)."""
        dv = self.device
        p_iq = _dev_buf(iq, "iq", dv, (iq_samples or 0) * 8, None)
        p_desc = _dev_buf(desc, "desc", dv, (frames + 1) * 32, None)
        p_syms = _dev_buf(syms, "syms", dv, (out_syms or 0) * 2, 2)
        p_meta = _dev_buf(meta, "meta", dv, frames * 32, None)
        p_pay = None
        if flags & F_DECODE:
            p_pay = _dev_buf(payload, "payload", dv, ((out_syms or 0) + 1) // 2, 1)
        _chk(self.lib.lphy_hip_demod_ragged(self.ctx, p_iq, p_desc, frames, p_syms, p_pay, p_meta,
                                            mode, flags, stream), "lphy_hip_demod_ragged")

    def demod_ragged_host(self, iq_flat: np.ndarray, lengths_or_desc, mode: int, flags: int = 0,
                          fill: int = 0):
        """Demodulate frames of different lengths in one call.  `lengths_or_desc`
        is a list of sample counts (frames packed back to back in `iq_flat`) or
        a RAGGED_DESC_DTYPE array of frames + 1 records.  Returns (symbols,
        bytes, meta, desc): flat arrays over the descriptors' extent, frame f's
        symbols at desc["sym_offset"][f], its bytes at half of that.  Slots no
        frame owns keep `fill` (symbols: fill, bytes: fill & 0xff)."""
        a = np.asarray(lengths_or_desc)
        desc = np.ascontiguousarray(a) if a.dtype == RAGGED_DESC_DTYPE else self.ragged_layout(a, mode)
        frames = desc.size - 1
        iq = np.ascontiguousarray(iq_flat, np.complex64).reshape(-1)
        n_iq, n_out, _, _ = self._ragged_extents(desc, mode)
        if iq.size < n_iq:
            raise ValueError(f"iq: {iq.size} samples, the descriptors span {n_iq}")
        syms = np.full(max(n_out, 1), fill, np.uint16)
        payload = np.full(max((n_out + 1) // 2, 1), fill & 0xFF, np.uint8)
        meta = np.zeros(frames, META_DTYPE)
        pad = np.zeros(1, np.complex64)
        _chk(self.lib.lphy_hip_demod_ragged_host(self.ctx, (iq if iq.size else pad).ctypes.data,
                                                 desc.ctypes.data, frames, syms.ctypes.data,
                                                 payload.ctypes.data, meta.ctypes.data, mode, flags),
             "lphy_hip_demod_ragged_host")
        return syms, payload, meta, desc

    # --- the detector on a batch of windows (lphy_hip_detect_*) ----------
    def detect_batch(self, iq, total_samples, first, hop, step, windows, out, flags=0, stream=None):
        """LoRaDetector::detect on `windows` windows of device IQ: window w
        reads iq[first + w*hop + i*step], i < N ([x down-chirp with
        DET_DECHIRP] [x the context's Hann window]).  `out`: device tensor of
        windows DETECT_DTYPE records (16 bytes each).  Asynchronous."""
        dv = self.device
        p_iq = _dev_buf(iq, "iq", dv, total_samples * 8, None)
        p_out = _dev_buf(out, "out", dv, windows * 16, None)
        _chk(self.lib.lphy_hip_detect_batch(self.ctx, p_iq, total_samples, first, hop, step, windows,
                                            p_out, flags, stream), "lphy_hip_detect_batch")

    def detect_host(self, iq: np.ndarray, first, hop, step, windows, flags=0) -> np.ndarray:
        """The same on host samples; returns the DETECT_DTYPE record array."""
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
        out = np.zeros(windows, DETECT_DTYPE)
        pad = np.zeros(1, DETECT_DTYPE)
        _chk(self.lib.lphy_hip_detect_host(self.ctx, iq.ctypes.data, iq.size, first, hop, step, windows,
                                           (out if windows else pad).ctypes.data, flags), "lphy_hip_detect_host")
        return out

    def detect_ragged(self, iq, desc, frames, out, phase=0, flags=0, stream=None, iq_samples=None, units=None):
        """LoRaDetector::detect on every whole symbol of every frame of a
        ragged table in one launch: symbol s of frame f reads
        iq[desc[f]["iq_offset"] + s*N*osr + phase + i*osr], i < N, prepared as
        detect_batch prepares a window, and its record goes to
        out[desc[f]["unit_offset"] + s] (lphy_hip_detect_ragged).  `desc`:
        device tensor of frames + 1 RAGGED_DESC_DTYPE records; `out`: device
        tensor of desc[frames]["unit_offset"] DETECT_DTYPE records.
        iq_samples / units: the extents the descriptors span (checked against
        the tensors).  Asynchronous."""
        dv = self.device
        p_iq = _dev_buf(iq, "iq", dv, (iq_samples or 0) * 8, None)
        p_desc = _dev_buf(desc, "desc", dv, (frames + 1) * 32, None)
        p_out = _dev_buf(out, "out", dv, (units or 0) * 16, None)
        _chk(self.lib.lphy_hip_detect_ragged(self.ctx, p_iq, p_desc, frames, phase, p_out, flags, stream),
             "lphy_hip_detect_ragged")

    def detect_ragged_host(self, iq_flat: np.ndarray, lengths_or_desc, phase: int = 0, flags: int = 0):
        """The same on host samples.  `lengths_or_desc` is a list of sample
        counts (frames packed back to back in `iq_flat`) or a
        RAGGED_DESC_DTYPE array of frames + 1 records (iq_offset, samples and
        unit_offset are read).  Returns (records, desc): one DETECT_DTYPE
        record per whole symbol, frame f's first at desc["unit_offset"][f]."""
        a = np.asarray(lengths_or_desc)
        desc = (np.ascontiguousarray(a) if a.dtype == RAGGED_DESC_DTYPE
                else self.ragged_layout(a, MODE_DEMODULATE))
        frames = desc.size - 1
        iq = np.ascontiguousarray(iq_flat, np.complex64).reshape(-1)
        n_iq, _, units, _ = self._ragged_extents(desc, MODE_DEMODULATE)
        if iq.size < n_iq:
            raise ValueError(f"iq: {iq.size} samples, the descriptors span {n_iq}")
        out = np.zeros(units, DETECT_DTYPE)
        pad = np.zeros(1, np.complex64)
        opad = np.zeros(1, DETECT_DTYPE)
        _chk(self.lib.lphy_hip_detect_ragged_host(self.ctx, (iq if iq.size else pad).ctypes.data,
                                                  desc.ctypes.data, frames, phase,
                                                  (out if units else opad).ctypes.data, flags),
             "lphy_hip_detect_ragged_host")
        return out, desc

    # --- the frame search (lphy_hip_find_frames*) ------------------------
    def find_frames_workspace(self, windows: int) -> int:
        """Bytes of device workspace find_frames needs for `windows` records."""
        return int(self.lib.lphy_hip_find_frames_workspace(windows))

    def find_frames(self, rec, windows, params, mode, max_frames, desc, info, work, stream=None):
        """The ragged table of the frames found in a capture, from the detector
        records of its windows (lphy_hip_find_frames).  `rec`: device tensor of
        `windows` DETECT_DTYPE records (detect_batch's output; may be None for
        windows == 0); `params`: one FIND_PARAMS record (find_params());
        `desc`: device tensor of max_frames + 1 RAGGED_DESC_DTYPE records, all
        written, valid for every ragged call with frames = max_frames; `info`:
        device tensor of one FIND_INFO record; `work`: device tensor of
        find_frames_workspace(windows) bytes.  Asynchronous."""
        dv = self.device
        prm = np.ascontiguousarray(params, FIND_PARAMS).reshape(-1)
        if prm.size != 1:
            raise ValueError(f"params: one FIND_PARAMS record expected, got {prm.size}")
        p_rec = _dev_buf(rec, "rec", dv, windows * 16, None) if (windows or rec is not None) else None
        p_desc = _dev_buf(desc, "desc", dv, (max_frames + 1) * 32, None)
        p_info = _dev_buf(info, "info", dv, 32, None)
        p_work = _dev_buf(work, "work", dv, self.find_frames_workspace(windows), None)
        _chk(self.lib.lphy_hip_find_frames(self.ctx, p_rec, windows, prm.ctypes.data, mode, max_frames, p_desc,
                                           p_info, p_work, stream), "lphy_hip_find_frames")

    def find_frames_host(self, rec: np.ndarray, params, mode: int, max_frames: int):
        """The same on host records; returns (desc, info): max_frames + 1
        RAGGED_DESC_DTYPE records and the FIND_INFO record."""
        r = np.ascontiguousarray(rec, DETECT_DTYPE).reshape(-1)
        prm = np.ascontiguousarray(params, FIND_PARAMS).reshape(-1)
        if prm.size != 1:
            raise ValueError(f"params: one FIND_PARAMS record expected, got {prm.size}")
        desc = np.zeros(max(max_frames, 0) + 1, RAGGED_DESC_DTYPE)
        info = np.zeros(1, FIND_INFO)
        _chk(self.lib.lphy_hip_find_frames_host(self.ctx, r.ctypes.data if r.size else None, r.size,
                                                prm.ctypes.data, mode, max_frames, desc.ctypes.data,
                                                info.ctypes.data), "lphy_hip_find_frames_host")
        return desc, info[0]

    # --- the channeliser (lphy_hip_channelize*) --------------------------
    def channelize(self, iq, plan, taps, rot, out, stream=None):
        """`channels` mixed, filtered and decimated streams from one wideband
        capture (lphy_hip_channelize): out[c*out_stride + m] = rot[c, (rot_first
        + m) % R] * sum_k iq[first + m*decim + k] * taps[c, k], every operation
        a float32 one in the header's order.  `plan`: one CHAN_PLAN record
        (chan_plan()); `iq`: device tensor of in_samples complex samples;
        `taps`, `rot`: device tensors of channels x taps and channels x
        rot_period complex samples (chan_design()); `out`: device tensor of
        channels x out_stride complex samples, of which the call writes the
        first `outputs` of every channel.  Asynchronous."""
        dv = self.device
        p, q = _one_plan(plan, CHAN_PLAN, "CHAN_PLAN")
        p_in = _dev_buf(iq, "iq", dv, int(q["in_samples"]) * 8, None)
        p_taps, p_rot = _tables_bufs(taps, rot, dv, q)
        p_out = _dev_buf(out, "out", dv, int(q["channels"]) * int(q["out_stride"]) * 8, None)
        _chk(self.lib.lphy_hip_channelize(self.ctx, p_in, p.ctypes.data, p_taps, p_rot, p_out, stream),
             "lphy_hip_channelize")

    def channelize_host(self, iq: np.ndarray, taps: np.ndarray, rot: np.ndarray, decim: int, first: int = 0,
                        outputs: int | None = None, rot_first: int = 0, out: np.ndarray | None = None) -> np.ndarray:
        """The same on host arrays: `taps` [channels, T] and `rot` [channels, R]
        complex64; `outputs` defaults to all the capture holds from `first`
        (channelize_outputs).  `out`, when given, is a C-contiguous complex64
        [channels, out_stride] array whose columns past `outputs` the call
        leaves alone.  Returns the (channels, outputs) complex64 result (a view
        of `out` when given)."""
        x = np.ascontiguousarray(iq, np.complex64).reshape(-1)
        return self._channelize_host(x, x.size, None, taps, rot, decim, first, outputs, rot_first, out)

    def _channelize_host(self, x, n, fmt, taps, rot, decim, first, outputs, rot_first, out):
        """channelize_host and channelize_raw_host behind their own check of the
        capture: `x` flat and contiguous, `n` its samples, `fmt` None for the
        float32 entry point."""
        t = np.ascontiguousarray(taps, np.complex64)
        r = np.ascontiguousarray(rot, np.complex64)
        if t.ndim != 2 or r.ndim != 2 or t.shape[0] != r.shape[0]:
            raise ValueError(f"taps {t.shape} and rot {r.shape}: [channels, T] and [channels, R] expected")
        if outputs is None:
            outputs = channelize_outputs(n, first, t.shape[1], decim)
        if out is None:
            out = np.zeros((t.shape[0], outputs), np.complex64)
        if (out.dtype != np.complex64 or out.ndim != 2 or not out.flags.c_contiguous or out.shape[0] != t.shape[0]
                or out.shape[1] < outputs):
            raise ValueError(f"out: C-contiguous complex64 [{t.shape[0]}, >= {outputs}] expected")
        p = chan_plan(first, n, outputs, out.shape[1], rot_first, t.shape[0], t.shape[1], decim, r.shape[1])
        p_x, p_t, p_r, p_out = _host_ptrs(x, t, r, out)
        if fmt is None:
            _chk(self.lib.lphy_hip_channelize_host(self.ctx, p_x, p.ctypes.data, p_t, p_r, p_out),
                 "lphy_hip_channelize_host")
        else:
            _chk(self.lib.lphy_hip_channelize_raw_host(self.ctx, p_x, fmt, p.ctypes.data, p_t, p_r, p_out),
                 "lphy_hip_channelize_raw_host")
        return out[:, :outputs]

    def channelize_raw(self, iq, fmt, plan, taps, rot, out, stream=None):
        """channelize() on a capture as the radio wrote it
        (lphy_hip_channelize_raw): `iq` is a device tensor of 2 * in_samples
        elements of fmt's type - float32 (FMT_CF32), int16 (FMT_SC16), int8
        (FMT_SC8) or uint8 (FMT_CU8, value = byte - 127.5) - interleaved I, Q.
        The result is channelize()'s on the capture converted to float32, which
        is exact; there is no scale: fold 1/32768 (1/128) into `taps`.
        Everything else as channelize().  Asynchronous."""
        dv = self.device
        dt = _fmt_dtype(fmt)
        p, q = _one_plan(plan, CHAN_PLAN, "CHAN_PLAN")
        p_in = _dev_buf(iq, "iq", dv, 0, None)
        want = "torch." + dt.name  # torch's dtypes print as numpy names them
        if str(iq.dtype) != want or iq.numel() != 2 * int(q["in_samples"]):
            raise ValueError(f"iq: {2 * int(q['in_samples'])} elements of {want} expected, got {iq.numel()} of "
                             f"{iq.dtype}")
        p_taps, p_rot = _tables_bufs(taps, rot, dv, q)
        p_out = _dev_buf(out, "out", dv, int(q["channels"]) * int(q["out_stride"]) * 8, None)
        _chk(self.lib.lphy_hip_channelize_raw(self.ctx, p_in, fmt, p.ctypes.data, p_taps, p_rot, p_out, stream),
             "lphy_hip_channelize_raw")

    def channelize_raw_host(self, x: np.ndarray, fmt: int, taps: np.ndarray, rot: np.ndarray, decim: int,
                            first: int = 0, outputs: int | None = None, rot_first: int = 0,
                            out: np.ndarray | None = None) -> np.ndarray:
        """channelize_host() on a capture as the radio wrote it
        (lphy_hip_channelize_raw_host): `x` is a numpy array of fmt's dtype,
        shaped [n, 2] (I, Q) or flat with 2n elements; the samples go to the
        device at sample_bytes(fmt) each.  Everything else as
        channelize_host()."""
        dt = _fmt_dtype(fmt)
        x = np.asarray(x)
        if x.dtype != dt or not (x.ndim == 1 and x.size % 2 == 0 or x.ndim == 2 and x.shape[1] == 2):
            raise ValueError(f"x: {dt.name} [n, 2] or flat with 2n elements expected, got {x.dtype} {x.shape}")
        x = np.ascontiguousarray(x).reshape(-1)
        return self._channelize_host(x, x.size // 2, fmt, taps, rot, decim, first, outputs, rot_first, out)

    # --- the synthesiser (lphy_hip_synthesize*) --------------------------
    def synthesize(self, streams, plan, taps, rot, out, stream=None):
        """One wideband stream from `channels` narrow ones
        (lphy_hip_synthesize): out[n] = sum_c sum_i rot[c, (rot_first + j) % R]
        * streams[c*in_stride + j] * taps[c, i*interp + p] with first + n = q *
        interp + p and j = q - i, every operation a float32 one in the header's
        order.  `plan`: one SYNTH_PLAN record (synth_plan()); `streams`: device
        tensor of channels x in_stride complex samples (the last channel may
        stop at in_samples), or None when in_samples is 0; `taps`, `rot`:
        device tensors of channels x taps and channels x rot_period complex
        samples (synth_design()); `out`: device tensor of `outputs` complex
        samples.  Asynchronous."""
        dv = self.device
        p, q = _one_plan(plan, SYNTH_PLAN, "SYNTH_PLAN")
        ch, n_in = int(q["channels"]), int(q["in_samples"])
        p_in = None
        if streams is not None or n_in:
            p_in = _dev_buf(streams, "streams", dv, ((max(ch, 1) - 1) * int(q["in_stride"]) + n_in) * 8 if n_in else 0,
                            None)
        p_taps, p_rot = _tables_bufs(taps, rot, dv, q)
        p_out = _dev_buf(out, "out", dv, int(q["outputs"]) * 8, None)
        _chk(self.lib.lphy_hip_synthesize(self.ctx, p_in, p.ctypes.data, p_taps, p_rot, p_out, stream),
             "lphy_hip_synthesize")

    def synthesize_host(self, streams: np.ndarray, taps: np.ndarray, rot: np.ndarray, interp: int, first: int = 0,
                        rot_first: int = 0, outputs: int | None = None) -> np.ndarray:
        """The same on host arrays: `streams` [channels, in_samples], `taps`
        [channels, T] and `rot` [channels, R] complex64; `outputs` defaults to
        all that an input sample reaches from `first` (synthesize_outputs).
        Returns the `outputs` complex64 wideband samples."""
        x = np.ascontiguousarray(streams, np.complex64)
        t = np.ascontiguousarray(taps, np.complex64)
        r = np.ascontiguousarray(rot, np.complex64)
        if x.ndim != 2 or t.ndim != 2 or r.ndim != 2 or not (x.shape[0] == t.shape[0] == r.shape[0]):
            raise ValueError(f"streams {x.shape}, taps {t.shape} and rot {r.shape}: [channels, in_samples], "
                             "[channels, T] and [channels, R] expected")
        if outputs is None:
            outputs = synthesize_outputs(x.shape[1], first, t.shape[1], interp)
        out = np.zeros(outputs, np.complex64)
        p = synth_plan(first, x.shape[1], x.shape[1], outputs, rot_first, t.shape[0], t.shape[1], interp, r.shape[1])
        p_x, p_t, p_r, p_out = _host_ptrs(x, t, r, out)
        _chk(self.lib.lphy_hip_synthesize_host(self.ctx, p_x, p.ctypes.data, p_t, p_r, p_out),
             "lphy_hip_synthesize_host")
        return out

    def detect_serial_count(self, reset: bool = True) -> int:
        """Windows whose power_avg took the in-order walk of the bins because
        the parallel sum could not certify it (device sync)."""
        n = C.c_ulonglong(0)
        _chk(self.lib.lphy_hip_detect_serial_count(self.ctx, C.byref(n), int(reset)),
             "lphy_hip_detect_serial_count")
        return int(n.value)

    def modulate_batch(self, syms, frames, nsyms, iq, amplitude=1.0, sync=0x12, stream=None):
        dv = self.device
        p_syms = _dev_buf(syms, "syms", dv, frames * nsyms * 2, 2) if nsyms else None
        p_iq = _dev_buf(iq, "iq", dv, frames * (nsyms + 2) * self.N * self.osr * 8, None)
        _chk(self.lib.lphy_hip_modulate_batch(self.ctx, p_syms, frames, nsyms, p_iq,
                                              amplitude, sync, stream),
             "lphy_hip_modulate_batch")

    # --- ragged transmit: frames of different lengths in one call --------
    def tx_layout(self, len_bytes) -> np.ndarray:
        """Descriptors (RAGGED_DESC_DTYPE, len(len_bytes) + 1 records) of frames
        carrying `len_bytes` payload bytes each, (2 len + 2) symbols packed
        back to back (lphy_hip_tx_layout): frame f's bytes start at
        desc["sym_offset"][f] // 2.  The same table demodulates the IQ."""
        n = np.ascontiguousarray(len_bytes, np.uint64).reshape(-1)
        desc = np.zeros(n.size + 1, RAGGED_DESC_DTYPE)
        _chk(self.lib.lphy_hip_tx_layout(self.ctx, n.ctypes.data if n.size else None, n.size, desc.ctypes.data),
             "lphy_hip_tx_layout")
        return desc

    def modulate_ragged(self, syms, desc, frames, iq, amplitude=1.0, sync=0x12, stream=None,
                        iq_samples=None, out_syms=None):
        """lphy_hip_modulate_ragged on device tensors: frame f's symbols at
        syms[desc[f]["sym_offset"]:], its IQ at iq[2 * desc[f]["iq_offset"]:]
        floats.  `desc`: device tensor of frames + 1 RAGGED_DESC_DTYPE records.
        iq_samples / out_syms: the extents the descriptors span (checked
        against the tensors).  Asynchronous."""
        dv = self.device
        p_syms = _dev_buf(syms, "syms", dv, (out_syms or 0) * 2, 2)
        p_desc = _dev_buf(desc, "desc", dv, (frames + 1) * 32, None)
        p_iq = _dev_buf(iq, "iq", dv, (iq_samples or 0) * 8, None)
        _chk(self.lib.lphy_hip_modulate_ragged(self.ctx, p_syms, p_desc, frames, p_iq, amplitude, sync, stream),
             "lphy_hip_modulate_ragged")

    def tx_ragged(self, data, desc, frames, iq, syms_out=None, amplitude=1.0, sync=0x12, stream=None,
                  iq_samples=None, out_syms=None):
        """lphy_hip_tx_ragged on device tensors: lora_encode + lora_modulate of
        frame f's bytes at data[desc[f]["sym_offset"] // 2:].  syms_out
        (optional) receives the encoded symbols at sym_offset.  Asynchronous."""
        dv = self.device
        p_data = _dev_buf(data, "data", dv, ((out_syms or 0) + 1) // 2, 1)
        p_desc = _dev_buf(desc, "desc", dv, (frames + 1) * 32, None)
        p_iq = _dev_buf(iq, "iq", dv, (iq_samples or 0) * 8, None)
        p_out = _dev_buf(syms_out, "syms_out", dv, (out_syms or 0) * 2, 2) if syms_out is not None else None
        _chk(self.lib.lphy_hip_tx_ragged(self.ctx, p_data, p_desc, frames, p_iq, p_out, amplitude, sync, stream),
             "lphy_hip_tx_ragged")

    def tx_ragged_host(self, payloads_or_data, desc=None, amplitude=1.0, sync=0x12, iq=None, syms_out=None,
                       want_syms=True):
        """Encode and modulate frames of different lengths in one call.  Either a
        list of payloads (bytes / uint8 arrays; the table comes from tx_layout)
        or a flat uint8 array with a RAGGED_DESC_DTYPE table of frames + 1
        records.  iq / syms_out: the caller's buffers over the descriptors'
        extent (what no frame owns keeps its values); made here when None.
        Returns (iq complex64, symbols uint16 or None, desc)."""
        if desc is None:
            pl = [np.frombuffer(bytes(p), np.uint8) for p in payloads_or_data]
            desc = self.tx_layout([p.size for p in pl])
            data = np.concatenate(pl) if pl else np.zeros(0, np.uint8)
        else:
            desc = np.ascontiguousarray(desc, RAGGED_DESC_DTYPE)
            data = np.ascontiguousarray(payloads_or_data, np.uint8).reshape(-1)
        frames = desc.size - 1
        n_iq, n_out, _, need = self._ragged_extents(desc, MODE_LORA_DEMODULATE)
        if data.size < need:
            raise ValueError(f"data: {data.size} bytes, the descriptors read {need}")
        if iq is None:
            iq = np.zeros(max(n_iq, 1), np.complex64)
        if iq.dtype != np.complex64 or not iq.flags.c_contiguous or iq.size < n_iq:
            raise ValueError(f"iq: contiguous complex64 of at least {n_iq} samples expected")
        if syms_out is None and want_syms:
            syms_out = np.zeros(max(n_out, 1), np.uint16)
        if syms_out is not None and (syms_out.dtype != np.uint16 or not syms_out.flags.c_contiguous
                                     or syms_out.size < n_out):
            raise ValueError(f"syms_out: contiguous uint16 of at least {n_out} symbols expected")
        pad = np.zeros(1, np.uint8)
        _chk(self.lib.lphy_hip_tx_ragged_host(self.ctx, (data if data.size else pad).ctypes.data, desc.ctypes.data,
                                              frames, iq.ctypes.data,
                                              syms_out.ctypes.data if syms_out is not None else None,
                                              amplitude, sync), "lphy_hip_tx_ragged_host")
        return iq, syms_out, desc

    def decode_batch(self, syms, frames, syms_per_frame, payload, meta, stream=None):
        dv = self.device
        p_syms = _dev_buf(syms, "syms", dv, frames * syms_per_frame * 2, 2)
        p_pay = _dev_buf(payload, "payload", dv, frames * (syms_per_frame // 2), 1)
        p_meta = _dev_buf(meta, "meta", dv, frames * 32, None)
        _chk(self.lib.lphy_hip_decode_batch(self.ctx, p_syms, frames, syms_per_frame,
                                            p_pay, p_meta, stream),
             "lphy_hip_decode_batch")

    def estimate_batch(self, iq, frames, frame_samples, est_samples, meta, stream=None):
        """estimate_offsets over the first `est_samples` samples of each of
        `frames` device frames; rewrites the frames' 32-byte `meta` records
        (lphy_hip_estimate_batch).  Asynchronous."""
        dv = self.device
        p_iq = _dev_buf(iq, "iq", dv, frames * frame_samples * 8, None)
        p_meta = _dev_buf(meta, "meta", dv, frames * 32, None)
        _chk(self.lib.lphy_hip_estimate_batch(self.ctx, p_iq, frames, frame_samples, est_samples,
                                              p_meta, stream),
             "lphy_hip_estimate_batch")

    def estimate_ragged(self, iq, desc, frames, est_samples, meta, stream=None, iq_samples=None):
        """The same for frames of different lengths in one launch: frame f is
        desc[f]["samples"] samples at desc[f]["iq_offset"], its estimate runs
        over the whole symbols of its first min(samples, est_samples) samples
        (est_samples = 0: the whole frame) and rewrites meta[f]; a frame
        without a whole symbol there keeps its record
        (lphy_hip_estimate_ragged).  `desc`: device tensor of
        RAGGED_DESC_DTYPE records; record [frames] is not read.  iq_samples:
        the extent the descriptors span (checked against the tensor).
        Asynchronous."""
        dv = self.device
        p_iq = _dev_buf(iq, "iq", dv, (iq_samples or 0) * 8, None)
        p_desc = _dev_buf(desc, "desc", dv, frames * 32, None)
        p_meta = _dev_buf(meta, "meta", dv, frames * 32, None)
        _chk(self.lib.lphy_hip_estimate_ragged(self.ctx, p_iq, p_desc, frames, est_samples, p_meta, stream),
             "lphy_hip_estimate_ragged")

    def compensate_batch(self, iq_in, iq_out, frames, frame_samples, meta, stream=None):
        """compensate_offsets on each of `frames` device frames with the frame's
        own meta[f].cfo / .time_offset, read on the device
        (lphy_hip_compensate_batch).  iq_out may be iq_in (in place) or a
        disjoint tensor; `meta` is not written.  Asynchronous."""
        dv = self.device
        p_in = _dev_buf(iq_in, "iq_in", dv, frames * frame_samples * 8, None)
        p_out = _dev_buf(iq_out, "iq_out", dv, frames * frame_samples * 8, None)
        p_meta = _dev_buf(meta, "meta", dv, frames * 32, None)
        _chk(self.lib.lphy_hip_compensate_batch(self.ctx, p_in, p_out, frames, frame_samples, p_meta,
                                                stream), "lphy_hip_compensate_batch")

    def compensate_ragged(self, iq_in, iq_out, desc, frames, meta, stream=None, iq_samples=None):
        """The same for frames of different lengths: frame f is
        desc[f]["samples"] samples at desc[f]["iq_offset"] in iq_in and iq_out
        alike (`desc`: device tensor of RAGGED_DESC_DTYPE records; record
        [frames] is not read).  iq_samples: the extent the descriptors span
        (checked against the tensors)."""
        dv = self.device
        p_in = _dev_buf(iq_in, "iq_in", dv, (iq_samples or 0) * 8, None)
        p_out = _dev_buf(iq_out, "iq_out", dv, (iq_samples or 0) * 8, None)
        p_desc = _dev_buf(desc, "desc", dv, frames * 32, None)
        p_meta = _dev_buf(meta, "meta", dv, frames * 32, None)
        _chk(self.lib.lphy_hip_compensate_ragged(self.ctx, p_in, p_out, p_desc, frames, p_meta, stream),
             "lphy_hip_compensate_ragged")

    # --- streaming ingestion (lphy_hip_demod_stream) --------------------
    def demod_stream(self, fd: int, frame_samples: int, mode: int, flags: int = 0,
                     chunk_frames: int = 0, max_frames: int = 0, capacity: int = 0):
        """Demodulate the float32 I/Q frames read from `fd` until EOF or
        max_frames.  The result arrays hold `capacity` frames (default:
        max_frames); at most min(max_frames, capacity) frames are read.
        chunk_frames = 0 lets the library pick ~64 MiB chunks (its pinned slots
        are kept with the context for the next call).  Returns (symbols,
        payload, meta, tail_bytes) for the whole frames read."""
        cap = capacity or max_frames
        if cap <= 0:
            raise ValueError("capacity or max_frames required")
        max_frames = min(max_frames, cap) if max_frames else cap
        per = self.syms_per_frame(frame_samples, mode)
        syms = np.zeros(max(cap * per, 1), np.uint16)
        payload = np.zeros(max(cap * (per // 2), 1), np.uint8)
        meta = np.zeros(cap, META_DTYPE)
        nout, tail = _sz(0), _sz(0)
        _chk(self.lib.lphy_hip_demod_stream(self.ctx, fd, frame_samples, chunk_frames, mode, flags,
                                            max_frames, syms.ctypes.data, payload.ctypes.data,
                                            meta.ctypes.data, C.byref(nout), C.byref(tail)),
             "lphy_hip_demod_stream")
        n = nout.value
        return (syms[: n * per].reshape(n, per), payload[: n * (per // 2)].reshape(n, per // 2),
                meta[:n], tail.value)

    # --- host convenience ----------------------------------------------
    def demod_host(self, iq: np.ndarray, frames: int, frame_samples: int, mode: int,
                   flags: int = 0):
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
        assert iq.size == frames * frame_samples
        per = self.syms_per_frame(frame_samples, mode)
        syms = np.zeros(max(frames * per, 1), np.uint16)
        payload = np.zeros(max(frames * (per // 2), 1), np.uint8)
        meta = np.zeros(frames, META_DTYPE)
        _chk(self.lib.lphy_hip_demod_host(self.ctx, iq.ctypes.data, frames, frame_samples,
                                          syms.ctypes.data, payload.ctypes.data,
                                          meta.ctypes.data, mode, flags),
             "lphy_hip_demod_host")
        return (syms[: frames * per].reshape(frames, per),
                payload[: frames * (per // 2)].reshape(frames, per // 2), meta)

    def decode_host(self, syms: np.ndarray):
        syms = np.ascontiguousarray(syms, np.uint16)
        out = np.zeros(max(len(syms) // 2, 1), np.uint8)
        meta = np.zeros(1, META_DTYPE)
        rc = self.lib.lphy_hip_decode_host(self.ctx, syms.ctypes.data, len(syms),
                                           out.ctypes.data, meta.ctypes.data)
        return rc, out[: len(syms) // 2], meta[0]

    def estimate_host(self, iq: np.ndarray):
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
        meta = np.zeros(1, META_DTYPE)
        _chk(self.lib.lphy_hip_estimate_host(self.ctx, iq.ctypes.data, iq.size,
                                             meta.ctypes.data), "lphy_hip_estimate_host")
        return meta[0]

    def estimate_ragged_host(self, iq_flat: np.ndarray, lengths_or_desc, est_samples: int = 0, meta=None):
        """estimate_offsets for frames of different lengths in one call.
        `lengths_or_desc` is a list of sample counts (frames packed back to
        back in `iq_flat`) or a RAGGED_DESC_DTYPE array of frames + 1 records
        (only iq_offset and samples of the first `frames` are read).  `meta`:
        the caller's `frames` META_DTYPE records, which go in and come back (a
        frame without a whole symbol in its estimate extent keeps its record);
        zeros when None.  Returns (meta, desc)."""
        a = np.asarray(lengths_or_desc)
        desc = (np.ascontiguousarray(a) if a.dtype == RAGGED_DESC_DTYPE
                else self.ragged_layout(a, MODE_DEMODULATE))
        frames = desc.size - 1
        iq = np.ascontiguousarray(iq_flat, np.complex64).reshape(-1)
        n_iq = self._ragged_extents(desc, MODE_DEMODULATE)[0]
        if iq.size < n_iq:
            raise ValueError(f"iq: {iq.size} samples, the descriptors span {n_iq}")
        m = (np.zeros(frames, META_DTYPE) if meta is None
             else np.array(meta, META_DTYPE, copy=True).reshape(-1))
        if m.size != frames:
            raise ValueError(f"meta: {m.size} records for {frames} frames")
        pad = np.zeros(1, np.complex64)
        mpad = np.zeros(1, META_DTYPE)
        _chk(self.lib.lphy_hip_estimate_ragged_host(self.ctx, (iq if iq.size else pad).ctypes.data,
                                                    desc.ctypes.data, frames, est_samples,
                                                    (m if m.size else mpad).ctypes.data),
             "lphy_hip_estimate_ragged_host")
        return m, desc

    def compensate_host(self, iq: np.ndarray, cfo: float, time_offset: float):
        x = np.array(iq, np.complex64, copy=True).reshape(-1)
        _chk(self.lib.lphy_hip_compensate_host(self.ctx, x.ctypes.data, x.size, cfo,
                                               time_offset), "lphy_hip_compensate_host")
        return x

    def compensate_batch_host(self, iq: np.ndarray, frames: int, frame_samples: int, meta: np.ndarray):
        """compensate_batch on host samples; `meta`: `frames` META_DTYPE
        records (cfo and time_offset are read).  Returns the corrected copy."""
        x = np.array(iq, np.complex64, copy=True).reshape(-1)
        m = np.ascontiguousarray(meta, META_DTYPE).reshape(-1)
        if x.size != frames * frame_samples or m.size != frames:
            raise ValueError(f"iq: {x.size} samples, meta: {m.size} records for {frames} x {frame_samples}")
        pad = np.zeros(1, np.complex64)
        _chk(self.lib.lphy_hip_compensate_batch_host(self.ctx, (x if x.size else pad).ctypes.data, frames,
                                                     frame_samples, m.ctypes.data if m.size else None),
             "lphy_hip_compensate_batch_host")
        return x

    def modulate_host(self, syms: np.ndarray, amplitude=1.0, sync=0x12):
        syms = np.ascontiguousarray(syms, np.uint16)
        out = np.zeros((len(syms) + 2) * self.N * self.osr, np.complex64)
        _chk(self.lib.lphy_hip_modulate_host(self.ctx, syms.ctypes.data, len(syms),
                                             out.ctypes.data, amplitude, sync),
             "lphy_hip_modulate_host")
        return out

    def bounds_violations(self, reset: bool = True) -> int:
        """Device index checks that failed since the last reset (test build
        only: the product library returns -ENOTSUP).  Synchronises."""
        n = C.c_ulonglong(0)
        _chk(self.lib.lphy_hip_bounds_violations(self.ctx, C.byref(n), int(reset)),
             "lphy_hip_bounds_violations")
        return int(n.value)

    def reserve(self, frames: int, frame_samples: int) -> None:
        _chk(self.lib.lphy_hip_ctx_reserve(self.ctx, frames, frame_samples), "lphy_hip_ctx_reserve")

    def parseval_count(self, reset: bool = True) -> int:
        """Test build only: symbols the wave kernel (k_wave, SF 7-12) certified by
        the Parseval certificate, without their FFT (device sync)."""
        fn = self.lib.lphy_hip_test_counter
        fn.argtypes = [_vp, C.c_int, C.POINTER(C.c_ulonglong), C.c_int]
        n = C.c_ulonglong(0)
        _chk(fn(self.ctx, 1, C.byref(n), int(reset)), "lphy_hip_test_counter")  # kCtrParseval
        return int(n.value)

    def mod_serial_count(self, reset: bool = True) -> int:
        """Test build only: frames the one-launch modulator (k_mod_fast) gave
        to its serial walk because the candidate chain left its windows
        (device sync)."""
        fn = self.lib.lphy_hip_test_counter
        fn.argtypes = [_vp, C.c_int, C.POINTER(C.c_ulonglong), C.c_int]
        n = C.c_ulonglong(0)
        _chk(fn(self.ctx, 2, C.byref(n), int(reset)), "lphy_hip_test_counter")  # kCtrModSerial
        return int(n.value)

    def mod_force_serial(self, on: bool) -> None:
        """Test build only: k_mod_fast takes its serial walk for every frame."""
        fn = self.lib.lphy_hip_test_mod_force_serial
        fn.argtypes = [_vp, C.c_int]
        _chk(fn(self.ctx, int(bool(on))), "lphy_hip_test_mod_force_serial")

    def pinned_max(self, nbytes: int) -> None:
        """Test build only: the largest *_host call that goes through the
        pinned mirror (0: every call takes the pageable copies)."""
        fn = self.lib.lphy_hip_test_pinned_max
        fn.argtypes = [_vp, _sz]
        _chk(fn(self.ctx, int(nbytes)), "lphy_hip_test_pinned_max")

    def grid_cap(self, blocks: int) -> None:
        """Test build only: at most `blocks` workgroups in the persistent grids
        of the ragged symbol kernel, the detector, the ragged transmit's
        sample pass and the frame search on this context (0: the default), so that a small call
        walks their grid-stride loops more than once."""
        fn = self.lib.lphy_hip_test_grid_cap
        fn.argtypes = [_vp, C.c_uint]
        _chk(fn(self.ctx, int(blocks)), "lphy_hip_test_grid_cap")

    def libm_probe(self, op: int, a, b=None, stream=None):
        """Test build only: csrc/libm_exact.h, the device sqrtf and
        detector_power as compiled for the device, on float32 device tensors
        (op: LIBM_*; b: the second argument of LIBM_ATAN2 / LIBM_CABS /
        LIBM_DETECTOR_POWER) -> (out0, out1) device tensors, out1 (the
        cosine) None for the ops with one result.  Asynchronous."""
        import torch
        fn = self.lib.lphy_hip_test_libm
        fn.argtypes = [_vp, C.c_int, _vp, _vp, _vp, _vp, _sz, _vp]
        n, dv = a.numel(), self.device
        p_a = _dev_buf(a, "a", dv, n * 4, 4)
        p_b = None if b is None else _dev_buf(b, "b", dv, n * 4, 4)
        out0 = torch.empty_like(a)
        out1 = torch.empty_like(a) if op in (LIBM_SINCOS_EXACT, LIBM_SINCOS_SPLIT, LIBM_SINCOS_LARGE) else None
        _chk(fn(self.ctx, int(op), p_a, p_b, out0.data_ptr(), None if out1 is None else out1.data_ptr(), n, stream),
             "lphy_hip_test_libm")
        return out0, out1

    def recheck_count(self, reset: bool = True) -> int:
        """Symbols the fused kernel re-ran with the exact rotation (device sync)."""
        n = C.c_ulonglong(0)
        _chk(self.lib.lphy_hip_recheck_count(self.ctx, C.byref(n), int(reset)),
             "lphy_hip_recheck_count")
        return int(n.value)


def hamming84_encode_table() -> np.ndarray:
    """encodeHamming84sx (LoRaCodes.hpp:229-242) for nibbles 0..15 (producer)."""
    t = np.zeros(16, np.uint16)
    for x in range(16):
        d = [(x >> i) & 1 for i in range(4)]
        t[x] = (x | (d[0] ^ d[1] ^ d[2]) << 4 | (d[1] ^ d[2] ^ d[3]) << 5
                | (d[0] ^ d[1] ^ d[3]) << 6 | (d[0] ^ d[2] ^ d[3]) << 7)
    return t


def encode_payloads(payloads: np.ndarray) -> np.ndarray:
    """lora_encode for a [frames, bytes] uint8 array -> [frames, 2*bytes] uint16."""
    t = hamming84_encode_table()
    p = np.asarray(payloads, np.uint8)
    out = np.empty(p.shape[:-1] + (2 * p.shape[-1],), np.uint16)
    out[..., 0::2] = t[p >> 4]
    out[..., 1::2] = t[p & 0x0F]
    return out


# --- LoRaCodes.hpp batch kernels (device tensors) -------
def _dptr(t, name, nbytes, itemsize=None):
    return _dev_buf(t, name, t.device.index or 0, nbytes, itemsize)


def gray_batch(syms, to_binary: bool, stream=None):
    """binaryToGray16 / grayToBinary16 in place on a uint16 (int16) tensor."""
    n = syms.numel()
    _chk(load().lphy_hip_gray_batch(_dptr(syms, "syms", n * 2, 2), n, int(to_binary), stream),
         "lphy_hip_gray_batch")


def interleave_batch(cw, frames, cw_stride, cw_per_frame, syms, sym_stride, ppm, rdd, stream=None):
    _chk(load().lphy_hip_interleave_batch(_dptr(cw, "cw", frames * cw_stride, 1), frames, cw_stride,
                                          cw_per_frame, _dptr(syms, "syms", frames * sym_stride * 2, 2),
                                          sym_stride, ppm, rdd, stream), "lphy_hip_interleave_batch")


def deinterleave_batch(syms, frames, sym_stride, syms_per_frame, cw, cw_stride, ppm, rdd, stream=None):
    _chk(load().lphy_hip_deinterleave_batch(_dptr(syms, "syms", frames * sym_stride * 2, 2), frames,
                                            sym_stride, syms_per_frame, _dptr(cw, "cw", frames * cw_stride, 1),
                                            cw_stride, ppm, rdd, stream), "lphy_hip_deinterleave_batch")


def whiten_batch(buf, frames, stride, length, kind, bit_ofs=0, rdd=4, stream=None):
    _chk(load().lphy_hip_whiten_batch(_dptr(buf, "buf", frames * stride, 1), frames, stride, length, kind,
                                      bit_ofs, rdd, stream), "lphy_hip_whiten_batch")


def hamming_batch(buf, op, flags=None, stream=None):
    n = buf.numel()
    pf = _dptr(flags, "flags", n, 1) if flags is not None else None
    _chk(load().lphy_hip_hamming_batch(_dptr(buf, "buf", n, 1), n, op, pf, stream), "lphy_hip_hamming_batch")


def checksum_batch(buf, frames, stride, length, kind, out, stream=None):
    _chk(load().lphy_hip_checksum_batch(_dptr(buf, "buf", frames * stride, 1), frames, stride, length, kind,
                                        _dptr(out, "out", frames * 2, 2), stream), "lphy_hip_checksum_batch")


def lora_encode_batch(data, frames, stride, length, syms, sym_stride, stream=None):
    """lora_encode (LoRaEncoder.cpp:6-18) per row on device tensors."""
    _chk(load().lphy_hip_lora_encode_batch(_dptr(data, "data", frames * stride, 1), frames, stride, length,
                                           _dptr(syms, "syms", frames * sym_stride * 2, 2), sym_stride, stream),
         "lphy_hip_lora_encode_batch")


# --- LoRaWAN (lorawan.cpp) ----------------------------
LW_APPEND = 1
# lphy_lorawan_desc / lphy_lorawan_frame (include/lphy_hip.h) as numpy dtypes
LORAWAN_DESC_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u4"), ("devaddr", "<u4"), ("fcnt", "<u4"),
                               ("key", "<u4"), ("uplink", "<u4"), ("reserved", "<u4")])
LORAWAN_FRAME_DTYPE = np.dtype([("status", "<i4"), ("devaddr", "<u4"), ("mic", "<u4"), ("calc_mic", "<u4"),
                                ("payload_offset", "<u4"), ("payload_len", "<u4"), ("fcnt", "<u2"),
                                ("mhdr", "u1"), ("fctrl", "u1"), ("fopts_len", "u1"), ("reserved", "u1", 3)])


def lorawan_mic_batch(data, desc, keys, mic=None, flags=0, stream=None):
    """compute_mic for every descriptor row.  data: uint8 device tensor;
    desc: device tensor holding len(desc) LORAWAN_DESC_DTYPE records (bytes);
    keys: uint8 device tensor of 16-byte keys; mic: int32 device tensor."""
    frames = desc.numel() * desc.element_size() // 32
    nkeys = keys.numel() // 16
    pm = _dptr(mic, "mic", frames * 4, 4) if mic is not None else None
    _chk(load().lphy_hip_lorawan_mic_batch(_dptr(data, "data", 1, 1), _dptr(desc, "desc", frames * 32), frames,
                                           _dptr(keys, "keys", nkeys * 16, 1), nkeys, pm, flags, stream),
         "lphy_hip_lorawan_mic_batch")


def lorawan_parse_batch(data, frames, stride, length, keys, out, lens=None, key_index=None, stream=None):
    """parse_frame's checks on `frames` rows of decoded bytes; out: device
    tensor of frames * 32 bytes (view it as LORAWAN_FRAME_DTYPE on the host)."""
    nkeys = keys.numel() // 16
    pl = _dptr(lens, "lens", frames * 4, 4) if lens is not None else None
    pk = _dptr(key_index, "key_index", frames * 4, 4) if key_index is not None else None
    _chk(load().lphy_hip_lorawan_parse_batch(_dptr(data, "data", (frames - 1) * stride + 1 if frames else 0, 1),
                                             frames, stride, pl, length, _dptr(keys, "keys", nkeys * 16, 1),
                                             nkeys, pk, _dptr(out, "out", frames * 32), stream),
         "lphy_hip_lorawan_parse_batch")


# lphy_lorawan_tx / lphy_lorawan_session (include/lphy_hip.h): LoRaWAN on the
# ragged table
LORAWAN_TX_DTYPE = np.dtype([("src_offset", "<u8"), ("devaddr", "<u4"), ("key", "<u4"), ("payload_len", "<u4"),
                             ("fcnt", "<u2"), ("mtype", "u1"), ("major", "u1"), ("fctrl", "u1"),
                             ("fopts_len", "u1"), ("reserved", "u1", 6)])
LORAWAN_SESSION_DTYPE = np.dtype([("devaddr", "<u4"), ("key", "<u4")])
assert LORAWAN_TX_DTYPE.itemsize == 32 and LORAWAN_SESSION_DTYPE.itemsize == 8
LW_NO_KEY = 0xFFFFFFFF


def lorawan_sessions_check(sessions) -> bool:
    """True when `sessions` (LORAWAN_SESSION_DTYPE, host) is sorted by devaddr
    ascending, as lorawan_parse_ragged's lookup needs it."""
    s = np.ascontiguousarray(sessions, LORAWAN_SESSION_DTYPE).reshape(-1)
    return load().lphy_hip_lorawan_sessions_check(s.ctypes.data if s.size else None, s.size) == 0


def lorawan_build_ragged(src, tx, desc, frames, symbol_samples, keys, data, status, syms_out=None, stream=None,
                         src_bytes=None, out_syms=None):
    """build_frame for every frame of a ragged table (lphy_hip_lorawan_build_ragged),
    device tensors throughout.  src: FOpts then FRMPayload of frame f at
    tx[f]["src_offset"]; tx: frames LORAWAN_TX_DTYPE records; desc: frames + 1
    RAGGED_DESC_DTYPE records (Demodulator.lorawan_tx_layout); symbol_samples:
    Demodulator.symbol_samples(); data: the frames' bytes at sym_offset // 2;
    syms_out (optional): their symbols at sym_offset; status: int32 per frame,
    2 * bytes or a negative errno.  src_bytes / out_syms: the extents the
    records span (checked against the tensors).  Asynchronous."""
    nkeys = keys.numel() // 16
    ps = _dptr(syms_out, "syms_out", (out_syms or 0) * 2, 2) if syms_out is not None else None
    _chk(load().lphy_hip_lorawan_build_ragged(
        _dptr(src, "src", src_bytes or 0, 1), _dptr(tx, "tx", frames * 32), _dptr(desc, "desc", (frames + 1) * 32),
        frames, symbol_samples, _dptr(keys, "keys", nkeys * 16, 1), nkeys,
        _dptr(data, "data", ((out_syms or 0) + 1) // 2, 1), ps, _dptr(status, "status", frames * 4, 4), stream),
        "lphy_hip_lorawan_build_ragged")


def lorawan_parse_ragged(data, desc, frames, symbol_samples, mode, keys, out, meta=None, key_index=None,
                         sessions=None, key_used=None, stream=None, out_syms=None):
    """parse_frame's checks on the bytes demod_ragged(mode, F_DECODE) left at
    sym_offset // 2 (lphy_hip_lorawan_parse_ragged), device tensors throughout.
    out: frames * 32 bytes (LORAWAN_FRAME_DTYPE); meta (optional): the
    demodulator's records, whose nonzero status becomes the frame's; the key is
    key_index[f], key 0, or found by DevAddr in `sessions` (LORAWAN_SESSION_DTYPE
    records sorted by devaddr; at most one of the two); key_used (optional):
    int32 per frame, LW_NO_KEY where no MIC was computed.  out_syms: the symbol
    extent the descriptors span (checked against `data`).  Asynchronous."""
    nkeys = keys.numel() // 16
    pm = _dptr(meta, "meta", frames * 32) if meta is not None else None
    pk = _dptr(key_index, "key_index", frames * 4, 4) if key_index is not None else None
    nsess = sessions.numel() * sessions.element_size() // 8 if sessions is not None else 0
    pse = _dptr(sessions, "sessions", nsess * 8) if sessions is not None else None
    pu = _dptr(key_used, "key_used", frames * 4, 4) if key_used is not None else None
    _chk(load().lphy_hip_lorawan_parse_ragged(
        _dptr(data, "data", ((out_syms or 0) + 1) // 2, 1), _dptr(desc, "desc", (frames + 1) * 32), frames,
        symbol_samples, mode, pm, _dptr(keys, "keys", nkeys * 16, 1), nkeys, pk, pse, nsess,
        _dptr(out, "out", frames * 32), pu, stream), "lphy_hip_lorawan_parse_ragged")


def lorawan_mic(key, uplink, devaddr, fcnt, data, device=0):
    """One compute_mic on the GPU from host bytes."""
    k = np.frombuffer(bytes(key), np.uint8)
    d = np.frombuffer(bytes(data) + b"\0", np.uint8)
    out = C.c_uint32()
    _chk(load().lphy_hip_lorawan_mic_host(device, k.ctypes.data, int(uplink), devaddr & 0xFFFFFFFF,
                                          fcnt & 0xFFFFFFFF, d.ctypes.data, len(data), C.byref(out)),
         "lphy_hip_lorawan_mic_host")
    return out.value


# --- the FRMPayload cipher (LoRaWAN 1.0.x 4.3.3; include/lphy_hip.h) -------
LW_CRYPT_MAX = 4080  # bytes of one range: 255 keystream blocks


def lorawan_crypt_batch(data, desc, keys, status=None, stream=None):
    """The payload cipher in place on the range of every descriptor row
    (lphy_hip_lorawan_crypt_batch).  data: uint8 device tensor; desc: device
    tensor holding LORAWAN_DESC_DTYPE records (bytes); keys: uint8 device tensor
    of 16-byte keys; status (optional): int32 per job, 0 or a negative errno.
    Asynchronous."""
    jobs = desc.numel() * desc.element_size() // 32
    nkeys = keys.numel() // 16
    ps = _dptr(status, "status", jobs * 4, 4) if status is not None else None
    _chk(load().lphy_hip_lorawan_crypt_batch(_dptr(data, "data", 1, 1), _dptr(desc, "desc", jobs * 32), jobs,
                                             _dptr(keys, "keys", nkeys * 16, 1), nkeys, ps, stream),
         "lphy_hip_lorawan_crypt_batch")


def lorawan_crypt_tx_ragged(src, tx, frames, keys, skip=0, status=None, stream=None, src_bytes=None):
    """The payload cipher on the FRMPayload of every frame of `tx`, in place in
    `src`, before lorawan_build_ragged reads it (lphy_hip_lorawan_crypt_tx_ragged).
    src, tx, src_bytes as for lorawan_build_ragged; keys: the payload keys,
    indexed like build's; skip: 1 leaves the first FRMPayload byte clear;
    status (optional): int32 per frame.  Asynchronous."""
    nkeys = keys.numel() // 16
    ps = _dptr(status, "status", frames * 4, 4) if status is not None else None
    _chk(load().lphy_hip_lorawan_crypt_tx_ragged(
        _dptr(src, "src", src_bytes or 0, 1), _dptr(tx, "tx", frames * 32), frames,
        _dptr(keys, "keys", nkeys * 16, 1), nkeys, skip, ps, stream), "lphy_hip_lorawan_crypt_tx_ragged")


def lorawan_crypt_rx_ragged(data, desc, parsed, frames, symbol_samples, mode, keys, key_used=None, skip=0,
                            status=None, stream=None, out_syms=None):
    """The payload cipher on the FRMPayload of every frame lorawan_parse_ragged
    accepted, in place in `data` (lphy_hip_lorawan_crypt_rx_ragged).  data,
    desc, symbol_samples, mode, out_syms as for lorawan_parse_ragged; parsed:
    its `out`; key_used (optional): its key_used, int32 per frame (absent: key
    0); keys: the payload keys, indexed like parse's; status (optional): int32
    per frame.  The MICs in `data` no longer cover it afterwards.  Asynchronous."""
    nkeys = keys.numel() // 16
    pu = _dptr(key_used, "key_used", frames * 4, 4) if key_used is not None else None
    ps = _dptr(status, "status", frames * 4, 4) if status is not None else None
    _chk(load().lphy_hip_lorawan_crypt_rx_ragged(
        _dptr(data, "data", ((out_syms or 0) + 1) // 2, 1), _dptr(desc, "desc", (frames + 1) * 32),
        _dptr(parsed, "parsed", frames * 32), pu, frames, symbol_samples, mode,
        _dptr(keys, "keys", nkeys * 16, 1), nkeys, skip, ps, stream), "lphy_hip_lorawan_crypt_rx_ragged")


def lorawan_crypt(key, uplink, devaddr, fcnt, data, device=0) -> bytes:
    """The payload cipher on host bytes, once through the GPU: ciphertext of a
    plaintext and the other way round."""
    k = np.frombuffer(bytes(key), np.uint8)
    d = np.frombuffer(bytes(data) + b"\0", np.uint8).copy()
    _chk(load().lphy_hip_lorawan_crypt_host(device, k.ctypes.data, int(uplink), devaddr & 0xFFFFFFFF,
                                            fcnt & 0xFFFFFFFF, d.ctypes.data, len(data)),
         "lphy_hip_lorawan_crypt_host")
    return d[:len(data)].tobytes()
