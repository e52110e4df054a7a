"""What the tests of lphy_hip_channelize_raw share: the definition's conversion
of an integer capture to the float32 capture x' (include/lphy_hip.h), and a
quantiser that makes integer captures for them.

to_float(): numpy's integer-to-float32 conversion and its float32 subtraction
are the same exact operations as the definition's (every int16, int8 and
uint8 - 127.5 is a float32)."""
import numpy as np

FMT_CF32, FMT_SC16, FMT_SC8, FMT_CU8 = 0, 1, 2, 3          # enum lphy_sample_format
INT_FORMATS = [FMT_SC16, FMT_SC8, FMT_CU8]
NAMES = {FMT_CF32: "cf32", FMT_SC16: "sc16", FMT_SC8: "sc8", FMT_CU8: "cu8"}
DTYPES = {FMT_CF32: np.dtype(np.float32), FMT_SC16: np.dtype("<i2"), FMT_SC8: np.dtype(np.int8),
          FMT_CU8: np.dtype(np.uint8)}
BYTES = {FMT_CF32: 8, FMT_SC16: 4, FMT_SC8: 2, FMT_CU8: 2}  # one I/Q pair


def to_float(x, fmt):
    """The complex64 capture x' of the definition: `x` holds interleaved I, Q of
    fmt's dtype, [n, 2] or flat."""
    x = np.asarray(x)
    assert x.dtype == DTYPES[fmt], (x.dtype, fmt)
    f = x.reshape(-1, 2).astype(np.float32)
    if fmt == FMT_CU8:
        f = f - np.float32(127.5)
    assert f.dtype == np.float32
    return np.ascontiguousarray(f).view(np.complex64).reshape(-1)


def quantise(z, fmt, scale):
    """Complex samples `z` times `scale` as a capture of `fmt`, [n, 2]: rounded
    to the nearest level (for CU8 the levels are the half-integers byte - 127.5)
    and clipped to the format's range."""
    z = np.asarray(z, np.complex128).reshape(-1)
    v = np.stack([z.real, z.imag], axis=1) * float(scale)
    if fmt == FMT_CU8:
        return np.clip(np.rint(v + 127.5), 0, 255).astype(np.uint8)
    info = np.iinfo(DTYPES[fmt])
    return np.clip(np.rint(v), info.min, info.max).astype(DTYPES[fmt])


def random_capture(rng, n, fmt):
    """n samples over the format's whole range, [n, 2]."""
    if fmt == FMT_CF32:
        return rng.standard_normal((n, 2)).astype(np.float32)
    info = np.iinfo(DTYPES[fmt])
    return rng.integers(info.min, info.max + 1, (n, 2)).astype(DTYPES[fmt])
