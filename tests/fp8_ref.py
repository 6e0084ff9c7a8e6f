"""numpy restatement of the quantised row tables (include/euler_gpu.h, "quantised (FP8) feature row
tables"; euler_amd/csrc/fp8_cvt.h), independent of the package: nothing here imports euler_amd
or torch.

  dec(code)            the exact float32 value of an OCP e4m3fn code (0x7f / 0xff: NaN)
  enc(f)               float32 -> code: clamp to [-448, 448], round to nearest even, subnormals
  column_absmax(x)     max |x| over the finite values of a column
  column_scale(x)      absmax / 448 in float32, 1 where the column holds no non-zero finite value
  quantize(x, scale)   enc(x / scale), an IEEE float32 division
  dequantize(q, scale) float32(dec(q) * scale), one float32 multiply

An op on a table is the existing reference (mp_base_ref.py, weighted_mp_ref.py) on dequantize()."""
import numpy as np

FP8_MAX = np.float32(448.0)


def _dec_table():
    c = np.arange(256, dtype=np.int64)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e.astype(np.float64) - 10))
    v = np.where(c & 0x80, -mag, mag).astype(np.float32)
    v[0x7f] = np.float32(np.nan)
    v[0xff] = -np.float32(np.nan)
    return v


DEC = _dec_table()


def dec(codes):
    return DEC[np.asarray(codes, np.uint8)]


def enc(f):
    """Round to nearest, ties to even, done in float64 where every step below is exact: a float32
    scaled by a power of two, np.rint (ties to even) of it, and the comparison with 2^k."""
    f = np.asarray(f, np.float32)
    sign = (f.view(np.uint32) >> 24).astype(np.uint8) & 0x80
    nan = np.isnan(f)
    a = np.minimum(np.abs(np.where(nan, 0, f)).astype(np.float64), 448.0)
    # the exponent of the result's binade: floor(log2 a), at least -6 (the subnormals share 2^-6's step)
    _, ex = np.frexp(a)
    e = np.maximum(ex - 1, -6)
    step = np.ldexp(1.0, e - 3)                      # the spacing of codes in that binade
    k = np.rint(a / step)                            # the value in steps: 0 .. 16 (16: the next binade)
    val = k * step
    _, ex2 = np.frexp(val)
    e2 = np.maximum(ex2 - 1, -6)
    man = np.rint(val / np.ldexp(1.0, e2 - 3)).astype(np.int64)       # 0 .. 15
    code = np.where(man >= 8, ((e2 + 7) << 3) | (man - 8), man).astype(np.uint8)
    code = np.where(nan, 0x7f, code).astype(np.uint8)
    return code | sign


def column_absmax(x):
    x = np.asarray(x, np.float32)
    a = np.where(np.isfinite(x), np.abs(x), np.float32(0))
    return a.max(axis=0).astype(np.float32) if x.shape[0] else np.zeros(x.shape[1], np.float32)


def scale_of(absmax):
    absmax = np.asarray(absmax, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(absmax > 0, (absmax / FP8_MAX).astype(np.float32), np.float32(1)).astype(np.float32)


def column_scale(x):
    return scale_of(column_absmax(x))


def quantize(x, scale):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return enc((x / np.asarray(scale, np.float32)).astype(np.float32))


def dequantize(q, scale):
    with np.errstate(all="ignore"):
        return (dec(q) * np.asarray(scale, np.float32)).astype(np.float32)
