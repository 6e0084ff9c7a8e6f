"""tests/fp8_ref.py - the numpy restatement the GPU tests of the quantised row tables compare
against - pinned to torch's CPU float8_e4m3fn and to the bounds the format itself gives.  CPU only."""
import numpy as np
import torch

import fp8_edges as E
import fp8_ref as R


def test_dec_and_enc_equal_torch():
    codes = np.arange(256, dtype=np.uint8)
    got, want = R.dec(codes), E.dec_cpu(codes)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    p = E.encode_set()
    bad = E.enc_mismatches(R.enc(p.view(np.float32)), p)
    assert bad.size == 0, [hex(int(p[i])) for i in bad[:8]]


def _table(rng, n, d):
    """values over many binades, with per-column magnitudes that differ"""
    x = rng.standard_normal((n, d)).astype(np.float32) * np.exp2(rng.integers(-8, 9, (n, d))).astype(np.float32)
    return x * np.exp2(rng.integers(-20, 20, d)).astype(np.float32)


def test_quantize_equals_torchs_cast_of_the_quotient():
    rng = np.random.default_rng(40)
    x = _table(rng, 4096, 24)
    x[::7, 3] = 0
    x[5, 4], x[6, 4], x[7, 4] = np.nan, np.inf, -np.inf
    for scale in (R.column_scale(x), np.ones(24, np.float32),
                  (R.column_scale(x) * np.float32(0.37)).astype(np.float32)):       # (one that clips)
        assert scale.dtype == np.float32 and np.all(scale > 0) and np.all(np.isfinite(scale))
        got = R.quantize(x, scale)
        quot = (torch.from_numpy(x) / torch.from_numpy(scale))
        assert quot.dtype == torch.float32
        bad = E.enc_mismatches(got, quot.contiguous())
        assert bad.size == 0
    # the edge set through a scale whose division is inexact
    p = E.encode_set().view(np.float32).reshape(-1, 3)
    scale = np.array([3.0, 0.7, 1.1], np.float32)
    with np.errstate(all="ignore"):
        quot = torch.from_numpy(np.array(p)) / torch.from_numpy(scale)
    assert E.enc_mismatches(R.quantize(p, scale), quot.contiguous()).size == 0


def test_the_bound_of_a_quantised_value():
    """Derived from the format: a normal e4m3 has 3 mantissa bits, so round-to-nearest is off by at
    most half a step = 2^-4 of the value's binade <= 2^-4 |y| for y = x / scale with |y| >= 2^-6;
    below 2^-6 the step is 2^-9, half of it 2^-10.  x^ = fl(dec * scale) and y = fl(x / scale) add
    one fp32 rounding each: a factor (1 + 2^-22) covers both (2 * 2^-24 and their product, rounded up)."""
    rng = np.random.default_rng(41)
    x = _table(rng, 8192, 16)
    scale = R.column_scale(x)
    xh = R.dequantize(R.quantize(x, scale), scale).astype(np.float64)
    x64, s64 = x.astype(np.float64), scale.astype(np.float64)
    assert np.all(np.abs(x64 / s64) <= 448 * (1 + 2.0 ** -22))          # the column's own scale never clips
    err = np.abs(xh - x64)
    wide = 1 + 2.0 ** -22
    big = np.abs(x64 / s64) >= 2.0 ** -6
    assert big.sum() > 1000 and (~big).sum() > 1000
    assert np.all(err[big] <= 2.0 ** -4 * np.abs(x64[big]) * wide)
    assert np.all(err[~big] <= (2.0 ** -10 * s64 * wide)[None, :].repeat(x.shape[0], 0)[~big])


def test_chunked_absmax_and_the_special_columns():
    rng = np.random.default_rng(42)
    x = _table(rng, 1000, 8)
    x[:, 2] = 0                                          # a column of zeros
    x[:, 5] = np.where(rng.random(1000) < 0.5, np.nan, np.inf)      # nothing finite
    x[3, 6], x[4, 6], x[5, 6] = np.nan, np.inf, -np.inf  # skipped among finite values
    x[9, 7] = -0.0
    whole = R.column_absmax(x)
    parts = np.zeros(8, np.float32)
    for lo, hi in ((0, 1), (1, 400), (400, 400), (400, 1000)):
        parts = np.maximum(parts, R.column_absmax(x[lo:hi]))
    assert np.array_equal(parts.view(np.uint32), whole.view(np.uint32))
    finite = np.where(np.isfinite(x), np.abs(x), 0).astype(np.float64)
    assert np.array_equal(whole.astype(np.float64), finite.max(0))
    scale = R.scale_of(whole)
    assert scale[2] == 1 and scale[5] == 1 and whole[6] == finite[:, 6].max() and whole[6] > 0
    assert np.array_equal(scale[[0, 1, 3, 4, 6, 7]], (whole / np.float32(448))[[0, 1, 3, 4, 6, 7]])
    q = R.quantize(x, scale)
    assert np.all(q[:, 2] == 0) and q[3, 6] & 0x7f == 0x7f and q[4, 6] == 0x7e and q[5, 6] == 0xfe
    assert q[9, 7] == 0x80
    # the largest value of a column is the largest code
    for c in (0, 1, 3, 4, 6, 7):
        assert (q[:, c] & 0x7f)[~E.nan_code(q[:, c])].max() == 0x7e
