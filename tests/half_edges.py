"""Inputs at the rounding edges of bf16 / fp16 and the CPU reference for them: torch's own CPU
conversions, as integer bits.  Shared by tests/test_half_cvt_host.py (the integer forms of
euler_amd/csrc/half_cvt.h, on the host) and the GPU tests of the device forms
(tests/test_half_cvt_gpu.py, tests/test_half_store_edges_gpu.py), so that both sides of the
chain  integer form == torch CPU == device form  see the same patterns.  No GPU import.

The comparison rule: a NaN stays a NaN with its sign (torch's CPU paths do not agree among
themselves on a NaN's payload, and not all of them keep its sign, so the sign is taken from the
INPUT); every other result is compared for bit equality."""
import numpy as np
import torch

# (exponent mask, mantissa mask, quiet bit, mantissa bits of fp32 that leave)
_FMT = {torch.bfloat16: (0x7f80, 0x007f, 0x0040, 16), torch.float16: (0x7c00, 0x03ff, 0x0200, 13)}


def edge_bits(dtype):
    """fp32 bit patterns around every rounding decision of the format"""
    out = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001,
           0xff800001, 0x7fffffff, 0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff,
           0xff7fffff]
    drop = 16 if dtype == torch.bfloat16 else 13          # mantissa bits that leave
    half = 1 << (drop - 1)
    for base in (0x3f800000, 0x3f810000, 0x40490000, 0xbf800000, 0xc2f70000, 0x00800000, 0x3effe000):
        base &= ~((1 << drop) - 1)
        for odd in (0, 1):                                  # ties towards an even and an odd neighbour
            b = base + (odd << drop)
            out += [b + half, b + half - 1, b + half + 1, b, b + (1 << drop) - 1]
    if dtype == torch.bfloat16:
        # the largest finite bf16 is 0x7f7f: 0x7f7f7fff stays, 0x7f7f8000 is the first to reach inf
        out += [0x7f7f0000, 0x7f7f7fff, 0x7f7f8000, 0x7f7f8001, 0xff7f7fff, 0xff7f8000]
    else:
        # 65504 = 0x477fe000 is the largest finite fp16; 65520 = 0x477ff000 the first to reach inf
        out += [0x477fe000, 0x477fefff, 0x477ff000, 0x477ff001, 0x47800000, 0xc77fefff, 0xc77ff000,
                0x4b000000, 0x7f000000]
        # subnormal range: 2^-14 = 0x38800000 (smallest normal), 2^-24 = 0x33800000 (smallest
        # subnormal), 2^-25 = 0x33000000 (its tie with zero)
        for b in (0x38800000, 0x387fffff, 0x387fe000, 0x387ff000, 0x387ff001, 0x38000000, 0x33800000,
                  0x33000000, 0x33000001, 0x32ffffff, 0x33c00000, 0x33bfffff, 0x33c00001, 0x34200000,
                  0x34600000, 0x32000000, 0x37000000, 0x37001000, 0x37003000):
            out += [b, b | 0x80000000]
        rng = np.random.default_rng(5)
        sub = rng.integers(0x32800000, 0x38900000, 4096, dtype=np.int64)      # 2^-26 .. 2^-14
        out += sub.tolist() + (sub | 0x80000000).tolist()
    return np.array(out, dtype=np.uint32)


def uniform_bits(n, seed):
    """n uniformly random 32-bit patterns"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def ranged_bits(dtype, n, seed):
    """n fp32 patterns with a random sign and mantissa and the BINADE uniform over the format's
    representable window widened by two binades on each side: fp16 [2^-27, 2^18); bf16 every fp32
    binade from the smallest fp32 subnormal 2^-149 (bf16's smallest subnormal is 2^-133) up to
    [2^127, 2^128).  A binade below 2^-126 is an fp32 subnormal: the leading bit sits in the
    mantissa field and only the bits below it are random."""
    rng = np.random.default_rng(seed)
    lo, hi = (-27, 17) if dtype == torch.float16 else (-149, 127)
    e = rng.integers(lo, hi + 1, n, dtype=np.int64)
    man = rng.integers(0, 1 << 23, n, dtype=np.int64)
    sign = rng.integers(0, 2, n, dtype=np.int64) << 31
    lead = np.clip(e + 149, 0, 23)                           # subnormal: position of the leading bit
    sub = (np.int64(1) << lead) | (man & ((np.int64(1) << lead) - 1))
    bits = np.where(e >= -126, ((e + 127) << 23) | man, sub)
    return (sign | bits).astype(np.uint32)


def tie_bits(dtype, n, seed):
    """3 * n fp32 patterns: n exact ties of the format, each followed by its two fp32 neighbours
    (one unit in the last fp32 place below and above it).  A tie is a finite 16-bit value of
    `dtype`, widened on the CPU, plus exactly half a unit of ITS last place away from zero - the
    16-bit patterns are random, so the kept bit has both parities - and the first patterns are the
    ones whose upper neighbour is inf (the largest finite value), the smallest normal (the largest
    subnormal) and the smallest subnormal (zero), with both signs."""
    exp_mask, man_mask, _, _ = _FMT[dtype]
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 1 << 16, n, dtype=np.int64)
    while True:
        bad = (h & exp_mask) == exp_mask                     # inf and NaN have no upper neighbour
        if not bad.any():
            break
        h[bad] = rng.integers(0, 1 << 16, int(bad.sum()), dtype=np.int64)
    top = exp_mask - (man_mask + 1) + man_mask               # the largest finite pattern
    special = [top, man_mask, 0, man_mask + 1, 1]
    special += [s | 0x8000 for s in special]
    h[:len(special)] = special
    v = widen_cpu(h.astype(np.uint16), dtype).view(np.float32).astype(np.float64)
    man_bits = 7 if dtype == torch.bfloat16 else 10
    e_min = -126 if dtype == torch.bfloat16 else -14
    _, ex = np.frexp(np.abs(v))                              # |v| = f * 2^ex, f in [0.5, 1)
    e = np.where(v == 0, e_min, np.maximum(ex - 1, e_min))
    half_ulp = np.ldexp(0.5, e - man_bits)
    tie64 = np.abs(v) + half_ulp
    tie = tie64.astype(np.float32)
    assert np.array_equal(tie.astype(np.float64), tie64)    # exact in fp32
    t = tie.view(np.uint32) | ((h.astype(np.uint32) & 0x8000) << 16)
    out = np.stack([t, t - 1, t + 1], 1).reshape(-1)
    assert not np.isnan(out.view(np.float32)).any() and not np.isinf(out.view(np.float32)).any()
    return out


def all16():
    """the 65 536 16-bit patterns"""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def narrow_set(dtype):
    """P: the patterns every narrowing path is checked on, padded with +0 to a multiple of 64"""
    p = np.concatenate([edge_bits(dtype), uniform_bits(1 << 20, 20), ranged_bits(dtype, 1 << 18, 21),
                        tie_bits(dtype, 1 << 14, 22)])
    return np.concatenate([p, np.zeros((-p.size) % 64, np.uint32)])


def bits32(x):
    """fp32 values as uint32 bits: a torch tensor (any device), a float32 or a uint32 array"""
    if torch.is_tensor(x):
        assert x.dtype == torch.float32
        return x.detach().contiguous().cpu().view(torch.int32).numpy().view(np.uint32).reshape(-1)
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.uint32), x.dtype
    return x.view(np.uint32).reshape(-1)


def bits16(x):
    """16-bit values as uint16 bits: a torch bf16 / fp16 tensor (any device) or a uint16 array"""
    if torch.is_tensor(x):
        assert x.dtype in _FMT
        return x.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16).reshape(-1)
    x = np.ascontiguousarray(x)
    assert x.dtype == np.uint16, x.dtype
    return x.reshape(-1)


def round_cpu(t32, dtype):
    """torch's CPU conversion fp32 -> dtype of the values (or uint32 bits) t32, as uint16 bits"""
    b = np.array(bits32(t32))                               # (a copy: the input may be read-only)
    t = torch.from_numpy(b.view(np.int32)).view(torch.float32)
    return t.to(dtype).view(torch.int16).numpy().view(np.uint16)


def widen_cpu(b16, dtype):
    """torch's CPU conversion dtype -> fp32 of the uint16 bits b16, as uint32 bits"""
    b = np.array(bits16(b16))
    t = torch.from_numpy(b.view(np.int16)).view(dtype)
    return t.float().view(torch.int32).numpy().view(np.uint32)


def nan_mask32(b32):
    return (bits32(b32) & 0x7fffffff) > 0x7f800000


def nan_mask16(b16, dtype):
    exp_mask, man_mask, _, _ = _FMT[dtype]
    b = bits16(b16)
    return ((b & exp_mask) == exp_mask) & ((b & man_mask) != 0)


def quiet_bit(dtype):
    return _FMT[dtype][2]


def mismatches16(got, want, dtype, sign_of):
    """Positions where the 16-bit results `got` break the comparison rule against `want` (both
    uint16 bits): a NaN of `want` must be a NaN with the sign of the input (sign_of: the 0 / 1 sign
    of every input), everything else the same bits."""
    got, want = bits16(got), bits16(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = nan_mask16(want, dtype)
    ok_nan = nan_mask16(got, dtype) & ((got >> 15) == np.asarray(sign_of).reshape(-1).astype(np.uint16))
    return np.flatnonzero(np.where(nan, ~ok_nan, got != want))


def mismatches32(got, want, sign_of):
    """the same rule for fp32 results (uint32 bits)"""
    got, want = bits32(got), bits32(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = nan_mask32(want)
    ok_nan = nan_mask32(got) & ((got >> 31) == np.asarray(sign_of).reshape(-1).astype(np.uint32))
    return np.flatnonzero(np.where(nan, ~ok_nan, got != want))


def is_tie(b32, dtype):
    """which fp32 patterns lie exactly half way between two adjacent values of dtype (inf counting
    as the value after the largest finite one)"""
    b = bits32(b32)
    a = b & 0x7fffffff
    finite = a < 0x7f800000
    if dtype == torch.bfloat16:
        return finite & ((b & 0xffff) == 0x8000)
    normal = (a >= 0x38800000) & (a < 0x47800000) & ((b & 0x1fff) == 0x1000)     # 2^-14 <= |x| < 2^16
    small = np.where(a < 0x38800000, a, 0).astype(np.uint32)                    # below 2^-14
    units = small.view(np.float32).astype(np.float64) * 2.0 ** 25               # of half the subnormal step
    sub = (units == np.floor(units)) & (np.mod(units, 2.0) == 1.0)
    return finite & (normal | sub)


def classes(t32, dtype):
    """How many of the fp32 values (or bits) t32 fall into each class of `dtype`, by the CPU
    reference's result: normal, subnormal, zero, NaN, to_inf (a FINITE value that rounds to inf),
    and tie (an exact tie, whatever it rounds to)."""
    b = bits32(t32)
    exp_mask, man_mask, _, _ = _FMT[dtype]
    r = round_cpu(b, dtype)
    e, m = r & exp_mask, r & man_mask
    finite_in = (b & 0x7fffffff) < 0x7f800000
    return {
        "n": int(b.size),
        "normal": int(((e != 0) & (e != exp_mask)).sum()),
        "subnormal": int(((e == 0) & (m != 0)).sum()),
        "zero": int(((e == 0) & (m == 0)).sum()),
        "nan": int(((e == exp_mask) & (m != 0)).sum()),
        "to_inf": int(((e == exp_mask) & (m == 0) & finite_in).sum()),
        "tie": int(is_tie(b, dtype).sum()),
    }


# ---- helpers of the GPU tests (tensors go to the current device; nothing is imported for it) ----
def to_dev16(b16, dtype):
    """uint16 bits -> a tensor of dtype on the GPU"""
    return torch.from_numpy(np.array(b16, dtype=np.uint16).view(np.int16)).cuda().view(dtype)


def to_dev32(b32):
    """uint32 bits -> an fp32 tensor on the GPU"""
    return torch.from_numpy(np.array(b32, dtype=np.uint32).view(np.int32)).cuda().view(torch.float32)


def assert_same16(got, want, dtype, src32, what):
    """got == want (16-bit results) under the NaN rule; src32: the fp32 values that were rounded,
    whose sign a NaN keeps.  A NaN result is also a quiet one (half_cvt.h)."""
    src32 = bits32(src32)
    g, w = bits16(got), bits16(want)
    bad = mismatches16(g, w, dtype, src32 >> 31)
    assert bad.size == 0, (what, "%d of %d differ" % (bad.size, g.size),
                           [(int(i), hex(int(src32[i])), hex(int(g[i])), hex(int(w[i]))) for i in bad[:8]])
    nan = nan_mask32(src32)
    assert np.all((g[nan] & quiet_bit(dtype)) != 0), (what, "a NaN result is not quiet")


def assert_same32(got, want, sign_of, what):
    """got == want (fp32 results) under the NaN rule"""
    g, w = bits32(got), bits32(want)
    bad = mismatches32(g, w, sign_of)
    assert bad.size == 0, (what, "%d of %d differ" % (bad.size, g.size),
                           [(int(i), hex(int(g[i])), hex(int(w[i]))) for i in bad[:8]])
