"""Inputs at the rounding edges of OCP e4m3fn and the CPU reference for them: torch's own CPU
float8_e4m3fn conversions, as integer bits.  Shared by tests/test_fp8_cvt_host.py (the integer
forms of euler_amd/csrc/fp8_cvt.h on the host), tests/test_fp8_ref_host.py (the numpy restatement)
and tests/test_fp8_rows_gpu.py (the device forms), so that every side of the chain
integer form == numpy == torch CPU == device  sees the same patterns.  No GPU import.

torch's CPU cast fp32 -> float8_e4m3fn rounds to nearest even and does NOT saturate (a value past
the last tie becomes NaN), so the reference of Enc is x.clamp(-448, 448).to(float8_e4m3fn).  The
comparison rule: a NaN input gives a NaN code with the input's sign; everything else the same bits."""
import numpy as np
import torch

F8 = torch.float8_e4m3fn


def code_values():
    """the fp32 value of every code, by torch's CPU cast, as uint32 bits [256]"""
    c = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(F8)
    return c.float().view(torch.int32).numpy().view(np.uint32)


def _finite_magnitudes():
    """the 127 non-negative finite values 0 .. 448 in code order, float64"""
    v = code_values()[:0x7f].view(np.float32).astype(np.float64)
    assert v[0] == 0 and v[-1] == 448 and np.all(np.diff(v) > 0)
    return v


def tie_magnitudes():
    """every exact tie between adjacent codes (2^-10, between 0 and the smallest subnormal, first)
    and 464, the tie between 448 and the 480 the format does not have; float32, exact"""
    v = _finite_magnitudes()
    t = np.concatenate([(v[:-1] + v[1:]) / 2, [464.0]])
    t32 = t.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), t) and t32[0] == 2.0 ** -10
    return t32


def _with_neighbours(b):
    """uint32 patterns of finite values -> each with the fp32 pattern below and above it"""
    b = np.asarray(b, np.uint32)
    lo = np.where((b & 0x7fffffff) == 0, b ^ 0x80000001, b - 1)      # below +-0: the other sign's first
    return np.stack([b, lo, b + 1], 1).reshape(-1)


def edge_bits():
    """fp32 bit patterns around every rounding decision of the format"""
    vals = code_values()
    finite = vals[(np.arange(256) & 0x7f) != 0x7f]
    ties = tie_magnitudes().view(np.uint32)
    ties = np.concatenate([ties, ties | 0x80000000])
    special = np.array([0x43e00000, 0xc3e00000,                       # +-448
                        0x7f800000, 0xff800000, 0x00000000, 0x80000000,
                        0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff,
                        0x3a800000, 0xba800000, 0x43e80000, 0xc3e80000,          # +-2^-10, +-464
                        0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff],
                       dtype=np.uint32)
    return np.concatenate([special, _with_neighbours(finite), _with_neighbours(ties)])


def uniform_bits(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def ranged_bits(n, seed):
    """n fp32 patterns with a random sign and mantissa and the binade uniform over 2^-12 .. 2^10:
    the format's window (2^-9 .. 448) widened by three binades below and one above"""
    rng = np.random.default_rng(seed)
    e = rng.integers(-12, 11, n, dtype=np.int64)
    man = rng.integers(0, 1 << 23, n, dtype=np.int64)
    sign = rng.integers(0, 2, n, dtype=np.int64) << 31
    return (sign | ((e + 127) << 23) | man).astype(np.uint32)


def repeated_ties(times, seed):
    """The format has 127 ties a sign; the set holds each `times` times in a shuffled order, so
    that a tie meets many lanes, columns and (in the GPU test) column scales."""
    t = tie_magnitudes().view(np.uint32)
    t = np.tile(np.concatenate([t, t | 0x80000000]), times)
    np.random.default_rng(seed).shuffle(t)
    return t


_SET = []


def encode_set():
    """P: the patterns every encoding path is checked on, padded with +0 to a multiple of 48 (rows of
    16 and of 3 columns).  Read-only, built once."""
    if not _SET:
        p = np.concatenate([edge_bits(), uniform_bits(1 << 20, 30), ranged_bits(1 << 18, 31),
                            repeated_ties(8, 32)])
        p = np.concatenate([p, np.zeros((-p.size) % 48, np.uint32)])
        p.setflags(write=False)
        _SET.append(p)
    return _SET[0]


def bits32(x):
    if torch.is_tensor(x):
        assert x.dtype == torch.float32
        return x.detach().contiguous().cpu().view(torch.int32).numpy().view(np.uint32).reshape(-1)
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.uint32), x.dtype
    return x.view(np.uint32).reshape(-1)


def enc_cpu(x32):
    """the reference of Enc: torch's x.clamp(-448, 448).to(float8_e4m3fn) of fp32 values (or uint32
    bits), as uint8 codes"""
    b = np.array(bits32(x32))
    t = torch.from_numpy(b.view(np.int32)).view(torch.float32)
    return t.clamp(-448.0, 448.0).to(F8).view(torch.uint8).numpy()


def dec_cpu(codes):
    """torch's float8_e4m3fn -> fp32 of uint8 codes, as float32"""
    c = torch.from_numpy(np.array(codes, dtype=np.uint8))
    return c.view(F8).float().numpy()


def nan_code(c):
    return (np.asarray(c, np.uint8) & 0x7f) == 0x7f


def enc_mismatches(got, x32):
    """positions where the codes `got` break the rule against enc_cpu(x32)"""
    b = bits32(x32)
    got = np.asarray(got, np.uint8).reshape(-1)
    want = enc_cpu(b)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan_in = (b & 0x7fffffff) > 0x7f800000
    assert np.array_equal(nan_code(want), nan_in)           # the reference never overflows into NaN
    ok_nan = got == (0x7f | ((b >> 24) & 0x80)).astype(np.uint8)
    return np.flatnonzero(np.where(nan_in, ~ok_nan, got != want))


def classes(x32):
    """How many of the fp32 values (or bits) fall into each class, by the CPU reference's result:
    normal, subnormal, zero, nan, saturated (|x| > 448, inf included) and tie (an exact tie between
    adjacent codes, 2^-10 and 464 included, whatever it rounds to)."""
    b = bits32(x32)
    r = enc_cpu(b)
    a = b & 0x7fffffff
    e, m = (r >> 3) & 15, r & 7
    nan = nan_code(r)
    return {
        "n": int(b.size),
        "normal": int(((e != 0) & ~nan & (a <= 0x43e00000)).sum()),
        "subnormal": int(((e == 0) & (m != 0)).sum()),
        "zero": int(((e == 0) & (m == 0)).sum()),
        "nan": int(nan.sum()),
        "saturated": int(((a > 0x43e00000) & (a <= 0x7f800000)).sum()),
        "tie": int(np.isin(a, tie_magnitudes().view(np.uint32)).sum()),
    }
