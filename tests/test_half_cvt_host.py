"""The host forms of euler_amd/csrc/half_cvt.h - the conversions behind the bf16 / fp16 feature
tables and message-passing kernels - against torch's own CPU conversions.  CPU only.

Every comparison is bit equality.  The one exception is the payload of a NaN result: torch's
CPU paths (scalar and vectorised) do not agree among themselves on it, so a NaN is only
required to stay a NaN (the header makes it a quiet one and keeps its sign)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from half_edges import classes, edge_bits, narrow_set

HERE = os.path.dirname(os.path.abspath(__file__))
u16p, f32p = C.POINTER(C.c_uint16), C.POINTER(C.c_float)
DT = {torch.bfloat16: 1, torch.float16: 2}


@pytest.fixture(scope="module")
def HCV():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libhalf_cvt_check.so")
    src = os.path.join(HERE, "csrc", "half_cvt_check.cc")
    deps = [src, os.path.join(ROOT, "euler_amd", "csrc", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    for name in ("hcv_widen", "hcv_widen8"):
        getattr(L, name).argtypes = [C.c_int, u16p, C.c_int64, f32p]
        getattr(L, name).restype = None
    for name in ("hcv_narrow", "hcv_narrow8"):
        getattr(L, name).argtypes = [C.c_int, f32p, C.c_int64, u16p]
        getattr(L, name).restype = None
    return L


def _widen(L, fn, dtype, bits):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    out = np.empty(bits.size, np.float32)
    getattr(L, fn)(DT[dtype], bits.ctypes.data_as(u16p), bits.size, out.ctypes.data_as(f32p))
    return out


def _narrow(L, fn, dtype, f_bits):
    f = np.ascontiguousarray(f_bits, dtype=np.uint32).view(np.float32)
    out = np.empty(f.size, np.uint16)
    getattr(L, fn)(DT[dtype], f.ctypes.data_as(f32p), f.size, out.ctypes.data_as(u16p))
    return out


def _torch_widen(dtype, bits):
    t = torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).view(dtype)
    return t.float().numpy()


def _torch_narrow(dtype, f_bits):
    t = torch.from_numpy(np.ascontiguousarray(f_bits, dtype=np.uint32).view(np.int32)).view(torch.float32)
    return t.to(dtype).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_every_16_bit_pattern_widens_to_torchs_float(HCV, dtype):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    want = _torch_widen(dtype, bits)
    for fn in ("hcv_widen", "hcv_widen8"):
        got = _widen(HCV, fn, dtype, bits)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), fn
        assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), fn
        # a NaN keeps its sign (bf16 widens by a shift: the payload is the input's)
        assert np.array_equal(got.view(np.uint32)[nan] >> 31, (bits[nan] >> 15).astype(np.uint32))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_narrowing_equals_torchs_to(HCV, dtype):
    # the edge list, 2^20 uniform patterns, 2^18 with a uniform binade, 2^14 exact ties with their
    # fp32 neighbours (a multiple of 8 patterns)
    f_bits = narrow_set(dtype)
    assert f_bits[:edge_bits(dtype).size].tolist() == edge_bits(dtype).tolist() and f_bits.size % 8 == 0
    want = _torch_narrow(dtype, f_bits)
    exp_mask, man_mask = (0x7f80, 0x007f) if dtype == torch.bfloat16 else (0x7c00, 0x03ff)
    want_nan = ((want & exp_mask) == exp_mask) & ((want & man_mask) != 0)
    in_nan = np.isnan(f_bits.view(np.float32))
    assert np.array_equal(want_nan, in_nan)
    quiet = 0x0040 if dtype == torch.bfloat16 else 0x0200
    for fn in ("hcv_narrow", "hcv_narrow8"):
        got = _narrow(HCV, fn, dtype, f_bits)
        got_nan = ((got & exp_mask) == exp_mask) & ((got & man_mask) != 0)
        assert np.array_equal(got_nan, in_nan), fn
        bad = np.flatnonzero((got != want) & ~in_nan)
        assert bad.size == 0, (fn, [hex(int(x)) for x in f_bits[bad[:8]]])
        assert np.all((got[in_nan] & quiet) != 0)
        assert np.array_equal(got[in_nan] >> 15, (f_bits[in_nan] >> 31).astype(np.uint16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_round_trip_is_the_identity_on_16_bit_values(HCV, dtype):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    wide = _widen(HCV, "hcv_widen", dtype, bits)
    keep = ~np.isnan(wide)
    back = _narrow(HCV, "hcv_narrow", dtype, wide.view(np.uint32))
    assert np.array_equal(back[keep], bits[keep])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_the_patterns_reach_every_class(dtype):
    """A condition on the INPUTS, against the CPU reference alone: the set every narrowing path is
    checked on (here and on the GPU) holds at least 1000 results of each class.  bf16 alone has
    few finite values that round to inf - the edge list, the ties at the top binade and what the
    uniform draws give - and needs 10."""
    got = classes(narrow_set(dtype), dtype)
    for name in ("normal", "subnormal", "zero", "nan", "tie"):
        assert got[name] >= 1000, (name, got)
    assert got["to_inf"] >= (10 if dtype == torch.bfloat16 else 1000), got
