"""The host forms of euler_amd/csrc/fp8_cvt.h - the conversions behind the quantised (fp8 e4m3fn)
feature row tables - against torch's own CPU float8_e4m3fn conversions.  CPU only.

Every comparison is bit equality, except that a NaN need only stay a NaN with its sign.  torch's
CPU cast to float8 is round-to-nearest-even and non-saturating, so the reference of Enc is
x.clamp(-448, 448).to(torch.float8_e4m3fn) (fp8_edges.enc_cpu)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import fp8_edges as E

HERE = os.path.dirname(os.path.abspath(__file__))
u8p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def F8C():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libfp8_cvt_check.so")
    src = os.path.join(HERE, "csrc", "fp8_cvt_check.cc")
    deps = [src, os.path.join(ROOT, "euler_amd", "csrc", "fp8_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    for name in ("f8_dec", "f8_dec16"):
        getattr(L, name).argtypes = [u8p, C.c_int64, f32p]
        getattr(L, name).restype = None
    L.f8_enc.argtypes = [f32p, C.c_int64, u8p]
    L.f8_enc.restype = None
    return L


def _dec(L, fn, codes):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    out = np.empty(codes.size, np.float32)
    getattr(L, fn)(codes.ctypes.data_as(u8p), codes.size, out.ctypes.data_as(f32p))
    return out


def _enc(L, f_bits):
    f = np.ascontiguousarray(f_bits, dtype=np.uint32).view(np.float32)
    out = np.empty(f.size, np.uint8)
    L.f8_enc(f.ctypes.data_as(f32p), f.size, out.ctypes.data_as(u8p))
    return out


def test_every_code_decodes_to_torchs_float(F8C):
    codes = np.arange(256, dtype=np.uint8)
    want = E.dec_cpu(codes)
    assert want[0x7e] == 448 and want[0x01] == 2.0 ** -9 and np.isnan(want[[0x7f, 0xff]]).all()
    assert want.view(np.uint32)[0x80] == 0x80000000
    for fn in ("f8_dec", "f8_dec16"):
        got = _dec(F8C, fn, codes)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), fn
        assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), fn
        assert np.array_equal(got.view(np.uint32)[nan] >> 31, (codes[nan] >> 7).astype(np.uint32)), fn


def test_encoding_equals_torchs_clamped_cast(F8C):
    p = E.encode_set()
    assert p[:E.edge_bits().size].tolist() == E.edge_bits().tolist() and p.size % 48 == 0
    got = _enc(F8C, p)
    bad = E.enc_mismatches(got, p)
    assert bad.size == 0, [(hex(int(p[i])), hex(int(got[i])), hex(int(E.enc_cpu(p[i:i + 1])[0]))) for i in bad[:8]]
    # what the contract names one by one
    one = lambda bits: int(_enc(F8C, np.array([bits], np.uint32))[0])
    assert one(0x3a800000) == 0x00 and one(0xba800000) == 0x80          # the tie at 2^-10 goes to 0
    assert one(0x3a800001) == 0x01
    assert one(0x43e80000) == 0x7e and one(0x7f800000) == 0x7e and one(0xff800000) == 0xfe
    assert one(0x7f7fffff) == 0x7e and one(0x80000000) == 0x80
    assert one(0x7fc00000) == 0x7f and one(0xffc00000) == 0xff and one(0xff800001) == 0xff


def test_round_trip_is_the_identity_on_codes(F8C):
    codes = np.arange(256, dtype=np.uint8)
    keep = ~E.nan_code(codes)
    back = _enc(F8C, _dec(F8C, "f8_dec", codes).view(np.uint32))
    assert np.array_equal(back[keep], codes[keep])


def test_the_patterns_reach_every_class():
    """A condition on the INPUTS, against the CPU reference alone: the set every encoding path is
    checked on (here and on the GPU) holds at least 1000 results of each class."""
    got = E.classes(E.encode_set())
    for name in ("normal", "subnormal", "zero", "saturated", "tie", "nan"):
        assert got[name] >= 1000, (name, got)
