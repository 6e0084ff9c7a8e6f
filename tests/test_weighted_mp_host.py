"""The per-row arithmetic of the edge-weighted reduces (euler_amd/csrc/mp_weighted.h), compiled
with the host compiler, against the numpy restatement tests/weighted_mp_ref.py.  CPU only; every
comparison is bit equality.  Also: the new C-ABI entries are exported and bound."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import weighted_mp_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
f32p, i32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
MODE = {"add": 0, "max": 1, "mean": 2}

NEW_SYMBOLS = ["euler_gpu_gather_scatter_w", "euler_gpu_gather_segment_reduce_w",
               "euler_gpu_gather_segment_reduce_ids_w", "euler_gpu_gather_scatter_w_t",
               "euler_gpu_gather_segment_reduce_w_t", "euler_gpu_gather_segment_reduce_ids_w_t",
               "euler_gpu_edge_dot", "euler_gpu_edge_dot_t"]


@pytest.fixture(scope="module")
def MPW():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libmp_weighted_check.so")
    src = os.path.join(HERE, "csrc", "mp_weighted_check.cc")
    deps = [src, os.path.join(ROOT, "euler_amd", "csrc", "mp_weighted.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # -ffp-contract=off: the host build may not fuse the product and the sum either
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.mpw_reduce_row.argtypes = [C.c_int, C.c_int, f32p, C.c_int64, i32p, C.c_int32, C.c_uint32, u32p, f32p,
                                 C.c_int32, C.c_int64, C.c_int64, f32p]
    L.mpw_reduce_row.restype = C.c_int
    return L


def row(L, op, lane_cols, x, w, b, en, gather=None, perm=None, gstride=1, row_max=0xFFFFFFFF):
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    out = np.full(x.shape[1], np.nan, np.float32)
    g = None if gather is None else np.ascontiguousarray(gather, np.int32)
    pm = None if perm is None else np.ascontiguousarray(perm, np.uint32)
    rc = L.mpw_reduce_row(MODE[op], lane_cols, x.ctypes.data_as(f32p), x.shape[1],
                          g.ctypes.data_as(i32p) if g is not None else None, gstride, row_max,
                          pm.ctypes.data_as(u32p) if pm is not None else None,
                          w.ctypes.data_as(f32p), w.shape[1], b, en, out.ctypes.data_as(f32p))
    assert rc == 0
    return out


def same(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("op", ["add", "max", "mean"])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("seg_len", [0, 1, 19])      # empty; one update; the 8 / 4 / 1 tails (8+8+1+1+1)
def test_row_function_equals_the_numpy_loop(MPW, op, heads, seg_len):
    rng = np.random.default_rng(100 * heads + seg_len)
    rows, d, e = 64, 32, 64                       # (rows == e: without a gather, update p is row p)
    x = ((rng.random((rows, d)) * 8 - 4) * 10.0 ** rng.integers(-3, 4, (rows, d))).astype(np.float32)
    w = (rng.random((e, heads)) * 4 - 2).astype(np.float32)
    gather = rng.integers(0, rows, e).astype(np.int32)
    perm = rng.permutation(e).astype(np.uint32)
    b = 11
    en = b + seg_len
    for lane_cols in (1, 4, 8):                   # d / heads = 32 or 8: every lane shape applies
        for g, pm in ((gather, None), (gather, perm), (None, None), (None, perm)):
            pos = np.arange(b, en) if pm is None else pm[b:en].astype(np.int64)
            rws = pos if g is None else g[pos]
            want = ref.reduce_segment(op, x, w, rws, pos)
            got = row(MPW, op, lane_cols, x, w, b, en, g, pm)
            assert same(got, want), (lane_cols, g is None, pm is None)
    if seg_len == 0:
        assert np.all(row(MPW, op, 1, x, w, b, en, gather) == np.float32(-1e9 if op == "max" else 0.0))


def test_int64_ids_are_read_by_their_low_word_and_clamped(MPW):
    rng = np.random.default_rng(3)
    rows, d, e = 20, 8, 19
    x = (rng.random((rows, d)) * 2 - 1).astype(np.float32)
    w = (rng.random((e, 1)) + 0.5).astype(np.float32)
    ids = rng.integers(0, rows + 10, e).astype(np.int64)
    ids[3] = -1
    ids[5] += 1 << 33
    low = (ids & 0xFFFFFFFF).astype(np.int64)
    want_rows = np.minimum(low, rows - 1)
    got = row(MPW, "add", 4, x, w, 0, e, ids.view(np.int32), None, gstride=2, row_max=rows - 1)
    assert same(got, ref.reduce_segment("add", x, w, want_rows, np.arange(e)))


def test_product_and_sum_are_two_roundings_not_an_fma(MPW):
    """x * w = 1 + 2^-11 + 2^-24 exactly; rounded to fp32 it is 1 + 2^-11 (a tie, to even), and
    adding it to acc = -(1 + 2^-11) gives 0.  A fused multiply-add keeps the 2^-24."""
    x = np.float32(1 + 2.0 ** -12)
    w = np.float32(1 + 2.0 ** -12)
    acc = np.float32(-(1 + 2.0 ** -11))
    two_step = np.float32(np.float32(x * w) + acc)
    fused = np.float32(np.float64(x) * np.float64(w) + np.float64(acc))       # exact in float64
    assert two_step == 0 and fused == np.float32(2.0 ** -24) and two_step != fused
    # the segment: first acc's row (weight 1: 0 + acc = acc), then x with weight w
    table = np.array([[acc] * 8, [x] * 8], np.float32)
    wts = np.array([[1.0], [w]], np.float32)
    for lane_cols in (1, 4, 8):
        got = row(MPW, "add", lane_cols, table, wts, 0, 2)
        assert same(got, np.zeros(8, np.float32)), lane_cols
        assert same(got, ref.reduce_segment("add", table, wts, [0, 1], [0, 1]))


def test_reference_restatement_against_plain_numpy():
    """the restatement itself: whole-op form == per-destination loops, dst >= size left out"""
    rng = np.random.default_rng(9)
    x = rng.random((12, 6)).astype(np.float32)
    gi = rng.integers(0, 12, 40)
    dst = rng.integers(0, 9, 40)
    w = rng.random((40, 2)).astype(np.float32)
    out = ref.gather_scatter_ref("add", x, gi, dst, 7, w)
    msg = (x[gi] * np.repeat(w, 3, axis=1)).astype(np.float32)
    for r in range(7):
        acc = np.zeros(6, np.float32)
        for p in np.flatnonzero(dst == r):
            acc = (acc + msg[p]).astype(np.float32)
        assert same(out[r], acc)
    assert np.array_equal(ref.segment_dst(3, count=2), [0, 0, 1, 1, 2, 2])
    assert np.array_equal(ref.segment_dst(3, seg_ptr=[0, 2, 2, 3]), [0, 0, 2])


def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
        assert name + "(" in hdr, name


def test_header_is_a_makefile_dependency():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "mp_weighted.h" in mk and "edge_dot_kernels.hip" in mk
