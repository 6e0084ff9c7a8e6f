"""The arithmetic of the GCN-normalised aggregation (euler_amd/csrc/mp_gcn.h), compiled with the
host compiler, against the numpy restatement tests/gcn_norm_ref.py.  CPU only; comparisons are bit
equality unless a bound is stated.  Also: the new C-ABI entries are exported and bound."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gcn_norm_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
f32p, i32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
MODE = {"add": 0, "mean": 2}
U = 2.0 ** -24

NEW_SYMBOLS = ["euler_gpu_gcn_norm", "euler_gpu_gather_reduce_norm_t"]


@pytest.fixture(scope="module")
def GCN():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libmp_gcn_check.so")
    src = os.path.join(HERE, "csrc", "mp_gcn_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h) for h in ("mp_gcn.h", "mp_weighted.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # -ffp-contract=off: the host build may not fuse a product and a sum either
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.gcn_norm_of.argtypes = [i32p, C.c_int64, f32p]
    L.gcn_norm_of.restype = None
    L.gcn_degrees.argtypes = [i32p, i32p, C.c_int64, C.c_int32, C.c_int32, i32p, i32p]
    L.gcn_degrees.restype = None
    L.gcn_reduce_row.argtypes = [C.c_int, C.c_int, f32p, C.c_int64, C.c_int64, i32p, u32p, C.c_float, f32p,
                                 C.c_int64, C.c_int64, f32p, C.c_float, C.c_float, f32p]
    L.gcn_reduce_row.restype = C.c_int
    return L


def row(L, op, lane_cols, x, gather, nd, norm_src, b, en, perm=None, root=None, a=1.0, rb=1.0):
    x = np.ascontiguousarray(x, np.float32)
    g = np.ascontiguousarray(gather, np.int32)
    ns = np.ascontiguousarray(norm_src, np.float32)
    pm = None if perm is None else np.ascontiguousarray(perm, np.uint32)
    rt = None if root is None else np.ascontiguousarray(root, np.float32)
    out = np.full(x.shape[1], np.nan, np.float32)
    rc = L.gcn_reduce_row(MODE[op], lane_cols, x.ctypes.data_as(f32p), x.shape[1], x.shape[0],
                          g.ctypes.data_as(i32p), pm.ctypes.data_as(u32p) if pm is not None else None,
                          float(nd), ns.ctypes.data_as(f32p), b, en,
                          rt.ctypes.data_as(f32p) if rt is not None else None, float(a), float(rb),
                          out.ctypes.data_as(f32p))
    assert rc == 0
    return out


def same(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def norm_of_host(L, deg):
    deg = np.ascontiguousarray(deg, np.int32)
    out = np.empty(deg.size, np.float32)
    L.gcn_norm_of(deg.ctypes.data_as(i32p), deg.size, out.ctypes.data_as(f32p))
    return out


@pytest.mark.parametrize("op", ["add", "mean"])
@pytest.mark.parametrize("seg_len", [0, 1, 3, 4, 7, 8, 9, 12, 13, 17])     # the batch ladder 8 / 4 / 1
def test_row_function_equals_the_numpy_loop(GCN, op, seg_len):
    rng = np.random.default_rng(1000 + seg_len)
    rows, d, e = 37, 12, 64
    x = ((rng.random((rows, d)) * 8 - 4) * 10.0 ** rng.integers(-3, 4, (rows, d))).astype(np.float32)
    norm_src = ref.norm_of(rng.integers(0, 5000, rows))
    nd = ref.norm_of(np.array([max(seg_len, 1)]))[0]
    gather = rng.integers(0, rows, e).astype(np.int32)
    gather[13] = -1                                # out of range: contributes nothing
    gather[16] = rows
    perm = rng.permutation(e).astype(np.uint32)
    root = (rng.random(d) * 6 - 3).astype(np.float32)
    b, en = 11, 11 + seg_len
    for lane_cols in (1, 4):
        for pm in (None, perm):
            pos = np.arange(b, en) if pm is None else pm[b:en].astype(np.int64)
            want = ref.reduce_segment(op, x, gather[pos], nd, norm_src)
            assert same(row(GCN, op, lane_cols, x, gather, nd, norm_src, b, en, pm), want), (lane_cols, pm is None)
            for a, rb in ((np.float32(1 - 0.1), np.float32(0.1)), (1.0, 1.0)):
                got = row(GCN, op, lane_cols, x, gather, nd, norm_src, b, en, pm, root, a, rb)
                assert same(got, ref.epilogue(want, root, a, rb)), (lane_cols, a)
    if seg_len == 0:
        assert same(row(GCN, op, 1, x, gather, nd, norm_src, b, en), np.zeros(d, np.float32))


def test_out_of_range_gather_leaves_every_bit_alone(GCN):
    """weight 0 and a clamped row: the bits of the reduce without that update, -0 rows included"""
    rng = np.random.default_rng(5)
    x = (rng.random((9, 8)) - 0.5).astype(np.float32)
    x[8] = -3.0                                    # the last row, which a clamped index reads
    norm_src = ref.norm_of(np.arange(1, 10))
    with_bad = np.array([-1, 2, 9, 5, 1 << 30, 7], np.int32)
    without = np.array([2, 5, 7], np.int32)
    for lane_cols in (1, 4):
        a = row(GCN, "add", lane_cols, x, with_bad, 0.5, norm_src, 0, 6)
        assert same(a, row(GCN, "add", lane_cols, x, without, 0.5, norm_src, 0, 3))
    only_bad = row(GCN, "add", 1, x, np.array([-1, 9], np.int32), 0.5, norm_src, 0, 2)
    assert same(only_bad, np.zeros(8, np.float32))          # +0, not the -0 of -3 * 0


def test_product_and_sum_are_two_roundings_not_an_fma(GCN):
    """x * w = 1 + 2^-11 + 2^-24 exactly; rounded to fp32 it is 1 + 2^-11 (a tie, to even), and
    adding it to acc = -(1 + 2^-11) gives 0.  A fused multiply-add keeps the 2^-24."""
    x = np.float32(1 + 2.0 ** -12)
    w = np.float32(1 + 2.0 ** -12)
    acc = np.float32(-(1 + 2.0 ** -11))
    two_step = np.float32(np.float32(x * w) + acc)
    fused = np.float32(np.float64(x) * np.float64(w) + np.float64(acc))       # exact in float64
    assert two_step == 0 and fused == np.float32(2.0 ** -24) and two_step != fused
    # the segment: first acc's row (norm 1: 0 + acc = acc), then x with norm_src = w; nd = 1
    table = np.array([[acc] * 4, [x] * 4], np.float32)
    norm_src = np.array([1.0, w], np.float32)
    for lane_cols in (1, 4):
        got = row(GCN, "add", lane_cols, table, [0, 1], 1.0, norm_src, 0, 2)
        assert same(got, np.zeros(4, np.float32)), lane_cols
        assert same(got, ref.reduce_segment("add", table, [0, 1], 1.0, norm_src))


def test_norm_is_one_over_sqrt_and_zero_at_degree_zero(GCN):
    import torch
    deg = np.arange(0, 4097)
    want = ref.norm_of(deg)
    assert want[0] == 0 and np.all(np.isfinite(want))
    assert same(norm_of_host(GCN, deg), want)
    t = (torch.arange(1, 4097, dtype=torch.float32) ** -0.5).numpy()          # torch-CPU deg ** -0.5
    assert same(want[1:], t)
    big = np.array([70000, 200000, (1 << 24) - 1, 1 << 24], np.int64)
    assert same(norm_of_host(GCN, big), ref.norm_of(big))
    assert same(norm_of_host(GCN, [-5]), np.zeros(1, np.float32))


def test_out_of_range_keys_change_no_degree(GCN):
    n_dst, n_src = 5, 7
    dst = np.array([0, 1, -1, 5, 2, 2, 4, 2 ** 31 - 1, 3, 0], np.int32)
    src = np.array([6, 7, 0, 1, -1, 3, 3, 2, 2 ** 31 - 1, 6], np.int32)
    dd, ds = ref.degrees(dst, src, n_dst, n_src)
    assert dd.tolist() == [2, 0, 1, 0, 1] and ds.tolist() == [0, 0, 0, 2, 0, 0, 2]
    gd, gs = np.zeros(n_dst, np.int32), np.zeros(n_src, np.int32)
    GCN.gcn_degrees(dst.ctypes.data_as(i32p), src.ctypes.data_as(i32p), dst.size, n_dst, n_src,
                    gd.ctypes.data_as(i32p), gs.ctypes.data_as(i32p))
    assert np.array_equal(gd, dd) and np.array_equal(gs, ds)
    nd, ns = ref.gcn_norm(dst, src, n_dst, n_src)
    assert same(nd, ref.norm_of(dd)) and same(ns, ref.norm_of(ds))


@pytest.mark.parametrize("op", ["add", "mean"])
def test_restatement_against_float64(op):
    """|out - ref| <= gamma_(n + 5) * sum_p |w_p x_p| (mean: one more rounding): two roundings per
    norm, one for their product, one for the message, n - 1 for the sum"""
    rng = np.random.default_rng(17)
    n_dst, n_src, e, d = 23, 41, 400, 5
    x = ((rng.random((n_src, d)) * 2 - 1) * 10.0 ** rng.integers(-2, 3, (n_src, d))).astype(np.float32)
    dst = rng.integers(-1, n_dst + 1, e)
    src = rng.integers(-1, n_src + 1, e)
    nd, ns = ref.gcn_norm(dst, src, n_dst, n_src)
    got = ref.gcn_aggregate(op, x, dst, src, n_dst, nd, ns).astype(np.float64)
    want, scale, lens = ref.exact_f64(op, x, dst, src, n_dst, n_src)
    k = lens + 5 + (op == "mean")
    gamma = (k * U / (1 - k * U))[:, None]
    assert np.all(np.abs(got - want) <= gamma * scale)
    assert np.any(got != want)


def test_whole_op_restatement_equals_per_destination_loops():
    rng = np.random.default_rng(9)
    x = rng.random((12, 6)).astype(np.float32)
    src = rng.integers(0, 12, 40)
    dst = rng.integers(0, 9, 40)
    nd, ns = ref.gcn_norm(dst, src, 7, 12)
    out = ref.gcn_aggregate("add", x, dst, src, 7, nd, ns)
    w = (nd[np.minimum(dst, 6)] * ns[src]).astype(np.float32)
    msg = (x[src] * w[:, None]).astype(np.float32)
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


def test_new_files_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "mp_gcn.h" in mk and "gcn_norm_kernels.hip" in mk
