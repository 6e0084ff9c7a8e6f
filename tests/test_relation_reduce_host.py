"""The per-destination arithmetic of the per-relation aggregation (euler_amd/csrc/mp_relation.h),
compiled with the host compiler, against the numpy restatement tests/relation_reduce_ref.py.
CPU only; every comparison is bit equality.  Also: the new C-ABI entry is exported and bound."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import relation_reduce_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
f32p, i32p, u32p, i64p = (C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                          C.POINTER(C.c_int64))


@pytest.fixture(scope="module")
def MPR():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libmp_relation_check.so")
    src = os.path.join(HERE, "csrc", "mp_relation_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h) for h in ("mp_relation.h", "mp_weighted.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the host compiler alone, no HIP header; -ffp-contract=off as the library's build
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.mpr_reduce_dest.argtypes = [C.c_int, C.c_int, f32p, C.c_int64, i32p, C.c_int32, C.c_uint32, u32p, i32p,
                                  C.c_int32, C.c_int64, C.c_int64, f32p, i32p, i64p, i32p]
    L.mpr_reduce_dest.restype = C.c_int
    return L


def dest(L, op, lane_cols, x, types, R, b, en, gather=None, perm=None, gstride=1, row_max=0xFFFFFFFF,
         tally=False):
    """-> (out [R, d], counts [R]) and, with tally, (loads per table row, stores per relation)"""
    x = np.ascontiguousarray(x, np.float32)
    types = np.ascontiguousarray(types, np.int32)
    out = np.full((R, x.shape[1]), np.nan, np.float32)
    counts = np.full(R, -7, np.int32)
    loads = np.zeros(x.shape[0], np.int64)
    stores = np.zeros(R, np.int32)
    g = None if gather is None else np.ascontiguousarray(gather, np.int32)
    pm = None if perm is None else np.ascontiguousarray(perm, np.uint32)
    rc = L.mpr_reduce_dest(ref.MODE[op], lane_cols, x.ctypes.data_as(f32p), x.shape[1],
                           g.ctypes.data_as(i32p) if g is not None else None, gstride, row_max,
                           pm.ctypes.data_as(u32p) if pm is not None else None,
                           types.ctypes.data_as(i32p), R, b, en, out.ctypes.data_as(f32p),
                           counts.ctypes.data_as(i32p), loads.ctypes.data_as(i64p), stores.ctypes.data_as(i32p))
    assert rc == 0
    return (out, counts, loads, stores) if tally else (out, counts)


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def table(rng, rows, d):
    return ((rng.random((rows, d)) * 8 - 4) * 10.0 ** rng.integers(-3, 4, (rows, d))).astype(np.float32)


@pytest.mark.parametrize("op", ref.OPS)
@pytest.mark.parametrize("R", [1, 3, 70])
@pytest.mark.parametrize("seg_len", [0, 1, 19, 70])     # empty; one; the 8 / 4 / 1 tails; more than 64 updates
def test_dest_function_equals_the_numpy_loops(MPR, op, R, seg_len):
    rng = np.random.default_rng(1000 * R + seg_len)
    rows, d, e = 96, 16, 96                     # (rows == e: without a gather, update p is row p)
    x = table(rng, rows, d)
    types = rng.integers(-1, R + 1, e).astype(np.int32)           # -1 and R: both invalid values
    gather = rng.integers(0, rows, e).astype(np.int32)
    perm = rng.permutation(e).astype(np.uint32)
    b = 11
    en = b + seg_len
    for lane_cols in (1, 4, 8):
        for g, pm in ((gather, None), (gather, perm), (None, None), (None, perm)):
            pos = np.arange(b, en) if pm is None else pm[b:en].astype(np.int64)
            rws = pos if g is None else g[pos]
            want, want_cnt = ref.reduce_dest(op, x, rws, types[pos], R)
            got, cnt, loads, stores = dest(MPR, op, lane_cols, x, types, R, b, en, g, pm, tally=True)
            assert same(got, want), (lane_cols, g is None, pm is None)
            assert np.array_equal(cnt, want_cnt)
            # every bucket is stored exactly once, every valid update's row loaded exactly once
            assert np.all(stores == 1)
            ok = (types[pos] >= 0) & (types[pos] < R)
            assert np.array_equal(loads, np.bincount(rws[ok], minlength=rows))


def test_one_relation_with_a_long_run_takes_full_batches(MPR):
    """70 updates of one type among 3: 8 full batches of eight, then 4 + 1 + 1"""
    rng = np.random.default_rng(5)
    x = table(rng, 80, 8)
    types = np.full(80, 1, np.int32)
    types[70:] = 2
    for op in ref.OPS:
        for lane_cols in (1, 4, 8):
            got, cnt = dest(MPR, op, lane_cols, x, types, 3, 0, 70)
            want, want_cnt = ref.reduce_dest(op, x, np.arange(70), types[:70], 3)
            assert same(got, want) and np.array_equal(cnt, want_cnt) and list(cnt) == [0, 70, 0]


@pytest.mark.parametrize("m", list(range(1, 13)))
def test_every_bucket_size_up_to_twelve(MPR, m):
    """m updates of relation 0 among others: 8 | 4 | the batch of the 1 .. 3 left, in every mix"""
    rng = np.random.default_rng(40 + m)
    x = table(rng, 40, 8)
    types = np.full(40, 1, np.int32)
    types[rng.choice(40, m, replace=False)] = 0
    for op in ref.OPS:
        for lane_cols in (1, 8):
            got, cnt, loads, _ = dest(MPR, op, lane_cols, x, types, 2, 0, 40, tally=True)
            want, want_cnt = ref.reduce_dest(op, x, np.arange(40), types, 2)
            assert same(got, want) and list(cnt) == [m, 40 - m] and np.all(loads == 1)


def test_int64_ids_are_read_by_their_low_word_and_clamped(MPR):
    rng = np.random.default_rng(3)
    rows, d, e, R = 20, 8, 19, 3
    x = table(rng, rows, d)
    types = rng.integers(0, R, e).astype(np.int32)
    ids = rng.integers(0, rows + 10, e).astype(np.int64)
    ids[3] = -1
    ids[5] += 1 << 33
    want_rows = np.minimum(ids & 0xFFFFFFFF, rows - 1)
    assert want_rows[3] == rows - 1 and want_rows[5] == min(ids[5] - (1 << 33), rows - 1)
    got, cnt = dest(MPR, "add", 4, x, types, R, 0, e, ids.view(np.int32), None, gstride=2, row_max=rows - 1)
    want, want_cnt = ref.reduce_dest("add", x, want_rows, types, R)
    assert same(got, want) and np.array_equal(cnt, want_cnt)


def test_invalid_types_are_left_out_of_sums_and_counts(MPR):
    rng = np.random.default_rng(4)
    x = table(rng, 12, 8)
    types = np.array([0, -1, 2, 3, 0, -1, 3, 1, 2, 0, 5, -2], np.int32)     # R = 3: -1, 3, 5, -2 invalid
    keep = (types >= 0) & (types < 3)
    for op in ref.OPS:
        got, cnt = dest(MPR, op, 4, x, types, 3, 0, 12)
        want, want_cnt = ref.reduce_dest(op, x, np.flatnonzero(keep), types[keep], 3)    # removed by hand
        assert same(got, want) and np.array_equal(cnt, want_cnt) and cnt.sum() == keep.sum()


def test_a_destination_of_invalid_updates_only(MPR):
    x = np.ones((6, 8), np.float32)
    types = np.array([-1, 3, -1, 3, 7, -1], np.int32)
    for op, value in (("add", 0.0), ("max", -1e9), ("mean", 0.0), ("mean_rel", 0.0)):
        for lane_cols in (1, 4, 8):
            got, cnt = dest(MPR, op, lane_cols, x, types, 3, 0, 6)
            assert same(got, np.full((3, 8), value, np.float32)) and not cnt.any()


def test_denominators_of_the_two_means(MPR):
    """3 updates of type 0, 1 of type 2, 1 invalid: mean / fl(4 + 1e-7f), mean_rel / fl(3 + 1e-7f)
    and / fl(1 + 1e-7f)"""
    x =np.array([[3.0] * 4, [5.0] * 4, [7.0] * 4, [11.0] * 4, [13.0] * 4], np.float32)
    types = np.array([0, 2, 0, -1, 0], np.int32)
    f = np.float32
    s0, s2 = f(f(f(3.0) + f(7.0)) + f(13.0)), f(5.0)
    d4, d3, d1 = f(f(4) + f(1e-7)), f(f(3) + f(1e-7)), f(f(1) + f(1e-7))
    got, cnt = dest(MPR, "mean", 4, x, types, 3, 0, 5)
    assert list(cnt) == [3, 0, 1]
    assert same(got[:, 0], np.array([s0 / d4, f(0) / d4, s2 / d4], np.float32))
    got, cnt = dest(MPR, "mean_rel", 4, x, types, 3, 0, 5)
    assert same(got[:, 0], np.array([s0 / d3, f(0), s2 / d1], np.float32))
    assert d1 != f(1) and s2 / d1 != s2                   # (1 + 1e-7f rounds to the float above 1)


def test_reference_restatement_against_a_plain_formulation():
    """the restatement itself: per-bucket loops == masked sums per (destination, relation)"""
    rng = np.random.default_rng(9)
    x = rng.integers(-8, 9, (12, 6)).astype(np.float32)        # small integers: every order is exact
    e, size, R = 60, 7, 3
    gi = rng.integers(0, 12, e)
    dst = rng.integers(-1, size + 2, e)
    ty = rng.integers(-1, R + 1, e)
    out, counts = ref.relation_reduce_ref("add", x, gi, ty, R, dst, size)
    mean, _ = ref.relation_reduce_ref("mean", x, gi, ty, R, dst, size)
    mean_rel, _ = ref.relation_reduce_ref("mean_rel", x, gi, ty, R, dst, size)
    mx, _ = ref.relation_reduce_ref("max", x, gi, ty, R, dst, size)
    for r in range(size):
        n_valid = np.sum((dst == r) & (ty >= 0) & (ty < R))
        for t in range(R):
            sel = (dst == r) & (ty == t)
            assert counts[r, t] == sel.sum()
            assert same(out[r, t], x[gi[sel]].sum(0, dtype=np.float32))
            assert same(mean[r, t], out[r, t] / np.float32(np.float32(n_valid) + np.float32(1e-7)))
            assert same(mean_rel[r, t], out[r, t] / np.float32(np.float32(sel.sum()) + np.float32(1e-7)))
            assert same(mx[r, t], x[gi[sel]].max(0) if sel.any() else np.full(6, -1e9, np.float32))
    assert np.array_equal(ref.segment_dst(3, count=2), [0, 0, 1, 1, 2, 2])
    assert np.array_equal(ref.segment_dst(3, seg_ptr=[0, 2, 2, 3]), [0, 0, 2])


def test_new_entry_is_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    name = "euler_gpu_relation_reduce"
    assert name in _lib.SIGNATURES
    assert hasattr(L, name)
    assert name + "(" in hdr
    assert len(_lib.SIGNATURES[name][1]) == 18


def test_sources_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "$(HERE)mp_relation.h" in mk and "relation_kernels.hip" in mk


def test_ops_are_public():
    from euler_amd import ops
    from euler_amd.euler_ops import mp_ops
    assert mp_ops.relation_reduce is ops.relation_reduce and mp_ops.relation_conv is ops.relation_conv
