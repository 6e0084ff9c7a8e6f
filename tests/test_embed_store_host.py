"""The shared pieces of the in-place embedding stores (euler_amd/csrc/embed_store.h), compiled with
the host compiler and driven over whole calls, against the numpy restatement
tests/embed_store_ref.py: bit equality of update / add / take.  Also: the restatement can tell
orders apart, the fp32 chain of add stays within its derived bound of the float64 sum, and the new
C-ABI entries are exported and bound.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import embed_store_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CODE = {"f32": 0, "bf16": 1, "f16": 2}
DIMS = [1, 3, 4, 8, 12, 64, 130, 260]
SIZES = [0, 1, 63, 64, 65, 1000]
ROWS = [1, 7, 50]


@pytest.fixture(scope="module")
def ES():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libembed_store_check.so")
    src = os.path.join(HERE, "csrc", "embed_store_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h) for h in ("embed_store.h", "mp_weighted.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the host compiler alone, no HIP header; -ffp-contract=off as the library's build
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.es_call.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                          C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_int32]
    L.es_call.restype = C.c_int
    L.es_key_bits.argtypes = [C.c_int64]
    L.es_chunk_width.argtypes = [C.c_int64, C.c_uint64, C.c_int, C.c_uint64, C.c_int]
    return L


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host(L, op, table, dt, ids, other, odt, m=0, row_index=None, count=0, clear=False):
    """one call of the host build on a COPY of table -> the table afterwards (`other` is written by take)"""
    t = np.array(table, copy=True)
    ids = np.ascontiguousarray(ids, np.int64)
    ri = None if row_index is None else np.ascontiguousarray(row_index, np.int32)
    rc = L.es_call(op, ptr(t), CODE[dt], t.shape[0], t.shape[1], ptr(ids), len(ids), ptr(other), CODE[odt], m,
                   ptr(ri), count, int(clear))
    assert rc == 0
    return t


def stored(rng, shape, dt):
    """order-sensitive values stored as dt"""
    return ref.narrow(ref.sensitive_values(rng, shape), dt)


def check_all(L, rng, rows, d, ids, dt, vdt, row_index=None, count=0):
    """update, add, take and take + clear of the host build == the restatement"""
    e = len(ids)
    m = e // count if count else (9 if row_index is not None else e)
    table = stored(rng, (rows, d), dt)
    values = np.ascontiguousarray(stored(rng, (m, d), vdt))
    tag = (rows, d, e, dt, vdt, count, row_index is not None)
    assert ref.same(host(L, 0, table, dt, ids, values, vdt, m, row_index, count),
                    ref.update(table, dt, ids, values, vdt, row_index, count)), ("update",) + tag
    assert ref.same(host(L, 1, table, dt, ids, values, vdt, m, row_index, count),
                    ref.add(table, dt, ids, values, vdt, row_index, count)), ("add",) + tag
    for clear in (False, True):
        out = np.full((e, d), 0x7fc1 if vdt != "f32" else np.nan, np.float32 if vdt == "f32" else np.uint16)
        after = host(L, 2, table, dt, ids, out, vdt, clear=clear)
        want_out, want_after = ref.take(table, dt, ids, clear, vdt)
        assert ref.same(out, want_out) and ref.same(after, want_after), ("take", clear) + tag


@pytest.mark.parametrize("d", DIMS)
def test_host_build_equals_the_restatement(ES, d):
    """every E x rows, the id patterns rotating, ids that name no row mixed in; table fp32 / bf16 /
    fp16 x values fp32 / the table's dtype"""
    rng = np.random.default_rng(100 + d)
    n = 0
    for e in SIZES:
        for rows in ROWS:
            for dt in ref.DTYPES:
                ids = ref.id_pattern(rng, ref.PATTERNS[n % len(ref.PATTERNS)], rows, e)
                if n % 2:
                    ids = ref.with_bad_ids(ids, rows)
                vdt = dt if n % 3 else "f32"
                n += 1
                check_all(ES, rng, rows, d, ids, dt, vdt)


@pytest.mark.parametrize("dt", ref.DTYPES)
def test_count_and_row_index_forms(ES, dt):
    """the count and row_index forms == the plain form on the materialised block; a row_index
    entry outside [0, M) removes its occurrence"""
    rng = np.random.default_rng(7)
    rows, d, count = 50, 12, 5
    ids = ref.with_bad_ids(ref.id_pattern(rng, "hubs", rows, 60 * count), rows, every=11)
    check_all(ES, rng, rows, d, ids, dt, "f32", count=count)
    ri = rng.integers(0, 9, len(ids)).astype(np.int32)
    ri[[3, 40, 41]] = [-1, 9, 2 ** 31 - 1]
    check_all(ES, rng, rows, d, ids, dt, dt, row_index=ri)
    table, values = stored(rng, (rows, d), dt), stored(rng, (9, d), dt)
    block, keep = ref.materialise(values, 9, row_index=ri)
    assert not keep[3] and not keep[40] and not keep[41] and keep.sum() == len(ids) - 3
    plain_ids = np.where(keep, ids, -1)
    for fn in (ref.update, ref.add):
        assert ref.same(fn(table, dt, ids, values, dt, row_index=ri), fn(table, dt, plain_ids, block, dt))
    v60 = stored(rng, (60, d), dt)
    block, keep = ref.materialise(v60, 60, count=count)
    assert keep.all() and ref.same(block[7], v60[1])
    for fn in (ref.update, ref.add):
        assert ref.same(fn(table, dt, ids, v60, dt, count=count), fn(table, dt, ids, block, dt))


def test_the_restatement_tells_orders_apart():
    """300 occurrences of one id: adding in reversed position order changes bits in every column,
    and the first and the last duplicate carry different rows (update's winner is observable)"""
    rng = np.random.default_rng(5)
    table = np.zeros((7, 4), np.float32)
    ids = ref.id_pattern(rng, "equal", 7, 300)
    values = ref.sensitive_values(rng, (300, 4))
    fwd, rev = ref.add(table, "f32", ids, values, "f32"), ref.add(table, "f32", ids, values, "f32", reverse=True)
    assert np.all(fwd[3].view(np.uint32) != rev[3].view(np.uint32))
    assert not ref.same(values[0], values[-1])
    assert ref.same(ref.update(table, "f32", ids, values, "f32")[3], values[-1])


def test_special_values_and_untouched_rows(ES):
    """same-dtype update copies -0.0 and a NaN payload; rows no id names keep their bits"""
    for dt, neg0, nan in (("f32", 0x80000000, 0x7fc12345), ("bf16", 0x8000, 0x7fc5), ("f16", 0x8000, 0x7e05)):
        view = np.uint32 if dt == "f32" else np.uint16
        table = np.full((7, 3), nan, view).view(np.float32 if dt == "f32" else np.uint16)
        values = np.array([[neg0, nan, 1]] * 2, view).view(table.dtype)
        ids = np.array([2, -1], np.int64)
        got = host(ES, 0, table, dt, ids, values, dt, 2)
        assert ref.same(got, ref.update(table, dt, ids, values, dt))
        assert got.view(view)[2].tolist() == [neg0, nan, 1] and np.all(got.view(view)[[0, 1, 3, 4, 5, 6]] == nan)


def test_key_bits_and_chunk_width(ES):
    for rows, bits in ((1, 1), (2, 2), (3, 2), (4, 3), (7, 3), (8, 4), (2 ** 31, 32), (10 ** 8, 27)):
        assert ES.es_key_bits(rows) == bits and (rows >> bits) == 0
    assert ES.es_chunk_width(64, 32, 4, 64, 4) == 8 and ES.es_chunk_width(12, 32, 4, 64, 4) == 4
    assert ES.es_chunk_width(64, 32, 4, 68, 4) == 1 and ES.es_chunk_width(130, 32, 4, 64, 4) == 1
    assert ES.es_chunk_width(64, 8, 2, 16, 2) == 4 and ES.es_chunk_width(64, 8, 2, 8, 4) == 1
    assert ES.es_chunk_width(64, 34, 2, 16, 2) == 1


def test_add_chain_within_the_derived_bound_of_float64(capsys):
    """|fp32 chain - float64 sum| <= gamma(L + 1) * sum |terms|, u = 2^-24, no margin, per segment
    and column: each of the L adds is correctly rounded, so the chain carries at most L relative
    errors of u on every partial sum (Higham, Accuracy and Stability, eq. 4.4)"""
    worst = 0.0
    for seed, (rows, e, name) in enumerate(((7, 300, "equal"), (50, 1000, "hubs"), (50, 1000, "random"), (7, 65, "sorted"))):
        rng = np.random.default_rng(40 + seed)
        table = ref.sensitive_values(rng, (rows, 12))
        ids = ref.with_bad_ids(ref.id_pattern(rng, name, rows, e), rows, every=13)
        err, bound = ref.add_chain_error(table, ids, ref.sensitive_values(rng, (e, 12)))
        assert np.all(err <= bound), (name, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    with capsys.disabled():
        print("\n[embedding_add] worst error / bound = %.4f" % worst)
    assert 0 < worst <= 1


def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name, n_args in (("euler_gpu_store_update", 12), ("euler_gpu_store_add", 12), ("euler_gpu_store_take", 10)):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert name + "(" in hdr
        assert len(_lib.SIGNATURES[name][1]) == n_args


def test_sources_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "$(HERE)embed_store.h" in mk and "embed_store_kernels.hip" in mk


def test_ops_are_public():
    from euler_amd import ops
    assert callable(ops.embedding_update) and callable(ops.embedding_add) and callable(ops.embedding_take)
