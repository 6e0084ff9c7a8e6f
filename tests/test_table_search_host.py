"""The table search (euler_amd/csrc/table_search.h) compiled with the host compiler, over whole
calls, against the numpy restatement tests/table_search_ref.py: bit equality of the scores, the
rows and the ranks; the order rule on tie-heavy tables; the fills; exclude and target in and out of
range; the restatement within the derived bound of float64; the C-ABI entries exported and bound,
and every rule of their argument ladder (driven through the C ABI in a child process that sees no
GPU: every row stops in front of the first HIP call).  CPU only.

A NaN score is compared as "NaN on both sides": its sign and payload are the hardware's."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import table_search_ref as ref                                            # noqa: E402
from table_search_ref import DIMS, DTYPES, ITEM, KS, METRICS, queries_for, same_scores, tie_table, to_dtype   # noqa: E402,F401

f32p, i64p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
F = np.float32


@pytest.fixture(scope="module")
def TS():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libtable_search_check.so")
    src = os.path.join(HERE, "csrc", "table_search_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h)
                    for h in ("table_search.h", "kg_score.h", "mp_weighted.h", "sparse_embed.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the host compiler alone, no HIP header; -ffp-contract=off as the library's build
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.ts_chunk_width.argtypes = [C.c_int64, C.c_uint64, C.c_int32, C.c_uint64, C.c_int32]
    L.ts_chunk_width.restype = C.c_int
    L.ts_slabs.argtypes = [C.c_int64, C.c_int64]
    L.ts_slabs.restype = C.c_int64
    L.ts_wave_queries.argtypes = [C.c_int64, i32p]
    L.ts_wave_queries.restype = C.c_int32
    L.ts_search.argtypes = [C.c_int32, C.c_int32, f32p, C.c_int64, C.c_int64, f32p, C.c_int64, C.c_int64, i64p, i64p,
                            C.c_int32, f32p, i64p, i32p]
    L.ts_search.restype = C.c_int
    return L


def placed(a, shift=0):
    """a copy of fp32 `a` whose first element lies `shift` elements past a 16-byte boundary"""
    buf = np.empty(a.size + 8, F)
    at = (-(buf.ctypes.data // 4)) % 4 + shift
    out = buf[at:at + a.size].reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 16 == 4 * shift % 16
    return out


def fp(a):
    return a.ctypes.data_as(f32p) if a is not None else None


def ip_(a):
    return a.ctypes.data_as(i64p) if a is not None else None


def host_topk(L, table, queries, k, metric, v, exclude=None, backwards=False):
    q, (n, d) = len(queries), table.shape
    table, queries = np.ascontiguousarray(table, F), np.ascontiguousarray(queries, F)
    exclude = None if exclude is None else np.ascontiguousarray(exclude, np.int64)
    s, r = np.full((q, k), 7, F), np.full((q, k), -7, np.int64)
    assert L.ts_search(v, ref.METRIC[metric], fp(table), n, d, fp(queries), q, k, None, ip_(exclude), int(backwards),
                       fp(s), ip_(r), None) == 0
    return s, r


def host_rank(L, table, queries, target, metric, v, exclude=None):
    q, (n, d) = len(queries), table.shape
    table, queries = np.ascontiguousarray(table, F), np.ascontiguousarray(queries, F)
    target = np.ascontiguousarray(target, np.int64)
    exclude = None if exclude is None else np.ascontiguousarray(exclude, np.int64)
    out = np.full(q, -7, np.int32)
    assert L.ts_search(v, ref.METRIC[metric], fp(table), n, d, fp(queries), q, 1, ip_(target), ip_(exclude), 0,
                       None, None, out.ctypes.data_as(i32p)) == 0
    return out


def check_case(L, table, queries, metric, v, ks, ns, own, tag):
    """top-k for every (k, N) and the rank at the largest N: host build == restatement"""
    s_all = ref.scores(table, queries, metric, v)
    q = len(queries)
    for n in ns:
        t, s = table[:n], s_all[:, :n]
        excludes = [None, np.concatenate([own, np.full(q - len(own), -1)]) % max(n, 1),
                    np.array([-1, n, n + 5, 1 << 33, -(1 << 40), n][:q] + [n] * max(0, q - 6), np.int64)]
        for k in ks:
            for ei, exc in enumerate(excludes if (k in (3, 10) or n <= 3) else excludes[:1]):
                got = host_topk(L, t, queries, k, metric, v, exc)
                want = ref.topk(t, queries, k, metric, v, exc, s=s)
                assert same_scores(got[0], want[0]), tag + (n, k, ei, "scores")
                assert np.array_equal(got[1], want[1]), tag + (n, k, ei, "rows")
                cand = n - (np.zeros(q, np.int64) if exc is None else ((exc >= 0) & (exc < n)).astype(np.int64))
                assert np.array_equal((got[1] >= 0).sum(1), np.minimum(k, cand)), tag + (n, k, ei, "count")
                assert np.all(got[0][got[1] < 0] == ref.fill(metric)), tag + (n, k, ei, "fill")
        rng = np.random.default_rng(n)
        target = rng.integers(0, max(n, 1), q)
        target[-1] = n + 2                                               # names no row
        if q > 1:
            target[-2] = -1
        for exc in excludes:
            got = host_rank(L, t, queries, target, metric, v, exc)
            want = ref.rank(t, queries, target, metric, v, exc, s=s)
            assert got.dtype == want.dtype == np.int32 and np.array_equal(got, want), tag + (n, "rank")
            assert got[-1] == -1


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_host_build_equals_the_restatement(TS, d, metric):
    """all nine dtype pairs; k in KS x N in {1, k - 1, k, k + 1, 300}; V = 1 / 4 / 8 by d, at
    d = 130 a lane with more than one chunk; tie-heavy tables with NaN and inf rows"""
    for it, dtt in enumerate(DTYPES):
        for iq, dq in enumerate(DTYPES):
            rng = np.random.default_rng(1000 * d + 10 * it + iq)
            table = tie_table(rng, 300, d, dtt)
            queries, own = queries_for(rng, table, dq)
            v = ref.chunk_width(d, 0, ITEM[dtt], 0, ITEM[dq])
            assert v == TS.ts_chunk_width(d, 0, dtt == "f32", 0, dq == "f32") == (8 if d % 8 == 0 else 4 if d % 4 == 0 else 1)
            ks = KS if dtt == dq else (10,)
            ns = sorted({1, 300} | {n for k in ks for n in (k - 1, k, k + 1) if n >= 1})
            check_case(TS, table, queries, metric, v, ks, ns, own, (d, metric, dtt, dq))


@pytest.mark.parametrize("metric", METRICS)
def test_empty_table_and_no_queries(TS, metric):
    table, queries = np.zeros((0, 8), F), np.ones((3, 8), F)
    s, r = host_topk(TS, table, queries, 4, metric, 8)
    assert np.all(r == -1) and np.all(s == ref.fill(metric)) and np.isinf(ref.fill(metric))
    want = ref.topk(table, queries, 4, metric, 8)
    assert same_scores(s, want[0]) and np.array_equal(r, want[1])
    assert host_rank(TS, table, queries, [0, 1, -1], metric, 8).tolist() == [-1, -1, -1]
    assert ref.rank(table, queries, [0, 1, -1], metric, 8).tolist() == [-1, -1, -1]
    s, r = host_topk(TS, np.ones((5, 8), F), np.zeros((0, 8), F), 4, metric, 8)
    assert s.shape == (0, 4) and r.shape == (0, 4)


@pytest.mark.parametrize("dq", DTYPES)
@pytest.mark.parametrize("dtt", DTYPES)
def test_chunk_width_follows_the_tables_alignment(TS, dtt, dq):
    """the rule of KgChunkWidth: 16-byte starts for V = 8, 16 (fp32) / 8 (16-bit) for V = 4"""
    for d in DIMS + (16, 20):
        for at in (0, 2, 4, 8, 16):
            for aq in (0, 4, 8):
                if at % ITEM[dtt] or aq % ITEM[dq]:
                    continue
                assert TS.ts_chunk_width(d, 4096 + at, dtt == "f32", 8192 + aq, dq == "f32") == \
                    ref.chunk_width(d, 4096 + at, ITEM[dtt], 8192 + aq, ITEM[dq]), (d, at, aq)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [8, 64, 136])
def test_table_view_off_a_16_byte_boundary(TS, d, metric):
    """an fp32 table view that starts 4 bytes past a 16-byte boundary takes V = 1: other sums,
    other bits than the aligned table's V = 8 - and both agree with the restatement"""
    rng = np.random.default_rng(50 + d)
    base = tie_table(rng, 120, d, "f32")
    queries, own = queries_for(rng, base, "f32")
    queries = placed(queries)
    off = placed(base, shift=1)
    v = TS.ts_chunk_width(d, off.ctypes.data, 1, queries.ctypes.data, 1)
    assert v == 1 == ref.chunk_width(d, off.ctypes.data, 4, queries.ctypes.data, 4)
    assert TS.ts_chunk_width(d, placed(base).ctypes.data, 1, queries.ctypes.data, 1) == 8
    check_case(TS, off, queries, metric, 1, (3, 10), (120,), own, (d, metric, "off"))
    check_case(TS, base, queries, metric, 8, (3, 10), (120,), own, (d, metric, "on"))
    rnd = (rng.standard_normal((200, d)) * 3).astype(F)
    assert not same_scores(ref.scores(rnd, rnd[:4], metric, 1), ref.scores(rnd, rnd[:4], metric, 8))


@pytest.mark.parametrize("metric", METRICS)
def test_result_does_not_depend_on_the_visiting_order(TS, metric):
    """the host build visiting rows first-to-last and last-to-first returns the same lists; a
    selection that breaks ties by visiting order (a stable sort of the rows as visited backwards)
    differs from the restatement on the tie-heavy table and agrees where the scores are distinct"""
    rng = np.random.default_rng(3)
    d, n, k = 8, 300, 17
    table = tie_table(rng, n, d, "f32")
    queries, _ = queries_for(rng, table, "f32")
    fwd = host_topk(TS, table, queries, k, metric, 8)
    bwd = host_topk(TS, table, queries, k, metric, 8, backwards=True)
    assert same_scores(fwd[0], bwd[0]) and np.array_equal(fwd[1], bwd[1])
    want = ref.topk(table, queries, k, metric, 8)
    assert np.array_equal(fwd[1], want[1])

    def by_visit(s):
        with np.errstate(invalid="ignore"):
            key = np.where(np.isnan(s), np.inf, -s if ref.larger_is_better(metric) else s)
        back = key[::-1]
        return (len(s) - 1 - np.argsort(back, kind="stable"))[:k]

    s = ref.scores(table, queries, metric, 8)
    naive = np.stack([by_visit(s[i]) for i in range(len(queries))])
    assert not np.array_equal(naive, want[1])
    ties = [i for i in range(len(queries)) if len(np.unique(s[i][want[1][i]])) < k]
    assert ties, "the table must make equal scores among the best k"
    for i in ties:                                       # among equal scores the lower row comes first
        rows, sc = want[1][i], s[i][want[1][i]]
        eq = (sc[1:] == sc[:-1]) | (np.isnan(sc[1:]) & np.isnan(sc[:-1]))
        assert np.all(rows[1:][eq] > rows[:-1][eq])
    distinct = rng.standard_normal((n, d)).astype(F)
    s2 = ref.scores(distinct, queries[-2:], metric, 8)
    assert all(len(np.unique(x)) == n for x in s2)
    naive2 = np.stack([by_visit(x) for x in s2])
    assert np.array_equal(naive2, ref.topk(distinct, queries[-2:], k, metric, 8)[1])


@pytest.mark.parametrize("metric", METRICS)
def test_order_rule_on_planted_scores(metric):
    """NaN after every number, +0 == -0, two NaNs equal: by row; the fills past the candidates"""
    best, worse = (F(2), F(1)) if ref.larger_is_better(metric) else (F(1), F(2))
    s = np.array([np.nan, worse, F(0.0), best, F(-0.0), np.nan, best, worse], F)
    assert ref.order(s, metric).tolist() == ([3, 6, 1, 7, 2, 4, 0, 5] if ref.larger_is_better(metric)
                                             else [2, 4, 3, 6, 1, 7, 0, 5])
    table, queries = np.zeros((8, 1), F), np.zeros((1, 1), F)
    sc, rows = ref.topk(table, queries, 10, metric, 1, exclude=[6], s=s[None, :])
    assert rows[0, 7:].tolist() == [-1, -1, -1] and np.all(sc[0, 7:] == ref.fill(metric)) and 6 not in rows[0]
    # the rank: ties go against the target, NaN never counts, nothing counts against a NaN target
    got = ref.rank(table, np.zeros((4, 1), F), [3, 1, 0, 2], metric, 1, exclude=[-1, 7, -1, 9], s=np.stack([s] * 4))
    # (the last target scores +0: row 4's -0 ties with it, then every row that beats 0)
    assert got.tolist() == ([1, 2, 0, 5] if ref.larger_is_better(metric) else [3, 4, 0, 1])


@pytest.mark.parametrize("metric", METRICS)
def test_rank_agrees_with_the_position_in_topk(TS, metric):
    """the target's position in the full list is <= its rank, with equality where its score is
    unique (NaN targets left out: nothing is counted against them)"""
    rng = np.random.default_rng(9)
    table = tie_table(rng, 60, 8, "f32")
    queries, _ = queries_for(rng, table, "f32", q=8)
    _, rows = host_topk(TS, table, queries, 64, metric, 8)
    s = ref.scores(table, queries, metric, 8)
    target = np.array([rows[i][p] for i, p in enumerate([0, 3, 10, 20, 30, 41, 50, 55])])
    rank = host_rank(TS, table, queries, target, metric, 8)
    seen_tie = seen_unique = False
    for i, t in enumerate(target):
        if np.isnan(s[i][t]):
            continue
        pos = rows[i].tolist().index(t)
        unique = np.count_nonzero(s[i] == s[i][t]) == 1
        assert pos <= rank[i] and (not unique or pos == rank[i]), (i, pos, rank[i])
        seen_tie, seen_unique = seen_tie or not unique, seen_unique or unique
    assert seen_tie and seen_unique


def test_restatement_within_the_derived_bound_of_float64(capsys):
    """|fp32 restatement - float64| <= the bound written out in table_search_ref.scores64 (from d,
    u = 2^-24 and the sum of the magnitudes of the terms), no margin; rows uniform in [-1, 1]"""
    worst = {}
    for d in DIMS:
        rng = np.random.default_rng(400 + d)
        table = (rng.random((200, d)) * 2 - 1).astype(F)
        queries = (rng.random((5, d)) * 2 - 1).astype(F)
        for metric in METRICS:
            exact, bound = ref.scores64(table, queries, metric)
            for v in {1, ref.chunk_width(d, 0, 4, 0, 4)}:
                err = np.abs(ref.scores(table, queries, metric, v).astype(np.float64) - exact)
                assert np.all(err <= bound), (d, metric, v, float((err / np.maximum(bound, 1e-300)).max()))
                worst[metric] = max(worst.get(metric, 0.0), float((err / np.maximum(bound, 1e-300)).max()))
    with capsys.disabled():
        print("\n[table_search] worst error / bound: " + ", ".join("%s %.4f" % kv for kv in sorted(worst.items())))
    assert all(0 < w <= 1 for w in worst.values())


def test_launch_shape_restated(TS):
    """slabs and queries a wave: the header's functions == the restatement the GPU tests size by"""
    staged = C.c_int32(0)
    for d in (1, 8, 128, 384, 385, 768, 3072, 3073, 100000):
        qw = TS.ts_wave_queries(d, C.byref(staged))
        assert (qw, bool(staged.value)) == ref.wave_queries(d), d
    for n in (0, 1, 1023, 1024, 1025, 3072, 3073, 10 ** 7):
        for tiles in (1, 2, 3, 64, 2048, 5000):
            assert TS.ts_slabs(n, tiles) == ref.slabs_of(n, tiles), (n, tiles)
    assert ref.slabs_of(1024, 1) == 1 and ref.slabs_of(1025, 1) == 2 and ref.slabs_of(3073, 1) == 4
    assert ref.slabs_of(10 ** 7, 1) == ref.MAX_SLABS and ref.slabs_of(10 ** 7, 32) == 64


def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name, n_args in (("euler_gpu_table_topk", 13), ("euler_gpu_table_rank", 12)):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert name + "(" in hdr
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert "knn/knn.py:35-77" in hdr and "utils/metrics.py:51-83" in hdr


def test_sources_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "$(HERE)table_search.h" in mk and "table_search_kernels.hip" in mk


def test_ops_are_public_and_refuse_before_any_launch():
    import torch
    from euler_amd import ops
    assert callable(ops.table_topk) and callable(ops.table_rank)
    t, q = torch.zeros(4, 3), torch.zeros(2, 3)
    for bad in (lambda: ops.table_topk(t, q, 2, metric="dot"), lambda: ops.table_topk(t, torch.zeros(2, 4), 2),
                lambda: ops.table_topk(t, q, 0), lambda: ops.table_topk(t, q, 65), lambda: ops.table_topk(t, q, 2.0),
                lambda: ops.table_topk(t[0], q, 2), lambda: ops.table_topk(t, q, 2, exclude=torch.zeros(3, dtype=torch.int64)),
                lambda: ops.table_topk(t, q, 2, exclude=torch.zeros(2, dtype=torch.int32)),
                lambda: ops.table_rank(t, q, None), lambda: ops.table_rank(t, q, torch.zeros(2)),
                lambda: ops.table_rank(t, q, torch.zeros(3, dtype=torch.int64))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.table_topk(t.double(), q, 2)
    with pytest.raises(RuntimeError):                                   # CPU tensors: no CPU path
        ops.table_topk(t, q, 2)


# ---- the argument ladder, through the C ABI -----------------------------------------------------
A = {n: 0x10000 * (i + 1) for i, n in enumerate(["table", "queries", "exclude", "scores", "rows", "target", "rank"])}
BASE = dict(A, metric=0, table_dtype=0, n=10, d=12, q_dtype=0, q=4, k=3)
HEAD = ["metric", "table", "table_dtype", "n", "d", "queries", "q_dtype", "q"]
ARGS = {"table_topk": HEAD + ["k", "exclude", "scores", "rows"], "table_rank": HEAD + ["target", "exclude", "rank"]}
BOTH, TOPK, RANK = ("table_topk", "table_rank"), ("table_topk",), ("table_rank",)
E31 = 1 << 31
T_METRIC = "metric outside 0..3 (0 ip, 1 cos, 2 l2, 3 l1)"
T_DTYPE = "unknown dtype (0 fp32, 1 bf16, 2 fp16)"
T_N, T_Q, T_K = "n outside 0 .. 2^31 - 1", "q outside 0 .. 2^31 - 1", "k outside 1..64"
T_NULL, T_ALIGN = "null buffer", "a table is not aligned to its type"
T_OUT = "an index or output buffer is not aligned to its type"
NOTHING = {n: None for n in A}
ROWS = [
    (BOTH, dict(metric=-1), -1, T_METRIC), (BOTH, dict(metric=4), -1, T_METRIC),
    (BOTH, dict(table_dtype=3), -1, T_DTYPE), (BOTH, dict(table_dtype=-1), -1, T_DTYPE),
    (BOTH, dict(q_dtype=3), -1, T_DTYPE), (BOTH, dict(q_dtype=-1), -1, T_DTYPE),
    (BOTH, dict(d=0), -1, "d < 1"), (BOTH, dict(d=-1), -1, "d < 1"), (BOTH, dict(d=E31), -1, "d >= 2^31"),
    (BOTH, dict(n=-1), -1, T_N), (BOTH, dict(n=E31), -1, T_N),
    (BOTH, dict(q=-1), -1, T_Q), (BOTH, dict(q=E31), -1, T_Q),
    (TOPK, dict(k=0), -1, T_K), (TOPK, dict(k=-1), -1, T_K), (TOPK, dict(k=65), -1, T_K),
    # nothing to do: OK before any pointer is looked at
    (BOTH, dict(q=0), 0, None), (BOTH, dict(NOTHING, q=0), 0, None), (BOTH, dict(NOTHING, q=0, n=0), 0, None),
    # the pointers
    (BOTH, dict(table=None), -1, T_NULL), (BOTH, dict(queries=None), -1, T_NULL),
    (TOPK, dict(scores=None), -1, T_NULL), (TOPK, dict(rows=None), -1, T_NULL),
    (RANK, dict(target=None), -1, T_NULL), (RANK, dict(rank=None), -1, T_NULL),
    (BOTH, dict(n=0, table=None, queries=None), -1, T_NULL),
    (BOTH, dict(table=A["table"] + 2), -1, T_ALIGN), (BOTH, dict(queries=A["queries"] + 2), -1, T_ALIGN),
    (BOTH, dict(table_dtype=1, table=A["table"] + 1), -1, T_ALIGN),
    (BOTH, dict(q_dtype=2, queries=A["queries"] + 1), -1, T_ALIGN),
    (TOPK, dict(scores=A["scores"] + 2), -1, T_OUT), (TOPK, dict(rows=A["rows"] + 4), -1, T_OUT),
    (BOTH, dict(exclude=A["exclude"] + 4), -1, T_OUT),
    (RANK, dict(target=A["target"] + 4), -1, T_OUT), (RANK, dict(rank=A["rank"] + 2), -1, T_OUT),
    # which rule answers where two could
    (BOTH, dict(metric=9, table_dtype=9), -1, T_METRIC), (BOTH, dict(table_dtype=9, d=0), -1, T_DTYPE),
    (BOTH, dict(q=0, d=0), -1, "d < 1"), (TOPK, dict(q=0, k=0), -1, T_K), (BOTH, dict(n=-1, q=-1), -1, T_N),
    (BOTH, dict(table=None, queries=A["queries"] + 2), -1, T_NULL),
    (TOPK, dict(table=A["table"] + 2, scores=A["scores"] + 2), -1, T_ALIGN),
]


def _cases(row):
    v = dict(BASE, **row[1])
    return [(entry, [v[n] for n in ARGS[entry]]) for entry in row[0]]


def _answer_all():
    """(child) every call of every row -> [[[rc, last error], ...], ...] on stdout"""
    spec = importlib.util.spec_from_file_location("_lib", os.path.join(ROOT, "euler_amd", "_lib.py"))
    _lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(_lib)             # (the binding alone: the package would import torch)
    L = _lib.lib()
    answers = []
    for row in ROWS:
        got = []
        for entry, values in _cases(row):
            rc = getattr(L, "euler_gpu_" + entry)(None, *values)
            got.append([rc, L.euler_gpu_last_error().decode()])
        answers.append(got)
    print(json.dumps(answers))


@pytest.fixture(scope="module")
def answers():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    return json.loads(run.stdout.decode().strip().splitlines()[-1])


def test_ladder_table_covers_both_entries():
    from euler_amd import _lib
    for entry, names in ARGS.items():
        assert len(_lib.SIGNATURES["euler_gpu_" + entry][1]) == 1 + len(names), entry
        assert all(n in BASE for n in names), entry


@pytest.mark.parametrize("i", range(len(ROWS)), ids=lambda i: "%02d-%s" % (i, "-".join(sorted(ROWS[i][1]))))
def test_ladder_row(answers, i):
    row = ROWS[i]
    for (entry, values), (rc, text) in zip(_cases(row), answers[i]):
        assert rc == row[2], (entry, values, rc, text)
        if row[2] != 0:
            assert text == entry + ": " + row[3], (entry, values)


if __name__ == "__main__":
    _answer_all()
