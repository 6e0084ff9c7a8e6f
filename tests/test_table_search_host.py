"""The table search (euler_amd/csrc/table_search.h) compiled with the host compiler, over whole
calls, against the numpy restatement tests/table_search_ref.py: bit equality of the scores, the
rows and the ranks; the order rule on tie-heavy tables; the fills; exclude and target in and out of
range; the restatement within the derived bound of float64; the C-ABI entries exported and bound,
and every rule of their argument ladder (driven through the C ABI in a child process that sees no
GPU: every row stops in front of the first HIP call).  Then what the GPU cases rest on: the slab
rule at its clamps and its shortest last slab, V of every alignment case, sparse_topk / sparse_rank
(a mostly-zero table that is never built) against the dense restatement, the chosen arrival orders,
NaN queries and fill-valued rows through the host build, the separation behind the float64 rank
check.  CPU only.

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


def test_slab_clamps_and_the_shortest_last_slab(TS):
    """the three terms of TsSlabs at the shapes test_table_search_gpu.py and test_big_offsets_gpu.py
    run, and the shortest last slab the rule allows: over every N up to 2^20 and every tile count, a
    last slab is never empty and never shorter than 512 rows, and is shortest against the other
    slabs at N = 511 * 1024 + 1 - 512 slabs of 1023 rows, the last of 512"""
    # the clamp by the number of tiles: 101 tiles, ceil(2048 / 101) = 21 < ceil(30000 / 1024) = 30
    q = 32 * 100 + 1
    assert ref.tiles_of(q, 4) == 101 and -(-2048 // 101) == 21 and -(-30000 // 1024) == 30
    assert ref.slabs_of(30000, 101) == 21 == TS.ts_slabs(30000, 101)
    for n in (21 * 1024 - 1, 21 * 1024, 21 * 1024 + 1):
        assert ref.slabs_of(n, 101) == 21 == TS.ts_slabs(n, 101), n
    assert ref.slabs_of(20 * 1024, 101) == 20                       # (below it the rows decide)
    # the cap
    for n in (512 * 1024 + 1, 10 ** 6, 10 ** 8, 2 ** 31 - 1):
        assert ref.slabs_of(n, 1) == 512 == TS.ts_slabs(n, 1) and ref.slabs_of(n, 4) == 512, n
    assert ref.slabs_of(511 * 1024, 1) == 511 and ref.slabs_of(512 * 1024 + 1, 5) == 410
    # every (N, tiles): the last slab
    n = np.arange(1, 1 << 20, dtype=np.int64)
    by_rows = -(-n // ref.MIN_SLAB_ROWS)
    worst = (2.0, None)
    first_tiles = {}                          # the rule sees the tiles through min(ceil(2048 / tiles), 512) alone
    for tiles in range(2050, 0, -1):
        first_tiles[min(-(-ref.TARGET_BLOCKS // tiles), ref.MAX_SLABS)] = tiles
    for cap, tiles in sorted(first_tiles.items(), reverse=True):
        s = np.maximum(1, np.minimum(by_rows, cap))
        assert s[-1] == ref.slabs_of(int(n[-1]), tiles) and s[2000] == ref.slabs_of(2001, tiles)
        slab_rows = -(-n // s)
        last = n - (s - 1) * slab_rows
        assert last.min() >= 1 and last[s > 1].min(initial=512) >= 512, tiles
        share = np.where(s > 1, last / slab_rows, 2.0)
        at = int(np.argmin(share))
        if share[at] < worst[0]:
            worst = (float(share[at]), (int(n[at]), tiles, int(s[at]), int(slab_rows[at]), int(last[at])))
    assert worst[1] == (511 * 1024 + 1, 1, 512, 1023, 512)


@pytest.mark.parametrize("case", ref.ALIGN_CASES, ids=lambda c: "%s+%d-%s+%d-d%d-V%d" % c)
def test_alignment_cases_take_the_width_they_are_meant_for(TS, case):
    """the case table of test_table_search_gpu.py::test_views_off_a_16_byte_boundary: V as stated,
    by the header's rule and by the restatement; the host build over that V == the restatement"""
    dtt, off_t, dq, off_q, d, v = case
    assert off_t % ITEM[dtt] == 0 and off_q % ITEM[dq] == 0 and d % v == 0
    assert ref.align_case_width(case) == v == TS.ts_chunk_width(d, 4096 + off_t, dtt == "f32", 8192 + off_q, dq == "f32")
    aligned = ref.chunk_width(d, 0, ITEM[dtt], 0, ITEM[dq])
    assert aligned == v or off_t or off_q                                # only an offset moves V
    assert ref.wave_queries(d)[1] == (d <= 3072)
    assert ref.slabs_of(ref.ALIGN_N, ref.tiles_of(ref.ALIGN_Q, d)) == 2 and ref.tiles_of(ref.ALIGN_Q, d) == 2
    rng = np.random.default_rng(d + off_t + off_q)
    n = 40 if d > 3072 else 120
    table = tie_table(rng, n, d, dtt)
    queries, own = queries_for(rng, table, dq)
    for metric in METRICS if d <= 3072 else ("cos", "l1"):
        check_case(TS, table, queries, metric, v, (10,), (n,), own, case + (metric,))


# ---- a mostly-zero table: sparse_topk / sparse_rank == the dense restatement ---------------------
SPARSE_N = 3000
SPARSE_PROBE = np.array([0, 1, 3, 700, 701, 1499, 1500, 2047, 2048, 2990, SPARSE_N - 2, SPARSE_N - 1])


def sparse_case(rng, d, dtt, dq):
    """-> (values [12, d], the dense table, queries [18, d], target [18], exclude [18]): queries equal
    to probe rows, to the zero row, and random; every pair of (target kind, exclude kind) out of
    probe row / zero row / -1 / n + 5, then target == exclude on a zero row and on a probe row"""
    n, probe = SPARSE_N, SPARSE_PROBE
    values = to_dtype(np.round(rng.standard_normal((len(probe), d)) * 16) / 16, dtt)
    values[4] = values[3]                                                 # two probe rows that tie
    dense = np.zeros((n, d), F)
    dense[probe] = values
    base = np.concatenate([values[[0, 3, 11]], np.zeros((1, d), F), -values[[5]], rng.standard_normal((3, d)).astype(F)])
    queries = to_dtype(base[np.arange(18) % 8], dq)
    kinds = {"probe": (0, 701, n - 1, 1500), "zero": (2, 4, 1600, n - 3), "none": (-1,) * 4, "past": (n + 5,) * 4}
    target, exclude = [], []
    for a, ka in enumerate(kinds):
        for b, kb in enumerate(kinds):
            target.append(kinds[ka][b])
            exclude.append(kinds[kb][(a + 1) % 4])
    target += [2, 701]
    exclude += [2, 701]
    return values, dense, queries, np.array(target, np.int64), np.array(exclude, np.int64)


@pytest.mark.parametrize("dtt", DTYPES)
@pytest.mark.parametrize("d", (129, 132, 136))
def test_sparse_helpers_equal_the_dense_restatement(d, dtt):
    """sparse_topk / sparse_rank (which never build the table) against topk / rank on the table
    built explicitly: n = 3000, 12 probe rows with rows 0, 1, n - 2, n - 1 among them; the four
    metrics, k = 1 / 10 / 64, with and without exclude.  Zero rows enter the lists ahead of probe
    rows and behind them."""
    n, probe = SPARSE_N, SPARSE_PROBE
    assert {0, 1, n - 2, n - 1} <= set(probe.tolist()) and len(probe) == 12
    dq = DTYPES[(DTYPES.index(dtt) + 1) % 3]
    rng = np.random.default_rng(7 * d + DTYPES.index(dtt))
    values, dense, queries, target, exclude = sparse_case(rng, d, dtt, dq)
    assert np.count_nonzero(dense.any(1)) == len(probe)
    v = ref.chunk_width(d, 0, ITEM[dtt], 0, ITEM[dq])
    assert v == (8 if d % 8 == 0 else 4 if d % 4 == 0 else 1)
    is_probe = np.zeros(n + 1, bool)
    is_probe[probe] = True
    ahead = behind = 0
    for metric in METRICS:
        s = ref.scores(dense, queries, metric, v)
        for exc in (None, exclude):
            for k in (1, 10, 64):
                got = ref.sparse_topk(probe, values, n, queries, k, metric, v, exc)
                want = ref.topk(dense, queries, k, metric, v, exc, s=s)
                assert same_scores(got[0], want[0]) and np.array_equal(got[1], want[1]), (metric, k, exc is None)
                if k == 64:
                    assert np.all(want[1] >= 0)
                    p = is_probe[want[1]]
                    ahead += np.count_nonzero(~p[:, :-1] & p[:, 1:])          # a zero row, then a probe row
                    behind += np.count_nonzero(p[:, :-1] & ~p[:, 1:])
            got = ref.sparse_rank(probe, values, n, queries, target, metric, v, exc)
            assert got.dtype == np.int32
            assert np.array_equal(got, ref.rank(dense, queries, target, metric, v, exc, s=s)), (metric, exc is None)
            assert np.array_equal(got, ref.rank_of_scores(s, target, metric, exc)), (metric, exc is None)
        assert np.array_equal(ref.topk_of_scores(s, 10, metric, exclude)[1],
                              ref.topk(dense, queries, 10, metric, v, exclude, s=s)[1])
    assert ahead > 0 and behind > 0


@pytest.mark.parametrize("metric", METRICS)
def test_block_forms_of_topk_and_rank_equal_the_loops(metric):
    """topk_of_scores / rank_of_scores (what the many-query GPU cases are compared with) == topk /
    rank on the tie-heavy table with its NaN and inf rows, exclude and targets in and out of range"""
    rng = np.random.default_rng(21)
    table = tie_table(rng, 300, 4, "f32")
    queries, _ = queries_for(rng, table, "f32", q=40)
    s = ref.scores(table, queries, metric, 4)
    for n in (1, 9, 10, 11, 300):
        exc, target = rng.integers(-2, n + 2, 40), rng.integers(-1, n + 1, 40)
        for k in (1, 10, 64):
            for e in (None, exc):
                got = ref.topk_of_scores(s[:, :n], k, metric, e)
                want = ref.topk(table[:n], queries, k, metric, 4, e, s=s[:, :n])
                assert same_scores(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, k)
        assert np.array_equal(ref.rank_of_scores(s[:, :n], target, metric, exc),
                              ref.rank(table[:n], queries, target, metric, 4, exc, s=s[:, :n])), n


# ---- the list under chosen arrival orders ---------------------------------------------------------
@pytest.mark.parametrize("metric", ("ip", "l2"))
@pytest.mark.parametrize("kind", ref.ARRIVAL_ORDERS)
def test_arrival_orders_host_build_equals_the_restatement(TS, kind, metric):
    """the cases of test_table_search_gpu.py::test_arrival_orders through the host build, which
    inserts row by row, forwards and backwards; and the scores are the chosen ones"""
    n = ref.ARRIVAL_N
    assert ref.slabs_of(n, 1) == 3
    for d in ref.ARRIVAL_DIMS:
        table, queries = ref.arrival_case(kind, metric, d)
        v = ref.chunk_width(d, 0, 4, 0, 4)
        s = ref.scores(table, queries, metric, v)
        col = table[:, 0].astype(np.float64)
        assert np.array_equal(s[0], col if metric == "ip" else col * col)
        best = ref.order(s[0], metric)
        if kind == "improving":
            assert best.tolist() == list(range(n - 1, -1, -1))
        elif kind == "worsening" or kind == "equal" or kind == "zeros":
            assert best.tolist() == list(range(n))
        else:
            assert best[:4].tolist() == ([6, 13, 20, 27] if metric == "ip" else [0, 7, 14, 21])
        for k in ref.ARRIVAL_KS if d == 4 else (63,):
            want = ref.topk(table, queries, k, metric, v, s=s)
            for backwards in (False, True):
                got = host_topk(TS, table, queries, k, metric, v, backwards=backwards)
                assert same_scores(got[0], want[0]) and np.array_equal(got[1], want[1]), (d, k, backwards)


@pytest.mark.parametrize("metric", METRICS)
def test_nan_queries_and_rows_that_score_the_fill(TS, metric):
    """table_search.h lines 30-35 on the restatement and the host build: a query with a NaN makes
    every score NaN - rows 0 .. k - 1 in row order, every rank 0; a real row whose score is the
    fill value comes back with its row number, behind every other row and ahead of the -1 entries"""
    larger = ref.larger_is_better(metric)
    rng = np.random.default_rng(5)
    table = rng.standard_normal((70, 4)).astype(F)
    queries = rng.standard_normal((2, 4)).astype(F)
    queries[0, 2] = np.nan
    s = ref.scores(table, queries, metric, 4)
    assert np.all(np.isnan(s[0])) and not np.any(np.isnan(s[1]))
    for fn in (lambda k: ref.topk(table, queries, k, metric, 4), lambda k: host_topk(TS, table, queries, k, metric, 4)):
        sc, rows = fn(64)
        assert rows[0].tolist() == list(range(64)) and np.all(np.isnan(sc[0]))
    target = np.array([33, 33])
    for got in (ref.rank(table, queries, target, metric, 4), host_rank(TS, table, queries, target, metric, 4)):
        assert got[0] == 0 and got[1] == np.count_nonzero((s[1] >= s[1][33]) if larger else (s[1] <= s[1][33])) - 1
    # a row that scores the fill value: -inf under ip / cos, +inf under l2 / l1 (positive queries)
    worst = F(-np.inf) if larger else F(np.inf)
    table, queries = np.abs(table[:5]) + F(1), np.abs(queries) + F(1)
    queries[0, 2] = 1
    table[2, 1] = worst
    if metric == "cos":                       # (an inf in a row makes its cos NaN: plant the score instead)
        s = ref.scores(table[[0, 1, 1, 3, 4]], queries, metric, 4)
        s[:, 2] = worst
    else:
        s = ref.scores(table, queries, metric, 4)
    assert np.all(s[:, 2] == worst) and np.all(np.isfinite(np.delete(s, 2, 1)))
    sc, rows = ref.topk(table, queries, 8, metric, 4, s=s)
    assert np.all(rows[:, 4] == 2) and np.all(sc[:, 4] == worst) and np.all(rows[:, 5:] == -1) and np.all(sc[:, 5:] == worst)
    assert np.all(np.sort(rows[:, :4], 1) == [0, 1, 3, 4])
    if metric != "cos":
        got = host_topk(TS, table, queries, 8, metric, 4)
        assert same_scores(got[0], sc) and np.array_equal(got[1], rows)
        # every row scores the fill value: the list is still rows 0 .. in order, each with its number
        table[:, 1] = worst
        for fn in (lambda: ref.topk(table, queries, 8, metric, 4), lambda: host_topk(TS, table, queries, 8, metric, 4)):
            sc, rows = fn()
            assert rows.tolist() == [[0, 1, 2, 3, 4, -1, -1, -1]] * 2 and np.all(sc == worst)
        assert ref.rank(table, queries, [2, 4], metric, 4).tolist() == [4, 4]
        assert host_rank(TS, table, queries, [2, 4], metric, 4).tolist() == [4, 4]


@pytest.mark.parametrize("metric", METRICS)
def test_separated_rank_case_holds_its_precondition(metric):
    """test_table_search_gpu.py::test_rank_equals_the_float64_count: no row's float64 score lies within
    2 * bound of a target's, the targets cover the best row, the last and the middle, and the
    restatement (fp32, in the stated order) already returns the float64 count"""
    table, queries, target, count, margin = ref.separated_rank_case(metric, **ref.SEPARATED)
    assert table.shape == (3073, 64) and queries.shape == (33, 64) and table.dtype == queries.dtype == F
    assert margin > 1
    assert count.min() == 0 and count.max() == 3072 and np.count_nonzero((count > 100) & (count < 2900)) >= 5
    assert np.array_equal(ref.rank(table, queries, target, metric, 8), count)


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
