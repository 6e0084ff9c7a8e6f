"""The table search (euler_amd/csrc/table_search.h) restated in numpy: the scores in the stated
lane order (triple_score_ref.lane_sum: chunks of V columns, L lanes, each lane adding its terms one
by one from its first, then the xor butterfly), the order of the rows, the top-k with its fills
and the full-table rank.  Tables come in already widened to fp32 (a 16-bit table: `.astype(float32)`
of it, which is exact); `v` is the chunk width KgChunkWidth gives for the real tables' types and
addresses (chunk_width below).

The order is built from a SORT KEY, not from a visiting order: rows are sorted by
(class, key, row) where class 1 holds the NaN scores (after every number), key is the score
negated for the larger-is-better metrics with -0 folded onto +0, and the row index breaks what
compares equal.  test_table_search_host.py holds the host build of the header - which inserts row
by row - against it."""
import numpy as np

import triple_score_ref as kg

F = np.float32
U = 2.0 ** -24
METRIC = {"ip": 0, "cos": 1, "l2": 2, "l1": 3}
EPS = kg.EPS
MAX_K = 64
# the launch shape (table_search.h): queries a wave, waves a block, rows a slab at least, the caps
WAVES, WAVE_QUERIES, LDS_FLOATS = 4, 8, 12288
MIN_SLAB_ROWS, MAX_SLABS, TARGET_BLOCKS, BLOCK_CAP = 1024, 512, 2048, 256 * 32

chunk_width = kg.chunk_width
lane_sum = kg.lane_sum


def larger_is_better(metric):
    return metric in ("ip", "cos")


def fill(metric):
    return F(-np.inf) if larger_is_better(metric) else F(np.inf)


def wave_queries(d):
    """-> (queries a wave, staged in LDS?)"""
    fit = LDS_FLOATS // (WAVES * d)
    return (WAVE_QUERIES if fit < 1 or fit > WAVE_QUERIES else fit), fit >= 1


def tiles_of(q, d):
    return -(-q // (WAVES * wave_queries(d)[0]))


def slabs_of(n, tiles):
    s = -(-TARGET_BLOCKS // max(tiles, 1))
    return max(1, min(s, -(-n // MIN_SLAB_ROWS), MAX_SLABS))


def inv_of(x, v):
    """KgInv(ss, true) of every row of x [N, d]"""
    with np.errstate(invalid="ignore", over="ignore"):
        ss = lane_sum(x * x, v) if len(x) else np.zeros(0, F)
        return (F(1) / np.sqrt(np.where(ss > EPS, ss, EPS))).astype(F)


def scores(table, queries, metric, v):
    """-> [Q, N] fp32 scores, every one in the stated order"""
    table, queries = np.ascontiguousarray(table, F), np.ascontiguousarray(queries, F)
    n, q = len(table), len(queries)
    out = np.zeros((q, n), F)
    if n == 0:
        return out
    inv_x = inv_of(table, v) if metric == "cos" else None
    inv_q = inv_of(queries, v) if metric == "cos" else None
    if q > n:                                    # (the same pairs, looped over the shorter side)
        return np.ascontiguousarray(_scores_by_row(table, queries, metric, v, inv_q, inv_x).T)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(q):
            if metric in ("ip", "cos"):
                terms = queries[i][None, :] * table
            else:
                e = queries[i][None, :] - table
                terms = e * e if metric == "l2" else np.abs(e)
            s = lane_sum(terms, v)
            if metric == "cos":
                s = (s * inv_q[i]) * inv_x
            out[i] = s
    return out


def _scores_by_row(table, queries, metric, v, inv_q, inv_x):
    """-> [N, Q]: scores() with the loop over the table's rows (term order q op x kept)"""
    out = np.zeros((len(table), len(queries)), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(len(table)):
            if metric in ("ip", "cos"):
                terms = queries * table[r][None, :]
            else:
                e = queries - table[r][None, :]
                terms = e * e if metric == "l2" else np.abs(e)
            s = lane_sum(terms, v)
            if metric == "cos":
                s = (s * inv_q) * inv_x[r]
            out[r] = s
    return out


def order_all(s, metric):
    """order() of every row of s [Q, N] at once -> [Q, N] (a stable sort: equal keys keep row order)"""
    s = np.asarray(s, F)
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):
        key = np.where(nan, F(np.inf), (-s if larger_is_better(metric) else s) + F(0))
    # NaN after +inf keys: sort by (nan, key) through two stable passes
    first = np.argsort(key, axis=1, kind="stable")
    second = np.argsort(np.take_along_axis(nan, first, 1), axis=1, kind="stable")
    return np.take_along_axis(first, second, 1)


def order(s, metric):
    """the rows of one query, best first, for its scores s [N]"""
    s = np.asarray(s, F)
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):
        key = np.where(nan, F(0), (-s if larger_is_better(metric) else s) + F(0))      # (-0 + 0 = +0)
    return np.lexsort((np.arange(len(s)), key, nan))


def _none_if_outside(ids, q, n):
    if ids is None:
        return np.full(q, -1, np.int64)
    ids = np.asarray(ids, np.int64)
    return np.where((ids >= 0) & (ids < n), ids, -1)


def topk(table, queries, k, metric, v, exclude=None, s=None):
    """-> (scores [Q, k] fp32, rows [Q, k] int64)"""
    q, n = len(queries), len(table)
    s = scores(table, queries, metric, v) if s is None else s
    exc = _none_if_outside(exclude, q, n)
    out_s, out_r = np.full((q, k), fill(metric), F), np.full((q, k), -1, np.int64)
    for i in range(q):
        rows = order(s[i], metric)
        rows = rows[rows != exc[i]][:k]
        out_r[i, :len(rows)] = rows
        out_s[i, :len(rows)] = s[i][rows]
    return out_s, out_r


def rank(table, queries, target, metric, v, exclude=None, s=None):
    """-> [Q] int32"""
    q, n = len(queries), len(table)
    s = scores(table, queries, metric, v) if s is None else s
    tgt, exc = _none_if_outside(target, q, n), _none_if_outside(exclude, q, n)
    out = np.full(q, -1, np.int32)
    r = np.arange(n)
    for i in range(q):
        if tgt[i] < 0:
            continue
        st = s[i][tgt[i]]
        with np.errstate(invalid="ignore"):
            hit = (s[i] >= st) if larger_is_better(metric) else (s[i] <= st)
        out[i] = np.count_nonzero(hit & (r != tgt[i]) & (r != exc[i]))
    return out


def scores64(table, queries, metric):
    """-> (float64 scores [Q, N], the bound of |fp32 restatement - them|).

    The bound, with u = 2^-24 and gamma(m) = m u / (1 - m u) (Higham, Accuracy and Stability, 3.1):
    a sum of d terms added in ANY order has error <= gamma(d - 1) * sum |terms| given exact terms;
    each term carries its own roundings - ip: one multiply, (1 + u); l2: a subtraction and a
    multiply of the rounded difference by itself, (1 + u)^3; l1: a subtraction, (1 + u).  So
      ip  gamma(d) * sum |q x|       l1  gamma(d) * sum |q - x|       l2  gamma(d + 2) * sum (q - x)^2
    cos = (ip * inv_q) * inv_x: inv = 1 / sqrt(ss) has ss within gamma(d) (all terms positive), the
    square root and the division one rounding each, so inv within gamma(d / 2 + 3) relatively (the
    square root halves the relative error of ss: count d / 2 + 1 roundings, then sqrt and divide);
    two more multiplies.  |cos^ - cos| <= gamma(d) sum|q x| inv_q inv_x (1 + small) +
    |cos| gamma(d + 8) <= gamma(2 d + 8) * sum |q x| * inv_q * inv_x, since |ip| <= sum |q x|.
    Rows with ss <= 1e-12 are left out by the caller (the clamp is not a rounding)."""
    t, qs = np.asarray(table, np.float64), np.asarray(queries, np.float64)
    d = t.shape[1]
    if metric in ("ip", "cos"):
        exact, mag = qs @ t.T, np.abs(qs) @ np.abs(t).T
        if metric == "ip":
            return exact, kg.gamma(d) * mag
        iq = 1.0 / np.sqrt((qs * qs).sum(1))[:, None]
        ix = 1.0 / np.sqrt((t * t).sum(1))[None, :]
        return exact * iq * ix, kg.gamma(2 * d + 8) * mag * iq * ix
    e = qs[:, None, :] - t[None, :, :]
    if metric == "l2":
        exact = (e * e).sum(-1)
        return exact, kg.gamma(d + 2) * exact
    exact = np.abs(e).sum(-1)
    return exact, kg.gamma(d) * exact


# ---- the cases both test files run ----------------------------------------------------------------
DIMS = (1, 3, 4, 8, 12, 64, 130)          # V = 1 / 4 / 8; at 130 a lane with more than one chunk
METRICS = ("ip", "cos", "l2", "l1")
DTYPES = ("f32", "bf16", "f16")
KS = (1, 2, 3, 10, 16, 17, 64)
ITEM = {"f32": 4, "bf16": 2, "f16": 2}


def to_dtype(x, dt):
    """fp32 values rounded to a storage type and widened again (what a table of that type holds)"""
    x = np.ascontiguousarray(x, F)
    if dt == "f32":
        return x
    if dt == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(F)
    u = x.view(np.uint32).astype(np.uint64)
    nan = np.isnan(x)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16                      # ties to even
    out = r.astype(np.uint32).view(F).copy()
    out[nan] = np.nan
    return out


def same_scores(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if not (a.dtype == b.dtype == np.float32 and a.shape == b.shape):
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def tie_table(rng, n, d, dt):
    """the first half drawn from {-2, -1, -0.0, 0, 1, 2} (exact scores that collide) with rows
    repeated, a row of NaN and a row with an inf; the second half random over four decades"""
    small = np.array([-2, -1, -0.0, 0, 1, 2], F)
    t = np.empty((n, d), F)
    half = max(1, n // 2)
    t[:half] = small[rng.integers(0, 6, (half, d))]
    t[half:] = (rng.random((n - half, d)) * 2 - 1) * 10.0 ** rng.integers(-2, 2, (n - half, d))
    if n >= 40:
        t[10], t[11], t[25], t[n - 1] = t[3], t[3], t[4], t[3]
        t[17] = np.nan
        t[18, 0] = np.inf
        t[half + 3] = t[half + 1]
    return to_dtype(t, dt)


def queries_for(rng, table, dq, q=6):
    """rows of the table (their own row excluded by the caller), small integers and random rows"""
    n, d = table.shape
    own = rng.integers(0, n, q // 2)
    small = np.array([-2, -1, -0.0, 0, 1, 2], F)
    rest = np.concatenate([small[rng.integers(0, 6, (1, d))], rng.standard_normal((q - len(own) - 1, d)).astype(F)])
    return to_dtype(np.concatenate([table[own], rest]), dq), own
