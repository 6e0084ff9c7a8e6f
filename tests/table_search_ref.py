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


# ---- a table whose rows are zero except a few ------------------------------------------------------
def _sparse_parts(probe, values, n, queries, metric, v):
    """-> (probe int64 [P], sp [Q, P] the probe rows' scores, z [Q] the score of a zero row).  A score is
    a function of the two rows, their types and V alone (table_search.h), so every zero row of the
    table scores what scores() gives for one literal zero row."""
    probe = np.asarray(probe, np.int64)
    values = np.ascontiguousarray(values, F)
    assert values.shape[0] == len(probe) and np.all(np.diff(probe) > 0)
    assert len(probe) == 0 or (probe[0] >= 0 and probe[-1] < n)
    sp = scores(values, queries, metric, v)
    z = scores(np.zeros((1, values.shape[1]), F), queries, metric, v)[:, 0]
    return probe, sp, z


def sparse_topk(probe, values, n, queries, k, metric, v, exclude=None):
    """topk() for the [n, d] table whose rows `probe` (sorted) hold `values` and whose other rows are
    all zero, without building it: the candidates of a query are the probe rows and the k
    lowest-numbered zero rows (a zero row past them is preceded by k rows that tie with it), without
    exclude[q]; ordered by order() with the real row numbers breaking ties."""
    probe, sp, z = _sparse_parts(probe, values, n, queries, metric, v)
    q = len(sp)
    exc = _none_if_outside(exclude, q, n)
    # the k + 1 lowest rows that are no probe row: among the first k + 1 + P rows
    low = np.setdiff1d(np.arange(min(n, k + 1 + len(probe)), dtype=np.int64), probe)[:k + 1]
    out_s, out_r = np.full((q, k), fill(metric), F), np.full((q, k), -1, np.int64)
    for i in range(q):
        zero = low[low != exc[i]][:k]
        rows = np.concatenate([probe, zero])
        sc = np.concatenate([sp[i], np.full(len(zero), z[i], F)])
        keep = rows != exc[i]
        rows, sc = rows[keep], sc[keep]
        by_row = np.argsort(rows, kind="stable")
        rows, sc = rows[by_row], sc[by_row]                 # order() breaks ties by position: make it the row
        best = order(sc, metric)[:k]
        out_r[i, :len(best)] = rows[best]
        out_s[i, :len(best)] = sc[best]
    return out_s, out_r


def sparse_rank(probe, values, n, queries, target, metric, v, exclude=None):
    """rank() for the same table: the probe rows that count, plus - where a zero row's score is
    better than or equal to the target's - every zero row but the target and the exclude"""
    probe, sp, z = _sparse_parts(probe, values, n, queries, metric, v)
    q = len(sp)
    tgt, exc = _none_if_outside(target, q, n), _none_if_outside(exclude, q, n)
    out = np.full(q, -1, np.int32)
    larger = larger_is_better(metric)
    for i in range(q):
        if tgt[i] < 0:
            continue
        at = np.searchsorted(probe, tgt[i])
        t_zero = not (at < len(probe) and probe[at] == tgt[i])
        st = z[i] if t_zero else sp[i][at]
        with np.errstate(invalid="ignore"):
            hit = (sp[i] >= st) if larger else (sp[i] <= st)
            z_hit = bool(z[i] >= st) if larger else bool(z[i] <= st)
        count = int(np.count_nonzero(hit & (probe != tgt[i]) & (probe != exc[i])))
        if z_hit:
            e_zero = exc[i] >= 0 and exc[i] not in probe and exc[i] != tgt[i]
            count += n - len(probe) - int(t_zero) - int(e_zero)
        out[i] = count
    return out


def topk_of_scores(s, k, metric, exclude=None):
    """topk() from a [Q, N] block of scores for many queries: a partition finds each query's k + 1
    best keys, order() then runs over the rows that reach them (all ties included) instead of N"""
    s = np.asarray(s, F)
    q, n = s.shape
    exc = _none_if_outside(exclude, q, n)
    out_s, out_r = np.full((q, k), fill(metric), F), np.full((q, k), -1, np.int64)
    if n == 0:
        return out_s, out_r
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):
        key = np.where(nan, F(np.inf), (-s if larger_is_better(metric) else s) + F(0))
    kth = min(k, n - 1)                                     # (k + 1 keys: one may be the excluded row's)
    bar = np.partition(key, kth, axis=1)[:, kth]
    for i in range(q):
        cand = np.flatnonzero(key[i] <= bar[i])             # in row order
        cand = cand[cand != exc[i]]
        best = cand[order(s[i][cand], metric)[:k]]
        out_r[i, :len(best)] = best
        out_s[i, :len(best)] = s[i][best]
    return out_s, out_r


def rank_of_scores(s, target, metric, exclude=None):
    """rank() from a [Q, N] block of scores, without the loop over the queries"""
    s = np.asarray(s, F)
    q, n = s.shape
    if n == 0:
        return np.full(q, -1, np.int32)
    tgt, exc = _none_if_outside(target, q, n), _none_if_outside(exclude, q, n)
    col = lambda ids: np.clip(ids, 0, max(n - 1, 0))[:, None]                 # noqa: E731
    st = np.take_along_axis(s, col(tgt), 1)
    with np.errstate(invalid="ignore"):
        hit = (s >= st) if larger_is_better(metric) else (s <= st)
    count = hit.sum(1) - np.take_along_axis(hit, col(tgt), 1)[:, 0]
    count -= np.where((exc >= 0) & (exc != tgt), np.take_along_axis(hit, col(exc), 1)[:, 0], False)
    return np.where(tgt >= 0, count, -1).astype(np.int32)


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


# ---- views off a 16-byte boundary -------------------------------------------------------------------
# (table dtype, its bytes past a 16-byte boundary, queries dtype, their bytes past one, d, the V the rule
# gives): the branches of KgChunkWidth that an aligned pair of tables never takes, and V = 1 / 4 in
# the unstaged path (d > 3072).  N = ALIGN_N rows (two slabs), ALIGN_Q queries (two tiles).
ALIGN_CASES = (
    ("bf16", 8, "f32", 0, 8, 4), ("bf16", 8, "f32", 0, 64, 4),     # a 16-bit table 8 bytes off: V = 4 although d % 8 == 0
    ("bf16", 2, "bf16", 0, 8, 1), ("f16", 0, "f16", 2, 64, 1),     # 16-bit views one element off
    ("f32", 8, "f32", 0, 8, 1), ("f32", 0, "f32", 4, 12, 1),       # fp32 needs 16 bytes for V = 4 too
    ("f32", 0, "bf16", 8, 12, 4),                                  # misaligned queries, V = 4 kept
    ("bf16", 0, "f32", 0, 3073, 1), ("f32", 0, "f16", 0, 3076, 4),  # unstaged
)
ALIGN_N, ALIGN_Q = 1100, 33


def align_case_width(case, base=4096):
    dtt, off_t, dq, off_q, d, _ = case
    return chunk_width(d, base + off_t, ITEM[dtt], 2 * base + off_q, ITEM[dq])


# ---- the list of the k best under chosen arrival orders ----------------------------------------------
# An fp32 table that is zero but for column 0, against queries that are zero but for column 0: under
# ip the score of row r is q_0 * x_r0, under l2 (q_0 - x_r0)^2, exact small integers, so the order
# in which the rows enter (and leave) a list is chosen by the column.
ARRIVAL_N = 2049                              # three slabs for one tile of queries
ARRIVAL_ORDERS = ("improving", "worsening", "equal", "sawtooth", "zeros")
ARRIVAL_DIMS = (1, 4, 64)                     # d = 1: 64 rows side by side, 256 candidates a step
ARRIVAL_KS = (1, 63, 64)


def arrival_case(kind, metric, d, n=ARRIVAL_N):
    """-> (table [n, d], queries [3, d]) fp32.  For the first query: `improving` - every row
    precedes all rows before it (each insert is at position 0), `worsening` - none enters a full list,
    `equal` - all tie, `sawtooth` - period 7, `zeros` - +0 and -0 alternating (equal).  The other two
    queries reverse and fold the order."""
    assert metric in ("ip", "l2") and kind in ARRIVAL_ORDERS
    r = np.arange(n, dtype=np.int64)
    up = r if metric == "ip" else n - r           # l2: smaller is better
    col = {"improving": up, "worsening": n - up, "equal": np.ones(n), "sawtooth": r % 7,
           "zeros": np.where(r % 2 == 0, 0.0, -0.0)}[kind]
    table, queries = np.zeros((n, d), F), np.zeros((3, d), F)
    table[:, 0] = col
    queries[:, 0] = (1, -1, 0.5) if metric == "ip" else (0, 3, -2)
    assert np.abs(table).max() + 3 < 2 ** 12                            # squares stay exact in fp32
    return table, queries


# ---- the rank against float64 --------------------------------------------------------------------------
SEPARATED = dict(seed=31, n=3073, d=64, q=33)


def separated_rank_case(metric, seed, n, d, q):
    """Random fp32 data and a target per query whose float64 score no other row's comes within
    2 * bound of (bound: the largest of scores64): the fp32 comparison of every row with the target
    then goes the way the float64 one does, so table_rank must return the float64 count.  The
    targets aim at places spread over the whole order (the best row ... the last) and move to the
    nearest place that is separated.  -> (table, queries, target [q], count [q] int32, the margin:
    the smallest distance to a target's score over 2 * bound)"""
    rng = np.random.default_rng(seed)
    table, queries = rng.standard_normal((n, d)).astype(F), rng.standard_normal((q, d)).astype(F)
    exact, bound = scores64(table, queries, metric)
    lim = 2 * bound.max()
    key = -exact if larger_is_better(metric) else exact
    aim = ((n - 1) * (np.arange(q) / (q - 1)) ** 3).astype(np.int64)     # 0 ... n - 1, dense near the best
    target, margin = np.zeros(q, np.int64), np.inf
    for i in range(q):
        by_key = np.argsort(key[i], kind="stable")
        gap = np.diff(key[i][by_key])
        ok = np.concatenate([[True], gap > lim]) & np.concatenate([gap > lim, [True]])
        places = np.flatnonzero(ok)
        target[i] = by_key[places[np.argmin(np.abs(places - aim[i]))]]
        away = np.abs(exact[i] - exact[i][target[i]])
        away[target[i]] = np.inf
        margin = min(margin, away.min() / lim)
    st = np.take_along_axis(exact, target[:, None], 1)
    count = ((exact >= st) if larger_is_better(metric) else (exact <= st)).sum(1) - 1
    return table, queries, target, count.astype(np.int32), float(margin)
