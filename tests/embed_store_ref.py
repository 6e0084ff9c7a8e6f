"""The in-place embedding stores (euler_amd/csrc/embed_store.h) restated as plain sequential numpy
loops over the occurrences - what tf.scatter_update / tf.scatter_add do on the CPU
(tf_euler/python/utils/embedding.py:24-68) and the lookup-then-clear of utils/encoders.py:738-743.
This is the reference of the host check and of the GPU tests: every comparison with it is bit
equality.

A table / values / out array is float32, or uint16 holding the bits of bf16 / fp16; `dt` names
which: "f32", "bf16", "f16".  Widening is exact; narrowing rounds once to nearest even."""
import numpy as np

DTYPES = ("f32", "bf16", "f16")
U = 2.0 ** -24                                    # unit roundoff of fp32


def gamma(n):
    return n * U / (1 - n * U)


def widen(a, dt):
    """-> float32, exactly"""
    if dt == "f32":
        return np.asarray(a, np.float32)
    a = np.asarray(a, np.uint16)
    if dt == "bf16":
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.view(np.float16).astype(np.float32)


def narrow(f, dt):
    """float32 -> the storage of dt, one round to nearest even (finite values and infinities)"""
    f = np.asarray(f, np.float32)
    if dt == "f32":
        return f
    if dt == "bf16":
        u = f.view(np.uint32).astype(np.uint64)
        return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    with np.errstate(over="ignore"):
        return f.astype(np.float16).view(np.uint16)


def convert(a, src, dst):
    """an array stored as src, stored as dst: the bits when they agree, else through float32"""
    return np.array(a, copy=True) if src == dst else narrow(widen(a, src), dst)


def zeros(shape, dt):
    return np.zeros(shape, np.float32 if dt == "f32" else np.uint16)


def in_range(i, rows):
    return 0 <= i < rows


def source_row(p, m, row_index, count):
    """the row of values occurrence p reads, or None when the range rule removes it"""
    if row_index is not None:
        r = int(row_index[p])
        return r if 0 <= r < m else None
    return p // count if count else p


def _check(ids, values, row_index, count):
    e, m = len(ids), values.shape[0]
    assert row_index is None or not count
    if row_index is not None:
        assert len(row_index) == e
    elif count:
        assert count > 0 and e % count == 0 and m == e // count
    else:
        assert m == e


def update(table, dt, ids, values, vdt, row_index=None, count=None):
    """-> the table after tf.scatter_update: a loop over p, later occurrences overwrite earlier"""
    _check(ids, values, row_index, count)
    out = np.array(table, copy=True)
    rows = out.shape[0]
    for p, i in enumerate(ids):
        s = source_row(p, values.shape[0], row_index, count)
        if in_range(int(i), rows) and s is not None:
            out[int(i)] = convert(values[s], vdt, dt)
    return out


def add(table, dt, ids, values, vdt, row_index=None, count=None, reverse=False):
    """-> the table after tf.scatter_add: per id an fp32 accumulator that starts from the widened
    row, one fp32 add per occurrence in increasing p (reverse: in decreasing p, for the tests that
    show the order is observable), one rounding at the end"""
    _check(ids, values, row_index, count)
    out = np.array(table, copy=True)
    rows = out.shape[0]
    acc = {}
    order = range(len(ids) - 1, -1, -1) if reverse else range(len(ids))
    for p in order:
        i = int(ids[p])
        s = source_row(p, values.shape[0], row_index, count)
        if not in_range(i, rows) or s is None:
            continue
        if i not in acc:
            acc[i] = widen(out[i], dt).copy()
        acc[i] = (acc[i] + widen(values[s], vdt)).astype(np.float32)
    for i, a in acc.items():
        out[i] = narrow(a, dt)
    return out


def take(table, dt, ids, clear=False, out_dt=None):
    """-> (out [e, d], the table afterwards): every occurrence reads the table as it was before
    the call; an id that names no row reads +0; clear zeroes the named rows"""
    out_dt = out_dt or dt
    rows, d = table.shape
    out = zeros((len(ids), d), out_dt)
    after = np.array(table, copy=True)
    for p, i in enumerate(ids):
        if in_range(int(i), rows):
            out[p] = convert(table[int(i)], dt, out_dt)
            if clear:
                after[int(i)] = 0
    return out, after


def materialise(values, m_rows, row_index=None, count=None):
    """(values [e, d], ids mask) of the plain form equivalent to a row_index / count call:
    -> the [e, d] block and a bool [e] of the occurrences that stay"""
    e = len(row_index) if row_index is not None else m_rows * count
    block = np.zeros((e,) + values.shape[1:], values.dtype)
    keep = np.zeros(e, bool)
    for p in range(e):
        s = source_row(p, values.shape[0], row_index, count)
        if s is not None:
            block[p], keep[p] = values[s], True
    return block, keep


def same(a, b):
    """bit equality of two stored arrays"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    v = np.uint32 if a.dtype == np.float32 else np.uint16
    return np.array_equal(a.view(v), b.view(v))


def sensitive_values(rng, shape):
    """source rows whose fp32 sum depends on the order: (U(0, 1) * 8 - 4) * 10^k, k in [-3, 3]"""
    return ((rng.random(shape) * 8 - 4) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32)


def add_chain_error(table, ids, values, row_index=None, count=None):
    """For an fp32 table: per (distinct id, column) the error of the fp32 chain against the
    float64 sum and its bound gamma(L + 1) * sum |terms| (L occurrences, the terms being the old
    element and the L source elements).  -> (err, bound) arrays over the touched rows"""
    got = add(table, "f32", ids, values, "f32", row_index, count)
    rows = table.shape[0]
    exact, mag, n = {}, {}, {}
    for p, i in enumerate(ids):
        i = int(i)
        s = source_row(p, values.shape[0], row_index, count)
        if not in_range(i, rows) or s is None:
            continue
        if i not in exact:
            exact[i], mag[i], n[i] = table[i].astype(np.float64), np.abs(table[i].astype(np.float64)), 0
        exact[i] = exact[i] + values[s].astype(np.float64)
        mag[i] = mag[i] + np.abs(values[s].astype(np.float64))
        n[i] += 1
    keys = sorted(exact)
    err = np.stack([np.abs(got[i].astype(np.float64) - exact[i]) for i in keys])
    bound = np.stack([gamma(n[i] + 1) * mag[i] for i in keys])
    return err, bound


# ---- the inputs the host check and the GPU tests share ------------------------------------------
PATTERNS = ("distinct", "equal", "hubs", "sorted", "reversed", "random")


def id_pattern(rng, name, rows, e):
    """int64 [e] in [0, rows): all distinct (as far as rows allows), all equal (one segment: the
    chain order), two hubs plus singletons, already sorted, reverse sorted, random"""
    if name == "distinct":
        ids = np.concatenate([rng.permutation(rows) for _ in range(e // rows + 1)])[:e]
    elif name == "equal":
        ids = np.full(e, rows // 2)
    elif name == "hubs":
        ids = rng.integers(0, rows, e)
        ids[::3], ids[1::3] = 0, rows - 1
    else:
        ids = rng.integers(0, rows, e)
        if name != "random":
            ids = np.sort(ids)[::-1 if name == "reversed" else 1]
    return np.array(ids, np.int64, order="C")                       # (a copy: no negative stride survives)


def bad_ids(rows):
    """ids that name no row"""
    return [-1, rows, 2 ** 40, -2 ** 63]


def with_bad_ids(ids, rows, every=5):
    """a copy with every `every`-th id (from position 2) replaced by an id that names no row"""
    ids = ids.copy()
    bad = bad_ids(rows)
    for n, p in enumerate(range(2, len(ids), every)):
        ids[p] = bad[n % len(bad)]
    return ids
