"""Where a table past 2^31 elements / 2^32 bytes can go wrong, as plain numpy: the rows of a
[n_elems // d, d] view that sit at the 32-bit boundaries of an element or byte offset, where a
narrowed offset of such a row would land instead, and the renumbering of ids onto a small table of
those rows alone.  Nothing here touches a GPU or imports euler_amd; tests/test_big_offsets_host.py
checks it and tests/test_big_offsets_gpu.py uses it.

An op of this project depends on the contents of the rows its ids name and on the order of the
occurrences, never on the row numbers.  So the expected result of an op on an 8 GiB table of which
only the probe rows are non-zero is the op's reference on the small table of the probe rows, with
the ids renumbered by `compact`."""
import numpy as np

DIMS = (136, 132, 129)                    # the 8-wide, 4-wide and element chunk paths; no power of two
EDGE_DIM = 520                            # the per-edge block: e = 2^23 + 5 rows of 520
EDGE_ROWS = (1 << 23) + 5
BIG = (1 << 32) + (1 << 20)               # elements of a full buffer
HALF = (1 << 31) + (1 << 20)              # elements of the table Adam's two fp32 states are built over
BUF = max(BIG, EDGE_ROWS * EDGE_DIM)      # elements of a buffer: the per-edge block needs 1.6% more than BIG
ELEM_BYTES = {"f32": 4, "bf16": 2, "f16": 2}
MODULI = ("2^31 elements", "2^32 elements", "2^32 bytes")


def boundaries(elem_bytes):
    """element offsets at which a 32-bit element or byte offset wraps: 2^31 (signed), 2^32 (unsigned),
    and for 4-byte elements 2^30 (byte offset 2^32).  The byte boundaries 2^32 and 2^33 of 2-byte and
    4-byte elements coincide with these."""
    return ((1 << 30,) if elem_bytes == 4 else ()) + (1 << 31, 1 << 32)


def probe_rows(n_elems, d, elem_bytes):
    """the rows of a [n_elems // d, d] view that matter, sorted: rows 0 and 1, the last two, and per
    boundary B the row that straddles (or ends at) B with its two neighbours"""
    rows = n_elems // d
    want = {0, 1, rows - 2, rows - 1}
    for b in boundaries(elem_bytes):
        want |= {b // d - 1, b // d, b // d + 1}
    return np.array(sorted(r for r in want if 0 <= r < rows), np.int64)


def wrapped_offsets(off, elem_bytes):
    """the element offset a narrowed `off` becomes, one per entry of MODULI"""
    off = int(off)
    return (off % (1 << 31), off % (1 << 32), (off * elem_bytes % (1 << 32)) // elem_bytes)


def alias_rows(rows, d, elem_bytes):
    """{row: the sorted rows a wrapped access to it would land in}: for the offsets of the row's first
    and last element, each taken modulo 2^31 elements, 2^32 elements and 2^32 bytes.  A row below
    every modulus aliases only itself."""
    out = {}
    for r in rows:
        r = int(r)
        hit = set()
        for off in (r * d, r * d + d - 1):
            hit |= {w // d for w in wrapped_offsets(off, elem_bytes)}
        out[r] = sorted(hit)
    return out


def straddling_row(boundary, d):
    """the row that holds element boundary - 1; it straddles the boundary unless d divides it"""
    return (boundary - 1) // d


def compact(ids, probe, rows):
    """ids over a [rows, d] table -> ids over the small table that holds only the rows `probe`
    (sorted), in order.  An id that names no row (< 0 or >= rows) keeps naming none: a negative id
    stays, an id >= rows keeps its distance past the end.  An id in [0, rows) that is no probe row
    is an error: the small table could not answer for it."""
    probe = np.asarray(probe, np.int64)
    ids = np.asarray(ids, np.int64)
    assert np.all(np.diff(probe) > 0) and probe[0] >= 0 and probe[-1] < rows
    pos = np.minimum(np.searchsorted(probe, ids), len(probe) - 1)
    hit = probe[pos] == ids
    inside = (ids >= 0) & (ids < rows)
    if np.any(inside & ~hit):
        raise ValueError("compact: id %d names a row that is no probe row" % ids[inside & ~hit][0])
    return np.where(hit, pos, np.where(ids >= rows, ids - rows + len(probe), ids)).astype(np.int64)


def expand(small_ids, probe, rows):
    """the inverse of compact"""
    probe = np.asarray(probe, np.int64)
    small_ids = np.asarray(small_ids, np.int64)
    n = len(probe)
    inside = (small_ids >= 0) & (small_ids < n)
    return np.where(inside, probe[np.clip(small_ids, 0, n - 1)],
                    np.where(small_ids >= n, small_ids - n + rows, small_ids)).astype(np.int64)


def no_row_ids(rows):
    """ids that name no row of a [rows, d] table"""
    return [-1, rows, rows + 5, (1 << 33) + 5]


def probe_values(rng, n, d):
    """float32 [n, d], every element non-zero in [-4, 4] and a multiple of 2^-5 (so bf16, fp16 and
    fp32 all hold it exactly): sign * k / 32 with k in 1 .. 128"""
    k = rng.integers(1, 129, (n, d)).astype(np.float32)
    return (np.where(rng.random((n, d)) < 0.5, -1, 1) * k / 32).astype(np.float32)


def named_twice(rng, probe, extra=(), repeat=2, total=None):
    """a shuffled int64 id list that names every probe row `repeat` times, then `extra`, padded with
    random probe rows to `total`"""
    ids = list(np.repeat(np.asarray(probe, np.int64), repeat)) + [int(x) for x in extra]
    if total is not None:
        assert total >= len(ids)
        ids += [int(x) for x in rng.choice(probe, total - len(ids))]
    ids = np.array(ids, np.int64)
    rng.shuffle(ids)
    return ids


SEARCH_Q, SEARCH_K = 33, 64               # two query tiles; more entries than probe rows: zero rows fill the tail


def boundary_rows(n_elems, d, elem_bytes):
    """the probe rows that straddle a boundary, then the last row"""
    rows = n_elems // d
    return np.array([straddling_row(b, d) for b in boundaries(elem_bytes) if b < rows * d] + [rows - 1], np.int64)


def zero_rows(probe, rows):
    """three rows that are no probe row: the lowest (the first to fill the tail of a list), one a
    third into the table, one just before the last two"""
    low = int(np.setdiff1d(np.arange(len(probe) + 1), probe)[0])
    out = [low, rows // 3, rows - 3]
    assert not np.isin(out, probe).any() and low < rows // 3 < rows - 3
    return out


def search_case(rng, probe, values, n_elems, d, elem_bytes):
    """what table_topk / table_rank are asked over the big table -> (queries [33, d] float32, exclude
    [33], target [33]).  Queries: every probe row (the rows at the boundaries among them), a zero row,
    random rows.  exclude: a probe query's own row (every second one), else in turn a boundary row, a
    zero row, -1 and rows + 5.  target: in turn a boundary row, a zero row, -1 and rows."""
    rows, p, q = n_elems // d, len(probe), SEARCH_Q
    edge, zero = boundary_rows(n_elems, d, elem_bytes).tolist(), zero_rows(probe, rows)
    assert p + 2 <= q and set(edge) <= set(int(x) for x in probe)
    queries = np.concatenate([values, np.zeros((1, d), np.float32),
                              rng.standard_normal((q - p - 1, d)).astype(np.float32)])
    turn_e, turn_t = edge + zero + [-1, rows + 5], edge + zero[:2] + [-1, rows]
    exclude = np.array([turn_e[i % len(turn_e)] for i in range(q)], np.int64)
    exclude[:p:2] = probe[::2]
    target = np.array([turn_t[(i + 3) % len(turn_t)] for i in range(q)], np.int64)
    return queries, exclude, target


def wrapped_read(values, probe, d, row, elem_bytes):
    """what a read of `row` through each narrowed offset of its first element returns, on a table
    whose probe rows hold `values` and whose other rows are zero -> one [d] array per modulus"""
    probe = [int(p) for p in probe]
    at = {p: values[n] for n, p in enumerate(probe)}
    out = []
    for w in wrapped_offsets(row * d, elem_bytes):
        flat = np.concatenate([at.get(w // d, np.zeros(d, values.dtype)),
                               at.get(w // d + 1, np.zeros(d, values.dtype))])
        out.append(flat[w % d:w % d + d])
    return out
