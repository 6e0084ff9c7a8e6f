"""A plain reference of the feature fetch and edge lookup ops: Python dicts and loops over numpy
arrays, nothing of the library or the oracle.  A table is what the library takes: `ptr [n + 1]`
(first value of each record), `idx [n * slots]` (slot ends relative to the record's first value)
and `val`; a slot that is missing or empty has no values.

  dense        tf_euler get_dense_feature: [n, dim] float32, a short slot zero-padded, a long one
               truncated, a zero row for row -1 or a slot id outside [0, slots)
  sparse       tf_euler get_sparse_feature: (indices [nnz, 2], values [nnz], [n, max_len]); a row
               without values is the one entry (i, 0) = default
  sparse_core  the GQL values() form: ([n, 2] int32 offsets, values), no default entries
  binary       (offsets [n + 1], bytes)
  rows_of / ordinals   the id -> row and (src, dst, type) -> ordinal lookups, -1 when unknown
"""
import numpy as np


class Table:
    def __init__(self, slots, ptr, idx, val):
        self.slots = int(slots)
        self.ptr = np.asarray(ptr, np.int64)
        self.idx = np.asarray(idx, np.int32).reshape(-1)
        self.val = np.asarray(val)
        self.n = len(self.ptr) - 1
        assert len(self.idx) == self.n * self.slots

    def slot(self, row, fid):
        """The values of slot `fid` of record `row` (a view of val); none when there is no such
        record or slot."""
        if row < 0 or fid < 0 or fid >= self.slots:
            return self.val[:0]
        ends = self.idx[row * self.slots:(row + 1) * self.slots]
        pre = 0 if fid == 0 else int(ends[fid - 1])
        first = int(self.ptr[row])
        return self.val[first + pre:first + int(ends[fid])]

    def is_uniform(self):
        """Every record has record 0's slot ends and its values begin at row * (record 0's
        length): the layout the library stores as one row of ends."""
        if self.n == 0:
            return False
        ends = self.idx.reshape(self.n, self.slots)
        length = int(self.ptr[1] - self.ptr[0])
        return bool((ends == ends[0]).all() and
                    np.array_equal(self.ptr, np.arange(self.n + 1, dtype=np.int64) * length))

    def as_tuple(self):
        """(slots, ptr, idx, val): the `features=` / `sparse_features=` argument of from_csr."""
        return self.slots, self.ptr, self.idx, self.val


def ragged_table(per_record, dtype, slots=None):
    """per_record[r][s] = the values of slot s of record r (any sequence; `bytes` for uint8)."""
    if slots is None:
        slots = max((len(rec) for rec in per_record), default=0)
    ptr, idx, val = [0], [], []
    for rec in per_record:
        end = 0
        for s in range(slots):
            if s < len(rec):
                v = rec[s]
                v = np.frombuffer(v, np.uint8) if isinstance(v, (bytes, bytearray)) else np.asarray(v, dtype)
                val.append(v.reshape(-1))
                end += v.size
            idx.append(end)
        ptr.append(ptr[-1] + end)
    flat = np.concatenate(val).astype(dtype) if val else np.zeros(0, dtype)
    return Table(slots, ptr, idx, flat)


def uniform_table(arrays, dtype):
    """One [n, d] array per slot: every record has d values in that slot."""
    arrays = [np.asarray(a, dtype) for a in arrays]
    n = len(arrays[0])
    ends = np.cumsum([a.shape[1] for a in arrays])
    val = np.concatenate(arrays, 1).reshape(-1)
    return Table(len(arrays), np.arange(n + 1, dtype=np.int64) * int(ends[-1]),
                 np.tile(ends.astype(np.int32), n), val)


def rows_of(ids, queries):
    """Row of each queried id (ids and queries compared as uint64), -1 for an unknown id; a
    repeated id keeps its last row."""
    where = {}
    for r, i in enumerate(np.asarray(ids).astype(np.uint64).tolist()):
        where[i] = r
    q = np.asarray(queries).astype(np.uint64).tolist()
    return np.array([where.get(i, -1) for i in q], np.int64).reshape(-1)


def ordinals(src, dst, type, queries):
    """Ordinal of each queried (src, dst, type) row of `queries` [n, 3] int64 (ids compared as
    uint64), -1 when there is no such record."""
    where = {}
    s = np.asarray(src).astype(np.uint64).tolist()
    d = np.asarray(dst).astype(np.uint64).tolist()
    t = np.asarray(type).astype(np.int64).tolist()
    for o in range(len(s)):
        where[(s[o], d[o], t[o])] = o
    q = np.asarray(queries, np.int64).reshape(-1, 3)
    qs = q[:, 0].astype(np.uint64).tolist()
    qd = q[:, 1].astype(np.uint64).tolist()
    qt = q[:, 2].tolist()
    return np.array([where.get(k, -1) for k in zip(qs, qd, qt)], np.int64).reshape(-1)


def dense(table, rows, fid, dim):
    rows = np.asarray(rows, np.int64)
    out = np.zeros((len(rows), dim), np.float32)
    for i, r in enumerate(rows.tolist()):
        v = table.slot(r, fid)[:dim]
        out[i, :len(v)] = v
    return out


def sparse(table, rows, fid, default):
    rows = np.asarray(rows, np.int64)
    ind, val, max_len = [], [], 0
    for i, r in enumerate(rows.tolist()):
        v = table.slot(r, fid).astype(np.uint64).astype(np.int64)   # the op's int64 view
        if len(v) == 0:
            v = np.array([default], np.int64)
        ind.append(np.stack([np.full(len(v), i, np.int64), np.arange(len(v), dtype=np.int64)], 1))
        val.append(v)
        max_len = max(max_len, len(v))
    if not ind:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64), [0, 0]
    return np.concatenate(ind), np.concatenate(val), [len(rows), max_len]


def sparse_core(table, rows, fid):
    rows = np.asarray(rows, np.int64)
    idx = np.zeros((len(rows), 2), np.int32)
    val, at = [], 0
    for i, r in enumerate(rows.tolist()):
        v = table.slot(r, fid)
        idx[i] = (at, at + len(v))
        at += len(v)
        val.append(v)
    flat = np.concatenate(val) if val else np.zeros(0, np.uint64)
    return idx, flat.astype(np.uint64).astype(np.int64)


def binary(table, rows, fid):
    rows = np.asarray(rows, np.int64)
    off = np.zeros(len(rows) + 1, np.int64)
    val = []
    for i, r in enumerate(rows.tolist()):
        v = table.slot(r, fid)
        off[i + 1] = off[i] + len(v)
        val.append(v)
    return off, (np.concatenate(val) if val else np.zeros(0, np.uint8)).astype(np.uint8)


def row_offsets(indices, n):
    """The offsets [n + 1] that a sparse result's row indices imply."""
    counts = np.bincount(np.asarray(indices)[:, 0], minlength=n) if n else np.zeros(0, np.int64)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(counts)
    return off
