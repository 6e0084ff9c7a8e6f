"""CPU-only proof, from the oracle and the host models of id_plumbing_cases.py alone, that the
cases of test_id_plumbing_gpu.py reach the paths they are named after: the probe wrap and the
capacity step of the ID_UNIQUE table, the 16-lane loop and the grid-stride loops of the gather
and merge kernels, the wave and block boundaries of the split, the chunk boundaries and the
second hash round of the front end - and that the row-count model of the front end holds
against a sequential emulation of its two mark passes."""
import numpy as np
import pytest

import id_plumbing_cases as IC


def test_mix64_restatement(O):
    """the models' hash == the oracle's numpy restatement (itself checked against the C)"""
    p = O.synth_params(1, 10, 10, hashed_ids=True)
    x = IC.u64([0, 1, 2, 63, 5000, 1 << 32, 1 << 63, IC.ALL_ONES, IC.GOLDEN2], IC.distinct_ids(50, 3))
    want = O.synth_external_ids(p, x)
    assert [IC.mix64(int(v)) for v in x] == [int(v) for v in want]
    assert np.array_equal(IC.mix64_np(x), want)
    for cap in (64, 1024, 1 << 23):
        assert IC.slot1_np(x, cap).tolist() == [IC.slot1(int(v), cap) for v in x]
        assert IC.slot2_np(x, cap).tolist() == [IC.slot2(int(v), cap) for v in x]
        assert IC.slot1_np(x, cap).max() < cap and IC.slot2_np(x, cap).max() < cap


def test_table_sizes():
    assert [IC.unique_cap(n) for n in (0, 1, 32, 33, 64, 65, 257)] == [64, 64, 64, 128, 128, 256, 1024]
    assert [IC.front_cap(n) for n in (0, 1, 240, 256, 257, 2048, 2049)] == \
        [1024, 1024, 1024, 1024, 2048, 8192, 16384]


# ---- A. id_unique ---------------------------------------------------------------------------
def test_unique_cases_shape(O):
    c = IC.unique_cases()
    assert len(c["n0"]) == 0 and len(c["n1"]) == 1 and c["n1_all_ones"].tolist() == [IC.ALL_ONES]
    for n in (32, 33, 255, 256, 257, 70001):
        ids = c["distinct_%d" % n]
        assert len(ids) == n == len(np.unique(ids)) and IC.ALL_ONES not in ids
    assert IC.unique_cap(32) == 64 and IC.unique_cap(33) == 128      # the capacity step
    for name in ("same_257", "all_ones_257"):
        uq, gi = O.id_unique(c[name])
        assert len(c[name]) == 257 and len(uq) == 1 and not gi.any()
    assert (c["all_ones_257"] == IC.ALL_ONES).all()
    assert c["all_ones_first"][0] == IC.ALL_ONES and c["all_ones_last"][-1] == IC.ALL_ONES
    uq, _ = O.id_unique(c["bit63"])
    assert uq.tolist() == [5, 5 | 1 << 63, 0, 1 << 63]
    uq, _ = O.id_unique(c["high_bits"])
    assert len(uq) == 6 and len(np.unique(uq & np.uint64(0xFFFFFFFF))) == 2
    uq, gi = O.id_unique(c["pool3_70001"])
    assert len(uq) == 3 and len(gi) == 70001 > 256 * 256      # more than one workgroup, an odd tail
    assert IC.ALL_ONES in uq


def test_oracle_answers_empty_inputs(O):
    uq, gi = O.id_unique(IC.u64())
    assert len(uq) == 0 and len(gi) == 0
    for parts, shards in IC.SPLIT_SHAPES:
        off, sid, mi = O.id_split(IC.split_ids(0), parts, shards)
        assert off.tolist() == [0] * (shards + 1) and len(sid) == 0 and len(mi) == 0
    assert O.idx_gather(IC.seg_idx(IC.SEG_LENS), []).shape == (0, 2)


def test_probe_wrap_case(O):
    ids = IC.probe_wrap_ids()
    assert len(ids) == 32 and IC.unique_cap(len(ids)) == 64
    home = ids[:15]
    assert len(np.unique(home)) == 15 and (ids[17:] == home[::-1]).all()
    assert (ids[15:17] == IC.ALL_ONES).all()
    assert all(IC.mix64(int(v)) & 63 == 63 for v in home)     # one home: the table's last slot
    assert home.max() <= 5000
    uq, gi = O.id_unique(ids)
    assert uq.tolist() == home.tolist() + [IC.ALL_ONES]
    assert gi.tolist() == list(range(15)) + [15, 15] + list(range(14, -1, -1))


# ---- B. gathers -----------------------------------------------------------------------------
def test_gather_cases_shape(O):
    idx = IC.seg_idx(IC.SEG_LENS)
    lens = (idx[:, 1] - idx[:, 0]).tolist()
    assert lens == [0, 1, 15, 16, 17, 33, 0] and idx[-1, 1] == 82
    # the 16 lanes of a row: fewer entries than lanes, exactly one step, one entry into the second, the third
    assert {(l + 15) // 16 for l in lens} == {0, 1, 2, 3}
    for name, g in IC.GATHERS.items():
        out = O.idx_gather(idx, g)
        assert np.array_equal(out[:, 1] - out[:, 0], np.asarray(lens, np.int32)[g])
    assert O.idx_gather(idx, IC.GATHERS["only_empty"]).max() == 0
    assert len(set(IC.GATHERS["repeats"])) < len(IC.GATHERS["repeats"])
    for dt in IC.GATHER_DTYPES:
        data = IC.gather_data(dt, 82)
        assert data.dtype == np.dtype(dt) and len(data) == 82
        got = O.data_gather(data, idx, IC.GATHERS["reverse"])
        want = np.concatenate([data[b:e] for b, e in idx[::-1]])
        assert np.array_equal(IC.bits_of(got), IC.bits_of(want))
    for dt, nan_bits, neg0 in (("float32", 0xFFC12345, 0x80000000),
                               ("float64", 0xFFF8000012345678, 1 << 63)):
        data = IC.gather_data(dt, 82)
        b = IC.bits_of(data)
        assert np.isnan(data).sum() >= 4 and np.isinf(data).sum() >= 2
        assert nan_bits in b and neg0 in b           # a payload, the negative zero: only bits tell


def test_big_gather_reaches_the_stride_loop(O):
    idx, g = IC.big_gather_case()
    # 16 lanes a row, GridFor caps the launch: rows beyond this wait for a second pass
    rows_per_pass = IC.GRID_CAP_THREADS // 16
    assert rows_per_pass == 65536 < len(g) == IC.BIG_GATHER_ROWS
    assert len(g) % rows_per_pass not in (0, rows_per_pass - 1)
    lens = idx[:, 1] - idx[:, 0]
    assert set(lens.tolist()) == {0, 1, 2, 3}
    assert lens[g[rows_per_pass:]].sum() > 1000      # the second pass has entries to move


def test_idx_gather_total_edge(O):
    """the totals of B.5: 2^30 and 2^31 - 1 are answered, 2^31 is the refusal's"""
    one = np.array([[0, 2 ** 30]], np.int32)
    assert O.idx_gather(one, [0])[0].tolist() == [0, 2 ** 30]
    two = np.array([[0, 2 ** 30], [0, 2 ** 30 - 1]], np.int32)
    assert O.idx_gather(two, [0, 1]).tolist() == [[0, 2 ** 30], [2 ** 30, 2 ** 31 - 1]]


def test_sparse_cases_shape(O):
    c = IC.sparse_cases()
    gi, ind, val, shape = c["row_of_40_int64"]
    assert (np.diff(ind[:, 0]) >= 0).all() and (np.bincount(ind[:, 0]) == 40).any()
    oi, ov, os_ = O.sparse_gather(gi, ind, val, shape)
    assert len(ov) == 3 * 40 + 17 + 3 + 1 and os_.tolist() == [len(gi), 50]
    val = c["float64_values"][2]
    assert val.dtype == np.float64 and np.isnan(val).any()
    ov = O.sparse_gather(gi, ind, val, shape)[1]          # the restatement keeps NaN payloads
    assert np.array_equal(IC.bits_of(ov), O.sparse_gather(gi, ind, IC.bits_of(val), shape)[1])
    gi, ind, val, shape = c["nnz0"]
    oi, ov, os_ = O.sparse_gather(gi, ind, val, shape)
    assert oi.shape == (0, 2) and len(ov) == 0 and os_.tolist() == [3, 50]


# ---- C. split / merge -----------------------------------------------------------------------
@pytest.mark.parametrize("parts,shards", IC.SPLIT_SHAPES, ids=str)
def test_split_cases_shape(O, parts, shards):
    ids = IC.split_ids(513)
    assert (ids >= 1 << 63).sum() > 100 and (ids == IC.ALL_ONES).sum() > 10 and ids[-1] == IC.ALL_ONES
    own = O.shard_of(ids, parts, shards)
    want = [(int(v) % parts) % shards for v in ids]            # unsigned, in Python integers
    assert own.tolist() == want
    signed = [(int(v) % parts) % shards for v in ids.view(np.int64)]
    if parts not in (1, 64):
        assert signed != want, "the ids at and above 2^63 tell signed from unsigned owners"
    off, sid, mi = O.id_split(ids, parts, shards)
    assert off[0] == 0 and off[-1] == 513 and np.array_equal(sid, ids[mi])
    for s in range(shards):                                    # stable: positions ascend in a bucket
        assert (np.diff(mi[off[s]:off[s + 1]]) > 0).all()
    counts = np.diff(off)
    if (parts, shards) == (64, 64):
        assert (counts > 0).sum() > 48                         # nearly every one of kMaxShards buckets
    if (parts, shards) == (3, 64):
        assert (counts[3:] == 0).all() and (counts[:3] > 0).all()      # shards > partitions: empty buckets
    assert IC.MAX_SHARDS == 64


def test_one_owner_full_wave(O):
    for parts, shards in ((7, 2), (64, 64)):
        ids = IC.one_owner_ids(513, parts, shards)
        assert not O.shard_of(ids, parts, shards).any() and len(np.unique(ids)) > 500
        off, sid, mi = O.id_split(ids, parts, shards)
        assert off.tolist() == [0] + [513] * shards and mi.tolist() == list(range(513))


def test_big_merge_reaches_the_stride_loop():
    words = IC.BIG_MERGE_ROWS * IC.BIG_MERGE_WORDS
    assert IC.GRID_CAP_THREADS == 1048576 < words < 2 * IC.GRID_CAP_THREADS
    assert words % IC.GRID_CAP_THREADS % 256 != 0          # and the tail is no whole workgroup


# ---- D. front end ---------------------------------------------------------------------------
def _emulated(eff, cap, seeds=200, stale=False):
    out = []
    for seed in range(seeds):
        rng = np.random.default_rng(seed)
        junk = rng.integers(0, 1 << 32, cap) if stale else None
        if stale and seed % 2:
            junk = rng.integers(0, max(len(eff), 1), cap)      # stale entries that name live positions
        out.append(IC.emulate_front_rows(eff, cap, rng, junk))
    return out


def test_round2_case_model():
    ids = IC.round2_ids()
    assert len(ids) == 6 == len(np.unique(ids)) and ids.max() <= 200000
    case = IC.round2_case()
    assert len(case) == 240 and IC.front_cap(len(case)) == 1024
    assert len(set(IC.slot1(int(v), 1024) for v in ids)) == 1
    assert len(set(IC.slot2(int(v), 1024) for v in ids)) == 6
    assert IC.dedup_row_bounds(case, 1024) == (6, 6)
    for stale in (False, True):
        assert set(_emulated(case, 1024, stale=stale)) == {6}
    # without the second round: the winner of round 1 merges, the other five ids do not
    assert 1 + 5 * IC.ROUND2_COPIES == 201
    ids2048 = IC.round2_ids(2048)
    assert len(set(IC.slot1_np(ids2048, 2048))) == 1 and len(set(IC.slot2_np(ids2048, 2048))) == 6


def test_double_collision_case_model():
    a, b, c = (int(v) for v in IC.double_collision_ids())
    assert IC.slot1(a, 1024) == IC.slot1(b, 1024) == IC.slot1(c, 1024)
    assert IC.slot2(b, 1024) == IC.slot2(c, 1024) != IC.slot2(a, 1024)
    case = IC.double_collision_case()
    k = IC.ROUND2_COPIES
    assert len(case) == 3 * k and IC.front_cap(len(case)) == 1024
    lo, hi = IC.dedup_row_bounds(case, 1024)
    assert (lo, hi) == (3, 1 + 2 * k)
    # who wins round 1 decides: b or c -> the other is the only writer of the shared round-2
    # slot, 3 rows; a -> b and c fight over it, the loser keeps a row per position, 2 + k
    for stale in (False, True):
        rows = _emulated(case, 1024, stale=stale)
        assert set(rows) == {3, 2 + k}
        assert all(lo <= r <= hi for r in rows)


@pytest.mark.parametrize("n", IC.FRONT_SIZES)
def test_front_size_cases_model(n):
    """chunk boundaries: 2047 / 2048 / 2049 positions are one chunk short of full, one full, one
    full plus a second of one position; the bounds of the pooled and the distinct draw"""
    chunks = (n + IC.FRONT_CHUNK - 1) // IC.FRONT_CHUNK
    assert chunks == {0: 0, 1: 1, 2047: 1, 2048: 1, 2049: 2, 4097: 3}[n]
    cap = IC.front_cap(n)
    pooled = IC.pool_ids(n, 50, 51)
    assert len(pooled) == n and len(np.unique(pooled)) == min(n, 50)
    lo, hi = IC.dedup_row_bounds(pooled, cap)
    assert lo == min(n, 50) <= hi
    distinct = IC.distinct_ids(n, 53)
    assert IC.dedup_row_bounds(distinct, cap) == (n, n)       # one position each: nothing to merge
    if n in (1, 2049):
        rows = _emulated(pooled, cap, seeds=3, stale=True)
        assert all(lo <= r <= hi for r in rows)


def test_row_bounds_hold_under_emulation():
    """a pool crowded into a small table (many shared slots in both rounds): the emulated row
    count stays inside the model's bounds, with and without stale second-table entries"""
    rng = np.random.default_rng(61)
    ids = rng.choice(np.arange(1, 400, dtype=np.uint64), 1000)
    lo, hi = IC.dedup_row_bounds(ids, 1024)
    assert lo < hi, "the case must have contested ids"
    rows = _emulated(ids, 1024, seeds=200, stale=True) + _emulated(ids, 1024, seeds=20)
    assert all(lo <= r <= hi for r in rows) and len(set(rows)) > 1


def test_mask_and_dense_cases_shape():
    m = IC.mask_cases()
    for name, (ids, mask, group) in m.items():
        assert len(mask) == (len(ids) + group - 1) // group
        eff = IC.effective_ids(ids, mask, group)
        assert ((eff == 0) | (eff == ids)).all()
    ids, mask, group = m["all_set"]
    assert len(ids) == 25 and len(mask) == 3 and not IC.effective_ids(ids, mask, group).any()
    ids, mask, group = m["middle_set"]
    assert np.flatnonzero(IC.effective_ids(ids, mask, group) == 0).tolist() == list(range(10, 20))
    ids, mask, group = m["real_zero_beside_mask"]
    assert np.flatnonzero(IC.effective_ids(ids, mask, group) == 0).tolist() == list(range(9, 21))
    ids, mask, group = m["nonzero_byte"]
    assert np.flatnonzero(IC.effective_ids(ids, mask, group) == 0).tolist() == list(range(20, 25))
    for name, (ids, mask, group) in m.items():       # a few ids in 1024 slots: the row count is exact
        eff = IC.effective_ids(ids, mask, group)
        assert IC.dedup_row_bounds(eff, IC.front_cap(len(ids))) == (len(np.unique(eff)),) * 2, name
    d = IC.dense_cases()
    ids, entries = d["limit_1"]
    assert entries == 2 and set(ids.tolist()) == {0, 1, 5, IC.ALL_ONES}
    ids, entries = d["limit_5"]
    assert entries == 6 and {4, 5, 6} <= set(ids.tolist())


def test_big_front_case_model():
    n = IC.BIG_FRONT_N
    assert n > IC.GRID_CAP_THREADS and n % IC.FRONT_CHUNK == 1 and n % 256 == 1
    ids = IC.pool_ids(n, 3000, 71)
    lo, hi = IC.dedup_row_bounds(ids, IC.front_cap(n))
    assert lo == 3000 and hi == lo, "4 M slots for 3000 ids: the model expects every id merged"


# ---- E. wire rows ---------------------------------------------------------------------------
def test_wire_cases_shape():
    ids, w, t, mask = IC.wire_rows(7, 3)
    assert (ids == -1).any() and (ids == -2 ** 63).any() and (t == -1).any()
    wb = IC.bits_of(w)
    assert 0x80000000 in wb and 0xFFC12345 in wb and 0x7F800000 in wb
    assert mask.any() and not mask.all()
    pos = IC.wire_pos(7, 20)
    assert len(np.unique(pos)) < len(pos) and len(np.unique(pos)) < 7 and pos.max() < 7 and pos.min() >= 0
    assert len(IC.wire_pos(1, 0)) == 0 and not IC.wire_pos(1, 5).any()
