"""The id-plumbing kernels at their edges (euler_amd/csrc/mp_kernels.hip: ID_UNIQUE, IDX_GATHER /
DATA_GATHER, ID_SPLIT, IDX_MERGE / DATA_MERGE, the fused front end dedup_split / FrontHandle;
sample_kernels.hip: pack_rows / expand_packed / expand_rows) against the oracle.  Every result is
an integer or a bit pattern: ids are compared as the same 64 bits, floats through unsigned views,
nothing has a tolerance.  test_id_plumbing_host.py proves on the CPU that the cases of
id_plumbing_cases.py reach the paths named here."""
import numpy as np
import pytest

import id_plumbing_cases as IC

pytestmark = pytest.mark.gpu

UNIQUE = IC.unique_cases()
MASKS = IC.mask_cases()
DENSE = IC.dense_cases()
SPARSE = IC.sparse_cases()


def t2n(t):
    return t.detach().cpu().numpy()


def dev(torch, a):
    """numpy -> GPU tensor with the same bits (uint64 travels as int64)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.as_tensor(a).cuda()


def u64_of(t):
    return np.ascontiguousarray(t2n(t)).view(np.uint64)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(IC.bits_of(got), IC.bits_of(want))


# ---- A. id_unique ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(UNIQUE))
def test_id_unique(EA, O, torch_cuda, name):
    ids = UNIQUE[name]
    uq_o, gi_o = O.id_unique(ids)
    uq, gi = EA.ops.id_unique(dev(torch_cuda, ids))
    assert gi.dtype == torch_cuda.int32
    assert np.array_equal(u64_of(uq), uq_o)
    assert np.array_equal(t2n(gi), gi_o)


# ---- B. idx_gather / data_gather / sparse_gather ---------------------------------------------
@pytest.mark.parametrize("dtype", IC.GATHER_DTYPES)
def test_data_gather_row_lengths(EA, O, torch_cuda, dtype):
    """rows of 0, 1, 15, 16, 17 and 33 entries under the 16 lanes that serve a row"""
    torch = torch_cuda
    idx = IC.seg_idx(IC.SEG_LENS)
    data = IC.gather_data(dtype, int(idx[-1, 1]))
    d_t, idx_t = dev(torch, data), dev(torch, idx)
    for name, g in IC.GATHERS.items():
        g = np.asarray(g, np.int32)
        want = O.data_gather(data, idx, g)
        oi, total = EA.ops.idx_gather(idx_t, dev(torch, g))
        assert total == len(want) and np.array_equal(t2n(oi), O.idx_gather(idx, g)), name
        out = EA.ops.data_gather(d_t, idx_t, dev(torch, g))
        assert out.dtype == d_t.dtype and tuple(out.shape) == (len(want),), name
        got_b, want_b = IC.bits_of(t2n(out)), IC.bits_of(want)
        bad = sorted({IC.SEG_LENS[s] for s, (b, e) in zip(g, O.idx_gather(idx, g))
                      if not np.array_equal(got_b[b:e], want_b[b:e])})
        assert not bad, "%s: gathered segments of %s entries differ" % (name, bad)
        assert same_bits(t2n(out), want), name
        if name in ("only_empty", "none"):
            assert out.numel() == 0


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_data_gather_grid_stride(EA, O, torch_cuda, dtype):
    """more gathered rows than one pass of the capped grid serves"""
    torch = torch_cuda
    idx, g = IC.big_gather_case()
    data = IC.gather_data(dtype, int(idx[-1, 1]), seed=11)
    out = EA.ops.data_gather(dev(torch, data), dev(torch, idx), dev(torch, g))
    assert same_bits(t2n(out), O.data_gather(data, idx, g))


@pytest.mark.parametrize("dtype", ["int16", "float16", "bfloat16"])
def test_data_gather_refuses_two_byte_elements(EA, torch_cuda, dtype):
    torch = torch_cuda
    idx = dev(torch, IC.seg_idx(IC.SEG_LENS))
    data = torch.arange(82, device="cuda").to(getattr(torch, dtype))
    with pytest.raises(EA._lib.EulerGpuError, match="elem_size"):
        EA.ops.data_gather(data, idx, dev(torch, np.array([1, 2], np.int32)))


def test_idx_gather_total_at_int32_edge(EA, O, torch_cuda):
    """offsets up to 2^31 - 1 are answered, a total of 2^31 is refused (the oracle wraps there)"""
    torch = torch_cuda
    one = np.array([[0, 2 ** 30]], np.int32)
    oi, total = EA.ops.idx_gather(dev(torch, one), dev(torch, np.array([0], np.int32)))
    assert total == 2 ** 30 and np.array_equal(t2n(oi), O.idx_gather(one, [0]))
    with pytest.raises(EA._lib.EulerGpuError, match="2\\^31"):
        EA.ops.idx_gather(dev(torch, one), dev(torch, np.array([0, 0], np.int32)))
    two = np.array([[0, 2 ** 30], [0, 2 ** 30 - 1]], np.int32)
    oi, total = EA.ops.idx_gather(dev(torch, two), dev(torch, np.array([0, 1], np.int32)))
    assert total == 2 ** 31 - 1 and np.array_equal(t2n(oi), O.idx_gather(two, [0, 1]))
    oi, total = EA.ops.idx_gather(dev(torch, two), dev(torch, np.zeros(0, np.int32)))
    assert total == 0 and tuple(oi.shape) == (0, 2)


@pytest.mark.parametrize("name", sorted(SPARSE))
def test_sparse_gather(EA, O, torch_cuda, name):
    torch = torch_cuda
    gi, ind, val, shape = SPARSE[name]
    oi_o, ov_o, os_o = O.sparse_gather(gi, ind, val, shape)
    oi, ov, os_ = EA.ops.sparse_gather(dev(torch, gi), dev(torch, ind), dev(torch, val), shape)
    assert oi.dtype == torch.int64 and np.array_equal(t2n(oi), oi_o)
    assert same_bits(t2n(ov), ov_o)
    assert np.array_equal(t2n(os_), os_o)


# ---- C. id_split / merge_rows -----------------------------------------------------------------
def _check_split(EA, O, torch, ids, parts, shards):
    off_o, sid_o, mi_o = O.id_split(ids, parts, shards)
    off, sid, mi = EA.ops.id_split(dev(torch, ids), parts, shards)
    what = "n=%d (%d, %d)" % (len(ids), parts, shards)
    assert list(off) == off_o.tolist(), what
    assert np.array_equal(u64_of(sid), sid_o), what
    assert mi.dtype == torch.int32 and np.array_equal(t2n(mi), mi_o), what


@pytest.mark.parametrize("parts,shards", IC.SPLIT_SHAPES, ids=str)
def test_id_split_wave_and_block_boundaries(EA, O, torch_cuda, parts, shards):
    """bit-exact offsets, ids and merge index: the stable order of the reference"""
    for n in IC.SPLIT_SIZES:
        _check_split(EA, O, torch_cuda, IC.split_ids(n), parts, shards)


@pytest.mark.parametrize("parts,shards", [(7, 2), (64, 64), (1, 1)], ids=str)
def test_id_split_one_owner_in_every_lane(EA, O, torch_cuda, parts, shards):
    _check_split(EA, O, torch_cuda, IC.one_owner_ids(513, parts, shards), parts, shards)


def test_id_split_refusals(EA, torch_cuda):
    ids = dev(torch_cuda, IC.split_ids(65))
    for parts, shards in ((8, 0), (8, 65), (0, 8)):
        with pytest.raises(EA._lib.EulerGpuError, match="id_split"):
            EA.ops.id_split(ids, parts, shards)


@pytest.fixture(scope="module")
def merge_index(O):
    ids = IC.split_ids(257)
    return O.id_split(ids, 7, 2)[2]


@pytest.mark.parametrize("dtype,cols", [("int32", None), ("int64", None), ("int32", 3), ("float64", 5)],
                         ids=str)
def test_merge_rows(EA, torch_cuda, merge_index, dtype, cols):
    torch = torch_cuda
    n = len(merge_index)
    rows = IC.gather_data(dtype, n * (cols or 1), seed=13)
    rows = rows.reshape(n, cols) if cols else rows
    merged = t2n(EA.ops.merge_rows(dev(torch, rows), dev(torch, merge_index)))
    assert same_bits(merged[merge_index], rows)
    inverse = np.empty(n, np.int64)
    inverse[merge_index] = np.arange(n)
    assert same_bits(merged, rows[inverse])


def test_merge_rows_grid_stride(EA, torch_cuda):
    """more words than one pass of the capped grid moves; the reversing permutation"""
    torch = torch_cuda
    n, words = IC.BIG_MERGE_ROWS, IC.BIG_MERGE_WORDS
    rows = np.arange(n * words, dtype=np.int32).reshape(n, words) * np.int32(7) - np.int32(3)
    mi = np.arange(n - 1, -1, -1, dtype=np.int32)
    merged = t2n(EA.ops.merge_rows(dev(torch, rows), dev(torch, mi)))
    assert np.array_equal(merged, rows[::-1])


def test_merge_rows_empty_and_refusal(EA, torch_cuda):
    torch = torch_cuda
    empty = EA.ops.merge_rows(torch.empty((0, 3), dtype=torch.int32, device="cuda"),
                              torch.empty(0, dtype=torch.int32, device="cuda"))
    assert tuple(empty.shape) == (0, 3)
    with pytest.raises(EA._lib.EulerGpuError, match="multiple of 4"):
        EA.ops.merge_rows(torch.zeros((5, 1), dtype=torch.int16, device="cuda"),
                          torch.arange(5, dtype=torch.int32, device="cuda"))


# ---- D. dedup_split / FrontHandle -------------------------------------------------------------
def check_front(O, ids, parts, shards, answer, mask=None, group=1, limit=None):
    """The invariants of one front-end answer for its own input; returns the number of rows.
    Hash mode (limit None): every position finds its effective id, the rows are the distinct
    ids, their number lies inside the model's bounds.  Dense mode: exact below the limit - one
    row per distinct id; the ids at or above it ("no such node") share one row."""
    off, sid, pos = answer
    n = len(ids)
    eff = IC.effective_ids(ids, mask, group)
    sid_n, pos_n = u64_of(sid), t2n(pos)
    off = np.asarray(off, np.int64)
    assert len(off) == shards + 1 and off[0] == 0 and (np.diff(off) >= 0).all()
    assert off[-1] == len(sid_n) <= n and len(pos_n) == n
    if n:
        assert pos_n.min() >= 0 and pos_n.max() < len(sid_n)
    got = sid_n[pos_n]
    if limit is None:
        assert np.array_equal(got, eff)
        assert np.array_equal(np.unique(sid_n), np.unique(eff))
        lo, hi = IC.dedup_row_bounds(eff, IC.front_cap(n))
        assert lo <= len(sid_n) <= hi, (lo, len(sid_n), hi)
    else:
        known = eff < limit
        assert np.array_equal(got[known], eff[known]) and (got[~known] >= limit).all()
        assert np.array_equal(np.sort(sid_n[sid_n < limit]), np.unique(eff[known]))
        beyond = sid_n[sid_n >= limit]
        assert len(beyond) == (1 if (~known).any() else 0) and np.isin(beyond, eff).all()
    own = O.shard_of(sid_n, parts, shards)
    assert np.array_equal(own, np.repeat(np.arange(shards, dtype=np.int32), np.diff(off)))
    return len(sid_n)


def run_front(EA, O, torch, ids, parts, shards, mask=None, group=1, table=None):
    answer = EA.ops.dedup_split(dev(torch, ids), parts, shards,
                                None if mask is None else dev(torch, mask), group, dense_table=table)
    return check_front(O, ids, parts, shards, answer, mask, group,
                       None if table is None else table.numel() - 1)


@pytest.mark.parametrize("n", IC.FRONT_SIZES)
def test_front_chunk_boundaries(EA, O, torch_cuda, n):
    for parts, shards in ((8, 8), (5, 1)):
        run_front(EA, O, torch_cuda, IC.pool_ids(n, 50, 51), parts, shards)
        # one position per id: the model's bounds meet at n, checked by run_front
        assert run_front(EA, O, torch_cuda, IC.distinct_ids(n, 53), parts, shards) == n


def test_front_one_id(EA, O, torch_cuda):
    assert run_front(EA, O, torch_cuda, np.full(2049, 77, np.uint64), 8, 8) == 1


def test_front_shard_shapes(EA, O, torch_cuda):
    """kMaxShards buckets; one bucket; one bucket taking every representative of a full chunk"""
    ids = np.random.default_rng(3).permutation(np.arange(4096, dtype=np.uint64))
    assert run_front(EA, O, torch_cuda, ids, 64, 64) == 4096
    assert run_front(EA, O, torch_cuda, ids, 5, 1) == 4096
    run_front(EA, O, torch_cuda, IC.u64(ids, ids[:100]), 3, 64)          # shards > partitions: empty buckets
    one = np.unique(IC.one_owner_ids(2049, 8, 8))
    assert len(one) == 2049 and run_front(EA, O, torch_cuda, one, 8, 8) == 2049


def test_front_second_round_merges(EA, O, torch_cuda):
    """six ids in one first-round slot: round 1 merges one of them, round 2 must merge the
    other five (201 rows without it)"""
    assert run_front(EA, O, torch_cuda, IC.round2_case(), 8, 8) == 6


def test_front_double_collision(EA, O, torch_cuda):
    """b and c share both slots: 3 rows when one of them wins round 1, else the loser of their
    round-2 slot keeps a row per position"""
    rows = run_front(EA, O, torch_cuda, IC.double_collision_case(), 8, 8)
    assert rows in (3, 2 + IC.ROUND2_COPIES)


def test_front_dirty_scratch(EA, O, torch_cuda):
    """calls of different sizes on one stream: what an earlier call left in the tables (the
    second one is never cleared) changes no answer"""
    torch = torch_cuda
    assert run_front(EA, O, torch, IC.pool_ids(5000, 50, 81), 8, 8) >= 50
    assert run_front(EA, O, torch, IC.round2_case(), 8, 8) == 6
    assert run_front(EA, O, torch, IC.distinct_ids(300, 83), 8, 8) == 300
    assert run_front(EA, O, torch, IC.round2_case(seed=85), 8, 8) == 6


@pytest.mark.parametrize("name", sorted(MASKS))
def test_front_root_masks(EA, O, torch_cuda, name):
    torch = torch_cuda
    ids, mask, group = MASKS[name]
    rows = run_front(EA, O, torch, ids, 8, 8, mask, group)
    eff = IC.effective_ids(ids, mask, group)
    assert rows == len(np.unique(eff))             # a few distinct ids in 1024 slots: checked exact by the bounds
    if name == "all_set":
        off, sid, pos = EA.ops.dedup_split(dev(torch, ids), 8, 8, dev(torch, mask), group)
        assert t2n(sid).tolist() == [0] and not t2n(pos).any()
    table = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    run_front(EA, O, torch, ids, 3, 2, mask, group, table=table)


def test_front_root_mask_too_short(EA, torch_cuda):
    """a mask with fewer bytes than groups is refused before anything is launched"""
    torch = torch_cuda
    ids = dev(torch, IC.distinct_ids(25, 31))
    short = torch.zeros(2, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="root_mask"):
        EA.ops.dedup_split(ids, 8, 8, short, 10)
    with pytest.raises(ValueError, match="root_mask"):
        EA.ops.dedup_split(ids, 8, 8, torch.zeros(24, dtype=torch.uint8, device="cuda"), 0)
    h = EA.ops.FrontHandle()
    with pytest.raises(ValueError, match="root_mask"):
        h.begin(ids, 8, 8, short, 10)
    off, sid, pos = h.begin(ids, 8, 8, torch.zeros(3, dtype=torch.uint8, device="cuda"), 10).end()
    assert off[-1] == 25


def test_front_two_handles_in_flight(EA, O, torch_cuda):
    torch = torch_cuda
    ids_a, ids_b = IC.pool_ids(2049, 50, 91), IC.pool_ids(300, 7, 93)
    a, b = EA.ops.FrontHandle(), EA.ops.FrontHandle()
    a.begin(dev(torch, ids_a), 8, 8)
    b.begin(dev(torch, ids_b), 3, 2)
    with pytest.raises(EA._lib.EulerGpuError, match="in flight"):
        a.begin(dev(torch, ids_b), 3, 2)
    check_front(O, ids_b, 3, 2, b.end())
    check_front(O, ids_a, 8, 8, a.end())
    # both handles are free again
    check_front(O, ids_b, 8, 8, a.begin(dev(torch, ids_b), 8, 8).end())


def test_front_grid_stride(EA, O, torch_cuda):
    """more positions than one pass of the mark and place kernels serves, hashed and dense"""
    torch = torch_cuda
    n = IC.BIG_FRONT_N
    assert run_front(EA, O, torch, IC.pool_ids(n, 3000, 71), 8, 8) == 3000
    rng = np.random.default_rng(95)
    small = rng.choice(rng.permutation(4096)[:3000].astype(np.uint64), n)
    table = torch.randint(-2 ** 31, 2 ** 31 - 1, (4097,), dtype=torch.int32, device="cuda")
    assert run_front(EA, O, torch, small, 8, 8, table=table) == len(np.unique(small))


def test_front_refusals(EA, torch_cuda):
    torch = torch_cuda
    ids = dev(torch, IC.distinct_ids(25, 31))
    with pytest.raises(EA._lib.EulerGpuError, match="shards"):
        EA.ops.dedup_split(ids, 8, 65)
    with pytest.raises(EA._lib.EulerGpuError, match="dense_limit"):
        EA.ops.dedup_split(ids, 8, 8, dense_table=torch.zeros(1, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("name", sorted(DENSE))
def test_front_dense_limits(EA, O, torch_cuda, name):
    """ids at limit - 1, limit and limit + 1; the table as a different call left it"""
    torch = torch_cuda
    ids, entries = DENSE[name]
    limit = entries - 1
    table = torch.randint(-2 ** 31, 2 ** 31 - 1, (entries,), dtype=torch.int32, device="cuda")
    want = len(np.unique(ids[ids < limit])) + 1
    for parts, shards in ((8, 8), (3, 64)):
        assert run_front(EA, O, torch, ids, parts, shards, table=table) == want
        other = np.arange(300, dtype=np.uint64)[::-1] % np.uint64(limit + 2)     # leaves every entry dirty
        assert run_front(EA, O, torch, other, parts, shards, table=table) == limit + 1
        assert run_front(EA, O, torch, ids, parts, shards, table=table) == want
    assert run_front(EA, O, torch, IC.u64(), 8, 8, table=table) == 0


# ---- E. pack_rows / expand_packed / expand_rows ------------------------------------------------
def packed_model(ids, w, t, mask, count, single_type):
    """the wire row: ids (2 words each) | weights | [types] | mask | zeros up to packed_words"""
    m = len(mask)
    cols = [ids.view(np.int32).reshape(m, 2 * count), w.view(np.int32)]
    if single_type is None:
        cols.append(t)
    cols.append(mask.astype(np.int32).reshape(m, 1))
    row = np.concatenate(cols, 1)
    words = ((3 if single_type is not None else 4) * count + 3) & ~1
    return np.concatenate([row, np.zeros((m, words - row.shape[1]), np.int32)], 1)


@pytest.mark.parametrize("single_type", [None, 3], ids=["typed", "single_type"])
@pytest.mark.parametrize("count", [1, 2, 3])
def test_pack_expand_round_trip(EA, torch_cuda, count, single_type):
    torch = torch_cuda
    ops = EA.ops
    for m, n in ((7, 20), (7, 0), (1, 5), (1, 1), (300, 1001)):
        ids, w, t, mask = IC.wire_rows(m, count)
        pos = IC.wire_pos(m, n)
        d = [dev(torch, x) for x in (ids, w, t, mask)]
        packed = ops.pack_rows(*d, count, single_type=single_type)
        assert tuple(packed.shape) == (m, ops.packed_words(count, single_type))
        assert np.array_equal(t2n(packed), packed_model(ids, w, t, mask, count, single_type))
        want_t = t[pos] if single_type is None else \
            np.where(mask[pos][:, None] != 0, -1, single_type).astype(np.int32) * np.ones((1, count), np.int32)
        o_id, o_w, o_t, o_m = (t2n(x) for x in ops.expand_packed(dev(torch, pos), packed, count, single_type))
        assert same_bits(o_id, ids[pos]) and same_bits(o_w, w[pos])
        assert same_bits(o_t, want_t.reshape(n, count)) and same_bits(o_m, mask[pos])
        if single_type is None:
            # the unpacked path answers the same, bit for bit
            e = [t2n(x) for x in ops.expand_rows(dev(torch, pos), *d, count)]
            assert same_bits(e[0], o_id) and same_bits(e[1], o_w)
            assert same_bits(e[2], o_t) and same_bits(e[3], o_m)
