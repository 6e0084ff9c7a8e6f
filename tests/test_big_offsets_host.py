"""tests/big_offsets.py on the CPU: the conditions under which a narrowed offset in a kernel is
visible to tests/test_big_offsets_gpu.py.

The GPU tests write non-zero values into the probe rows of an otherwise zero table and compare an
op's result with its reference on the small table of those rows.  A read through a wrapped offset
is visible when it returns anything but the row's own values; a write through one is visible when
it lands in a row that is compared (a probe row) or counted (every other row: the chunked
count_nonzero over the buffer).  The second holds for every row.  The first is checked here.

It cannot be had in the stronger form "no alias of a probe row is another probe row": rows 0 and 1
are probe rows, and the rows just past 2^32 wrap to the offsets just past 0 (d = 136: row
31580642 begins at element 2^32 + 16, which wraps to element 16 of row 0); likewise the rows at
2^32 taken modulo 2^31 land in the probe rows at 2^31.  Such a read returns another probe row's
values, shifted by some columns, which differ from the row's own:
test_a_wrapped_read_is_never_the_rows_own_values asserts exactly that, on the values the GPU tests write.

The table search scans every row instead of reading named ones: its queries are the probe rows
themselves, and a query equal to a row scores l2 = 0 and the largest ip against that row alone
(test_another_row_scores_differently), so a scan that reads another row shows in the lists."""
import numpy as np
import pytest

import big_offsets as bo
import embed_store_ref as store_ref

# every (n_elems, d, dtype) test_big_offsets_gpu.py builds a table over
CASES = ([(bo.BIG, d, dt) for d in bo.DIMS for dt in store_ref.DTYPES]
         + [(bo.HALF, d, dt) for d in bo.DIMS for dt in store_ref.DTYPES]
         + [(bo.EDGE_ROWS * bo.EDGE_DIM, bo.EDGE_DIM, dt) for dt in store_ref.DTYPES])


def test_the_sizes_are_past_the_boundaries():
    assert bo.BIG > 1 << 32 and bo.HALF > 1 << 31 and bo.EDGE_ROWS * bo.EDGE_DIM >= 1 << 32
    assert bo.EDGE_ROWS < 1 << 31 and bo.BIG <= bo.BUF >= bo.EDGE_ROWS * bo.EDGE_DIM
    for d in bo.DIMS + (bo.EDGE_DIM,):
        assert d & (d - 1) and bo.BIG // d < 1 << 31
    assert [d % 8 == 0 for d in bo.DIMS] == [True, False, False]
    assert [d % 4 == 0 for d in bo.DIMS] == [True, True, False]


@pytest.mark.parametrize("n_elems,d,dt", CASES)
def test_probe_rows_hold_the_edges_and_a_row_across_each_boundary(n_elems, d, dt):
    eb = bo.ELEM_BYTES[dt]
    rows = n_elems // d
    probe = bo.probe_rows(n_elems, d, eb)
    assert np.all(np.diff(probe) > 0) and probe[0] == 0 and probe[-1] == rows - 1
    assert {0, 1, rows - 2, rows - 1} <= set(probe.tolist()) and len(probe) <= 4 + 3 * 3
    seen = 0
    for b in bo.boundaries(eb):
        if b >= rows * d:
            continue
        r = bo.straddling_row(b, d)
        assert r == b // d and r * d < b < (r + 1) * d                # it holds element b - 1 and element b
        assert {r - 1, r, r + 1} <= set(probe.tolist())
        # in bytes: the row holds the byte before and the byte at b * eb
        assert r * d * eb < b * eb < (r + 1) * d * eb
        seen += 1
    assert seen == (len(bo.boundaries(eb)) if n_elems > 1 << 32 else len(bo.boundaries(eb)) - 1)


@pytest.mark.parametrize("n_elems,d,dt", CASES)
def test_alias_rows(n_elems, d, dt):
    """a row below every modulus aliases only itself; a row at or past one aliases some other row,
    below the modulus; every alias is a row of the table"""
    eb = bo.ELEM_BYTES[dt]
    probe = bo.probe_rows(n_elems, d, eb)
    alias = bo.alias_rows(probe, d, eb)
    lowest = min(1 << 31, (1 << 32) // eb)
    assert sorted(alias) == probe.tolist()
    for r, hits in alias.items():
        assert all(0 <= a <= r for a in hits) and (r in hits) == (r * d < 1 << 32)
        if r * d + d - 1 < lowest:
            assert hits == [r]
        else:
            assert any(a != r for a in hits)
    # by hand, d = 136 in 16 bits: the row past 2^32 lands in row 0, the row past 2^31 too
    if (n_elems, d, eb) == (bo.BIG, 136, 2):
        assert (1 << 32) // 136 == 31580641 and 31580642 * 136 - (1 << 32) == 16
        assert 0 in alias[31580642] and 0 in alias[(1 << 31) // 136 + 1]
        assert (1 << 31) // 136 in alias[31580641]                     # 2^32 modulo 2^31


@pytest.mark.parametrize("n_elems,d,dt", CASES)
def test_a_wrapped_read_is_never_the_rows_own_values(n_elems, d, dt):
    """with the values the GPU tests write: reading a probe row through its offset modulo 2^31
    elements, 2^32 elements or 2^32 bytes returns the row itself when nothing wrapped and otherwise
    something that differs from it - zeros from a row that is no probe row, or the shifted values of
    another probe row"""
    eb = bo.ELEM_BYTES[dt]
    probe = bo.probe_rows(n_elems, d, eb)
    values = bo.probe_values(np.random.default_rng(d), len(probe), d)
    wrapped = 0
    for n, r in enumerate(probe.tolist()):
        for w, got in zip(bo.wrapped_offsets(r * d, eb), bo.wrapped_read(values, probe, d, r, eb)):
            if w == r * d:
                assert np.array_equal(got, values[n])
            else:
                wrapped += 1
                assert np.count_nonzero(got != values[n]) > d // 2, (r, w)
    assert wrapped >= 3


def test_probe_values_are_exact_in_every_dtype_and_distinct():
    v = bo.probe_values(np.random.default_rng(1), 13, 136)
    assert v.dtype == np.float32 and np.all(v != 0) and np.abs(v).max() <= 4 and np.abs(v).min() >= 2.0 ** -5
    for dt in store_ref.DTYPES:
        assert np.array_equal(store_ref.widen(store_ref.narrow(v, dt), dt), v)
    assert len({row.tobytes() for row in v}) == 13


def test_compact_round_trips():
    rng = np.random.default_rng(2)
    for n_elems, d, dt in CASES:
        rows = n_elems // d
        probe = bo.probe_rows(n_elems, d, bo.ELEM_BYTES[dt])
        ids = bo.named_twice(rng, probe, extra=bo.no_row_ids(rows), total=64)
        assert len(ids) == 64 and all(np.count_nonzero(ids == p) >= 2 for p in probe)
        small = bo.compact(ids, probe, rows)
        named = (ids >= 0) & (ids < rows)
        assert np.array_equal(probe[small[named]], ids[named])
        # an id that names no row of the table names none of the small one, and keeps its kind
        assert np.all((small[~named] < 0) | (small[~named] >= len(probe)))
        assert np.array_equal(small[ids < 0], ids[ids < 0])
        assert np.array_equal(small[ids >= rows] - len(probe), ids[ids >= rows] - rows)
        assert np.array_equal(bo.expand(small, probe, rows), ids)
        # the order of the occurrences is kept: equal ids stay equal, distinct stay distinct
        assert np.array_equal(ids[:, None] == ids[None, :], small[:, None] == small[None, :])
    with pytest.raises(ValueError):
        bo.compact(np.array([2]), probe, rows)


# ---- the table search over the big table ------------------------------------------------------------
import table_search_ref as SR                                             # noqa: E402

SEARCH_CASES = [(d, dt) for d in bo.DIMS for dt in store_ref.DTYPES]


@pytest.mark.parametrize("d,dt", SEARCH_CASES)
def test_search_case_names_the_boundary_rows_and_runs_512_slabs(d, dt):
    """what test_big_offsets_gpu.py::test_table_search asks: at most 33 queries (two tiles), every
    probe row among them; exclude and target name boundary rows, zero rows and no row; the launch
    shape is 2 tiles x 512 slabs, each item a block of its own, every slab non-empty"""
    eb = bo.ELEM_BYTES[dt]
    rows = bo.BIG // d
    probe = bo.probe_rows(bo.BIG, d, eb)
    values = bo.probe_values(np.random.default_rng(d), len(probe), d)
    queries, exclude, target = bo.search_case(np.random.default_rng(9500 + d), probe, values, bo.BIG, d, eb)
    assert queries.shape == (bo.SEARCH_Q, d) and bo.SEARCH_Q <= 33 and len(probe) < bo.SEARCH_K <= SR.MAX_K
    edge, zero = bo.boundary_rows(bo.BIG, d, eb), bo.zero_rows(probe, rows)
    assert len(edge) == len(bo.boundaries(eb)) + 1 and edge[-1] == rows - 1 and zero[0] == 2
    for b, r in zip(bo.boundaries(eb), edge):
        assert r * d < b < (r + 1) * d
    assert np.array_equal(queries[:len(probe)], values) and not queries[len(probe)].any()
    for ids, none in ((exclude, rows + 5), (target, rows)):
        assert set(edge.tolist()) <= set(ids.tolist()) and zero[0] in ids and zero[1] in ids and -1 in ids and none in ids
    own = exclude[:len(probe)] == probe
    assert own[::2].all() and not own[1::2].any()
    tiles = SR.tiles_of(bo.SEARCH_Q, d)
    slabs = SR.slabs_of(rows, tiles)
    slab_rows = -(-rows // slabs)
    assert (tiles, slabs) == (2, 512) and tiles * slabs <= SR.BLOCK_CAP and (slabs - 1) * slab_rows < rows < 1 << 31
    assert slabs * bo.SEARCH_Q * bo.SEARCH_K * 8 < 10 << 20                # the scratch the cases add


@pytest.mark.parametrize("d,dt", SEARCH_CASES)
def test_another_row_scores_differently(d, dt):
    """why a scan that reads a wrong row shows: a query equal to a probe row scores l2 = 0 and the
    largest ip against that row alone - no other probe row, no zero row, and nothing a narrowed offset
    of the row returns gives either; so a wrong read moves the row in the list or changes its score"""
    eb = bo.ELEM_BYTES[dt]
    probe = bo.probe_rows(bo.BIG, d, eb)
    values = bo.probe_values(np.random.default_rng(d), len(probe), d)
    v = SR.chunk_width(d, 0, eb, 0, 4)
    table = np.concatenate([values, np.zeros((1, d), np.float32)])         # the probe rows and a zero row
    l2, ip = SR.scores(table, values, "l2", v), SR.scores(table, values, "ip", v)
    here = np.arange(len(probe))
    assert np.all(l2[here, here] == 0) and np.count_nonzero(l2 == 0) == len(probe)
    assert np.array_equal(np.argmax(ip, 1), here) and np.all(np.sort(ip, 1)[:, -1] > np.sort(ip, 1)[:, -2])
    wrapped = 0
    for n, r in enumerate(probe.tolist()):
        for w, got in zip(bo.wrapped_offsets(r * d, eb), bo.wrapped_read(values, probe, d, r, eb)):
            if w != r * d:
                wrapped += 1
                assert SR.scores(got[None, :], values[n:n + 1], "l2", v)[0, 0] > 0
                assert SR.scores(got[None, :], values[n:n + 1], "ip", v)[0, 0] < ip[n, n]
    assert wrapped >= 3


def test_sparse_expectations_at_the_big_shape():
    """sparse_topk / sparse_rank at n = 31.6 M rows, without a table: the zero rows that fill the
    tail are the lowest rows that are no probe row, in row order, and a zero-row target ranks behind
    every other zero row"""
    d, dt = 136, "bf16"
    rows = bo.BIG // d
    probe = bo.probe_rows(bo.BIG, d, 2)
    values = bo.probe_values(np.random.default_rng(d), len(probe), d)
    queries, exclude, target = bo.search_case(np.random.default_rng(9500 + d), probe, values, bo.BIG, d, 2)
    for metric in SR.METRICS:
        sc, got = SR.sparse_topk(probe, values, rows, queries, bo.SEARCH_K, metric, 8, exclude)
        z = SR.scores(np.zeros((1, d), np.float32), queries, metric, 8)[:, 0]
        for i in range(len(queries)):
            zero = got[i][~np.isin(got[i], probe)]
            want = [r for r in range(2, 2 + bo.SEARCH_K + 1) if r != exclude[i]][:len(zero)]
            assert zero.tolist() == want and len(zero) >= bo.SEARCH_K - len(probe)
            assert np.all(sc[i][~np.isin(got[i], probe)] == z[i]) and exclude[i] not in got[i]
        rank = SR.sparse_rank(probe, values, rows, queries, target, metric, 8, exclude)
        at_zero = np.isin(target, bo.zero_rows(probe, rows))
        assert np.all(rank[at_zero] >= rows - len(probe) - 2) and np.all(rank[(target < 0) | (target >= rows)] == -1)
