"""CPU-only proof, from the oracle alone, that the cases of neighbor_list_cases.py reach what
test_neighbor_lists_gpu.py needs them to reach: the row totals per type list, every top-k
branch with every weight family, the post-process batch classes, the super-window threshold
of the balanced fill - and that the oracle itself is right where it can be checked here
(against oracle/_ref where that is built; uint64 key order)."""
import numpy as np
import pytest

import neighbor_list_cases as NC


@pytest.fixture(scope="module")
def case(O):
    c = NC.CaseGraph()
    return c, O.OracleGraph(c.csr(O))


@pytest.fixture(scope="module")
def super_case(O):
    b = NC.SuperGraph()
    q = b.queries()
    return b, q, O.OracleGraph(b.csr(O)).get_full_neighbor(q, [0, 1])


def _lens(idx):
    return (idx[:, 1] - idx[:, 0]).astype(np.int64)


def test_case_graph_shape(case):
    c, _ = case
    assert 150 <= len(c.ids) <= 260 and int((c.ids >= 2 ** 63).sum()) >= 8
    # neighbour ids: at and above 2^63, ids without a row, a duplicate key in every row of two or more
    assert int((c.nbr >= 2 ** 63).sum()) > 1000 and np.isin(c.no_row, c.nbr).all()
    assert not np.isin(c.no_row, c.ids).any() and not np.isin(c.unknown, c.ids).any()
    for r in range(len(c.ids)):
        row = c.nbr[c.seg[2 * r]:c.seg[2 * r + 2]]
        assert len(row) < 2 or len(np.unique(row)) < len(row)
    assert c.w.min() == 0.0, "negative weights are outside the contract"
    q = c.queries()
    assert np.isin(c.ids, q).all() and 0 in q and np.isin(c.unknown, q).all()
    assert len(np.unique(q)) < len(q)
    # some row at or above 2^63 is longer than a wave ranks, some is not
    big = c.deg[c.ids >= 2 ** 63].sum(1)
    assert (big > 64).any() and ((big > 0) & (big <= 64)).any()


@pytest.mark.parametrize("et", NC.TYPE_LISTS, ids=str)
def test_row_totals_per_type_list(case, et):
    """Every boundary total is met by some queried row under every type list, as the oracle
    counts it; the query list starts and ends with a row that lists nothing."""
    c, OG = case
    q = c.queries()
    idx, ids, w, t = OG.get_full_neighbor(q, et)
    lens = _lens(idx)
    have = set(lens.tolist())
    want = set(NC.TOTALS) if et != [1, 1] else {e for s in NC.TOTALS for e in NC.doubled_totals(s)}
    assert want <= have, sorted(want - have)
    assert lens[0] == 0 and lens[-1] == 0 and q[0] != 0 and q[-1] != 0
    assert idx[-1, 1] == len(ids) == lens.sum()
    # the oracle's count == the degree table's
    known = {int(i): int(v) for i, v in zip(c.ids, c.totals(et))}
    assert [known.get(int(x), 0) for x in q] == lens.tolist()
    # a total below, equal to and above every k, and a total of 0
    for k in NC.TOP_KS:
        assert (k in have or (et == [1, 1] and k % 2 == 1)) and (lens < k).any() and (lens > k).any(), k
    assert 0 in have


def test_weights_are_the_raw_weights_and_families_hold(case):
    """The weight an entry reports is a difference of float32 running sums: on this graph it
    is the raw weight, bit for bit, and each family is what its name says in storage order."""
    c, OG = case
    idx, ids, w, t = OG.get_full_neighbor(c.ids, [0, 1])
    assert np.array_equal(w.view(np.uint32), c.w.view(np.uint32))
    assert np.array_equal(ids, c.nbr)
    seen = set()
    for r, fam in enumerate(c.family):
        x, tt = w[idx[r, 0]:idx[r, 1]], t[idx[r, 0]:idx[r, 1]]
        if len(x) < 2:
            continue
        seen.add(fam)
        d = np.diff(x)
        if fam == "asc":
            assert (d > 0).all()
        elif fam == "desc":
            assert (d < 0).all()
        elif fam == "equal":
            assert (d == 0).all()
        elif fam == "five":
            assert len(np.unique(x)) <= 5 and (len(x) < 10 or len(np.unique(x)) == 5)
        elif fam == "zeros":
            assert (x[::2] == 0).all() and (x[1::2] > 0).all()
        elif fam == "tail9":
            if len(x) > 9:
                assert x[-9:].min() > x[:-9].max()
        elif fam == "shared":
            a, b = x[tt == 0], x[tt == 1]
            m = min(len(a), len(b))
            assert np.array_equal(a[:m], b[:m])
    assert seen == set(NC.FAMILIES)


@pytest.mark.parametrize("et", NC.TYPE_LISTS, ids=str)
def test_top_k_branches_meet_every_family(case, et):
    """TopKNeighborKernel has three branches: a total of at most 64, a total over 64 with
    k <= 8 and a total over 64 with k > 8.  Under every type list some queried row of every
    weight family lands in each (both k ranges are in TOP_KS, so the last two share rows)."""
    c, OG = case
    q = c.queries()
    lens = _lens(OG.get_full_neighbor(q, et)[0])
    fam_of = {int(i): f for i, f in zip(c.ids, c.family)}
    assert min(NC.TOP_KS) <= 8 and 8 in NC.TOP_KS and max(NC.TOP_KS) > 8
    for fam in NC.FAMILIES:
        mine = np.array([fam_of.get(int(x)) == fam for x in q])
        assert ((lens > 1) & (lens <= 64) & mine).any(), (fam, "<= 64")
        assert ((lens > 64) & (lens <= 256) & mine).any(), (fam, "65..256")
        assert ((lens > 256) & mine).any(), (fam, "> 256")


def test_shared_rows_decide_ties_by_listed_order(O, case):
    """On a `shared` row the same weights stand in both segments: the heaviest k under [1, 0]
    start with type 1's entry, under [0, 1] with type 0's, and the two answers differ - a
    kernel that broke ties by physical position would give the same answer for both."""
    c, OG = case
    r = [i for i in c.rows_with(100, 100) if c.family[i] == "shared"][0]
    q = c.ids[r:r + 1]
    top = {}
    for et in ([0, 1], [1, 0]):
        full = OG.get_full_neighbor(q, et)
        top[tuple(et)] = O.neighbor_to_dense(*O.neighbor_post_process(*full, order_by="weight", desc=True,
                                                                      limit=8), 8, -1)
    assert top[(0, 1)][2][0, 0] == 0 and top[(1, 0)][2][0, 0] == 1
    assert not np.array_equal(top[(0, 1)][2], top[(1, 0)][2])
    assert np.array_equal(top[(0, 1)][1], top[(1, 0)][1])


@pytest.mark.parametrize("et", ([0, 1], [1, 0]), ids=str)
def test_post_process_batch_classes(case, et):
    c, OG = case
    b = c.batches(et)
    short, long_, mixed = (_lens(OG.get_full_neighbor(b[k], et)[0]) for k in ("short", "long", "mixed"))
    assert short.max() == 64 and (short == 0).any() and 63 in short
    assert long_.min() == 65 and long_.max() == 2049 and len(long_) > 20
    assert (mixed <= 64).any() and (mixed > 64).any()
    assert 5000 > mixed.max() and max(l for l in NC.LIMITS if l is not None) == 5000


def test_oracle_orders_ids_as_uint64(O):
    """order_by id compares keys as the reference does (uint64_t): ids at and above 2^63
    sort after every smaller id, not before as int64 would put them."""
    ids = np.array([2 ** 63 + 1, 5, 2 ** 64 - 1, 2 ** 63, 7, 2 ** 63 + 1, 0], np.uint64)
    idx = np.array([[0, 7]], np.int32)
    w = np.arange(7, dtype=np.float32)
    t = np.arange(7, dtype=np.int32)
    for desc in (False, True):
        _, gi, gw, gt = O.neighbor_post_process(idx, ids, w, t, order_by="id", desc=desc)
        order = np.argsort(ids, kind="stable") if not desc else \
            np.argsort(np.uint64(2 ** 64 - 1) - ids, kind="stable")
        assert np.array_equal(gi, ids[order]) and np.array_equal(gt, t[order])


def test_oracle_equals_ref_on_case_graph(O, case):
    """Where oracle/_ref is built: the oracle's get_full_neighbor == the reference's own on
    the case graph, for every type list (the [] and unknown-type lists included)."""
    if not O.have_ref():
        return
    c, OG = case
    R = O.RefGraph.build_raw(c.ids, c.seg, c.nbr, c.w, 2)
    q = c.queries()
    for et in list(NC.TYPE_LISTS) + [[], [9]]:
        for a, b in zip(OG.get_full_neighbor(q, et), R.get_full_neighbor(q, et)):
            if a.dtype == np.float32:
                a, b = a.view(np.uint32), b.view(np.uint32)
            assert a.shape == b.shape and np.array_equal(a, b), et


def test_super_window_query_reaches_the_threshold(super_case):
    """The query of the super-window test, as the oracle counts it: over the balanced fill's
    threshold (a later change of `32 << 20` in the kernel fails here instead of leaving the
    path silently unrun), not a multiple of the window, and with every shape of super window
    the kernel tells apart."""
    b, q, (idx, ids, w, t) = super_case
    total = int(idx[-1, 1])
    assert 1_500_000 <= b.n_edges <= 2_500_000
    assert total >= NC.SUPER_THRESHOLD, total
    assert total < 36 << 20 and total % NC.WINDOW != 0 and total % NC.SUPER != 0
    lens = _lens(idx)
    assert lens[0] == 0 and lens[-1] == 0 and not np.isin(q[[1, -1]], b.ids).any()
    R0, R1 = NC.window_rows(idx, NC.SUPER)
    r0, r1 = NC.window_rows(idx, NC.WINDOW)
    inside = R0 == R1
    assert inside.sum() > 1000, "whole super windows inside one row"
    # ... also of a hub whose neighbours in the query are empty rows / unknown ids
    h0 = np.flatnonzero(q == b.hub[0])
    assert np.diff(h0).min() == 1 and lens[h0[0] - 1] == 0 and lens[h0[-1] + 1] == 0
    assert (R1 - R0).max() > 300, "a super window over many rows"
    # rows that list nothing inside such a window (the walk to the next row skips them)
    many = int(np.argmax(R1 - R0))
    assert (lens[R0[many]:R1[many] + 1] == 0).sum() > 20
    # a 256-entry window inside one row while its super window spans several
    sup_of = np.arange(len(r0)) // 8
    assert ((r0 == r1) & ~inside[sup_of]).sum() > 1000
    # and windows over two or more rows
    assert ((r1 - r0) >= 2).sum() > 40
    assert (ids >= 2 ** 63).any() and (w == 0).any() and set(np.unique(t).tolist()) == {0, 1}


def test_overflow_queries_wrap_int32(super_case):
    """The totals test_neighbor_lists_gpu.py expects to be refused: 2049 times the hub wraps
    int32 negative, 4097 times wraps to a small positive number."""
    b, q, _ = super_case
    assert int(b.deg[0, 0]) == NC.HUB_ENTRIES == 2 ** 20 + 3
    for reps, sign in ((2049, -1), (4097, 1)):
        total = reps * NC.HUB_ENTRIES
        wrapped = int(np.int64(total).astype(np.int32))
        assert total >= 2 ** 31 and np.sign(wrapped) == sign
        if sign > 0:
            assert wrapped < 2 ** 21
    assert 2048 * (2 ** 20 - 1) + 2047 == 2 ** 31 - 1
