"""ops.table_topk / ops.table_rank on the GPU against the numpy restatement
(tests/table_search_ref.py), bit for bit: the case table of test_table_search_host.py, then the
smallest shapes that reach each path of the kernels.

The launch shape, read off LaunchSearch (table_search_kernels.hip) and restated in
table_search_ref: a block takes one (query tile, slab) item a trip; a tile is 4 waves x 8 queries
= 32 queries while d <= 384 (fewer a wave above, queries read from memory past d = 3072); a table
of up to 1024 rows is one slab, slabs = min(ceil(2048 / tiles), ceil(N / 1024), 512); the grid is
capped at 8192 blocks; the merge runs a wave per query, four a block, under the same cap.

After the feature's own cases: each term of the slab rule (the clamp by the tiles, the shortest last
slab, the cap of 512), every branch of the chunk-width rule on views off a 16-byte boundary, the
wave list under chosen arrival orders, all-NaN queries, rows that score the fill value, and
table_rank against the float64 count.  What can be evaluated without a GPU - V per case, slab
counts, the separation of the float64 scores, the helpers for many queries - is asserted in
test_table_search_host.py as well.  (Offsets past 2^31: test_big_offsets_gpu.py.)

A NaN score is compared as "NaN on both sides"."""
import ctypes as C

import numpy as np
import pytest

import table_search_ref as ref
from table_search_ref import DIMS, DTYPES, ITEM, KS, METRICS, queries_for, same_scores, tie_table

pytestmark = pytest.mark.gpu
F = np.float32


def _torch_dt(torch, dt):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dt]


def dev(torch, x, dt="f32"):
    """a widened fp32 array whose values the type holds exactly -> a device tensor of that type"""
    return torch.from_numpy(np.ascontiguousarray(x, F)).to("cuda").to(_torch_dt(torch, dt))


def ids_dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int64)).to("cuda")


def width(table, queries):
    d = table.shape[1]
    return ref.chunk_width(d, table.data_ptr(), table.element_size(), queries.data_ptr(), queries.element_size())


def check(torch, ops, table, queries, t_np, q_np, metric, k, exclude=None, target=None, s=None, tag=()):
    """one top-k call (and one rank call with `target`) == the restatement -> the scores used"""
    v = width(table, queries)
    s = ref.scores(t_np, q_np, metric, v) if s is None else s
    got_s, got_r = ops.table_topk(table, queries, k, metric=metric, exclude=ids_dev(torch, exclude))
    assert got_s.dtype == torch.float32 and got_r.dtype == torch.int64 and not got_s.requires_grad
    want = ref.topk(t_np, q_np, k, metric, v, exclude, s=s)
    assert same_scores(got_s.cpu().numpy(), want[0]), tag + ("scores",)
    assert np.array_equal(got_r.cpu().numpy(), want[1]), tag + ("rows",)
    if target is not None:
        got = ops.table_rank(table, queries, ids_dev(torch, target), metric=metric, exclude=ids_dev(torch, exclude))
        assert got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), ref.rank(t_np, q_np, target, metric, v, exclude, s=s)), tag + ("rank",)
    return s


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_case_table(torch_cuda, EA, d, metric):
    """the host test's case table through the ops: nine dtype pairs, k in KS x N in
    {1, k - 1, k, k + 1, 300}, tie-heavy tables with NaN and inf rows, exclude absent / in range /
    out of range, targets in and out of range"""
    torch, ops = torch_cuda, EA.ops
    for it, dtt in enumerate(DTYPES):
        for iq, dq in enumerate(DTYPES):
            rng = np.random.default_rng(1000 * d + 10 * it + iq)
            t_np = tie_table(rng, 300, d, dtt)
            q_np, own = queries_for(rng, t_np, dq)
            q = len(q_np)
            table, queries = dev(torch, t_np, dtt), dev(torch, q_np, dq)
            assert width(table, queries) == ref.chunk_width(d, 0, ITEM[dtt], 0, ITEM[dq])
            s_all = ref.scores(t_np, q_np, metric, width(table, queries))
            ks = KS if dtt == dq else (10,)
            for n in sorted({1, 300} | {n for k in ks for n in (k - 1, k, k + 1) if n >= 1}):
                excludes = [None, np.concatenate([own, np.full(q - len(own), -1)]) % n,
                            np.array([-1, n, n + 5, 1 << 33, -(1 << 40), n], np.int64)]
                target = np.random.default_rng(n).integers(0, n, q)
                target[-1], target[-2] = n + 2, -1
                for k in ks:
                    for ei, exc in enumerate(excludes if (k in (3, 10) or n <= 3) else excludes[:1]):
                        check(torch, ops, table[:n], queries, t_np[:n], q_np, metric, k, exc,
                              target if k == ks[0] or ei else None, s=s_all[:, :n], tag=(d, metric, dtt, dq, n, k, ei))


@pytest.mark.parametrize("metric,dtt,dq,d", [("ip", "bf16", "f32", 8), ("l1", "f32", "f32", 12), ("cos", "f16", "bf16", 64),
                                              ("l2", "bf16", "bf16", 130)])
def test_slab_and_tile_edges(torch_cuda, EA, metric, dtt, dq, d):
    """N = one slab - 1, one slab, one slab + 1 and three slabs + 1 (1, 1, 2 and 4 slabs: the merge
    runs) x Q = 1, one tile - 1, one tile, one tile + 1 and two tiles + 1"""
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(77 + d)
    n_max, q_max = 3 * ref.MIN_SLAB_ROWS + 1, 65
    t_np = tie_table(rng, n_max, d, dtt)
    q_np = ref.to_dtype(np.concatenate([t_np[rng.integers(0, n_max, 40)], rng.standard_normal((q_max - 40, d))]), dq)
    table, queries = dev(torch, t_np, dtt), dev(torch, q_np, dq)
    s_all = ref.scores(t_np, q_np, metric, width(table, queries))
    assert ref.wave_queries(d) == (8, True)
    for n, slabs in ((1023, 1), (1024, 1), (1025, 2), (3073, 4)):
        for q in (1, 31, 32, 33, 65):
            assert ref.slabs_of(n, ref.tiles_of(q, d)) == slabs
            exc = rng.integers(-2, n + 2, q)
            target = rng.integers(-1, n + 1, q)
            check(torch, ops, table[:n], queries[:q], t_np[:n], q_np[:q], metric, 10, exc, target, s=s_all[:q, :n],
                  tag=(metric, n, q))
    check(torch, ops, table, queries, t_np, q_np, metric, 64, None, None, s=s_all, tag=(metric, "k64"))


@pytest.mark.parametrize("d,qw,staged", [(768, 4, True), (3072, 1, True), (3080, 8, False)])
def test_wide_rows_take_fewer_queries_a_wave(torch_cuda, EA, d, qw, staged):
    """d past 384: fewer queries a wave so that the tile fits LDS; past 3072 the queries are read
    from memory.  Q = one tile + 1 of that shape, two slabs."""
    torch, ops = torch_cuda, EA.ops
    assert ref.wave_queries(d) == (qw, staged)
    rng = np.random.default_rng(d)
    n, q = ref.MIN_SLAB_ROWS + 1, 4 * qw + 1
    t_np = ref.to_dtype(rng.standard_normal((n, d)), "bf16")
    t_np[5] = t_np[900]
    q_np = ref.to_dtype(np.concatenate([t_np[[5, 1024]], rng.standard_normal((q - 2, d))]), "f16")
    table, queries = dev(torch, t_np, "bf16"), dev(torch, q_np, "f16")
    for metric in ("cos", "l1"):
        check(torch, ops, table, queries, t_np, q_np, metric, 5, None, rng.integers(0, n, q), tag=(d, metric))


def test_more_items_than_the_grid_cap(torch_cuda, EA):
    """Q = 8193 tiles + 1 query over a 40-row table, d = 4: LaunchSearch wants tiles * slabs =
    8194 * 1 items against the cap of 8192 blocks, so blocks 0 and 1 make a second trip (tiles
    8192 and 8193: queries 262144 on); the merge wants ceil(Q / 4) = 65545 blocks against the same
    cap.  Every query's rows, scores and rank are checked."""
    torch, ops = torch_cuda, EA.ops
    d, n, k = 4, 40, 5
    q = ref.BLOCK_CAP * 32 + 33
    tiles = ref.tiles_of(q, d)
    assert tiles * ref.slabs_of(n, tiles) == ref.BLOCK_CAP + 2 and -(-q // 4) > ref.BLOCK_CAP
    rng = np.random.default_rng(12)
    t_np = tie_table(rng, n, d, "f32")
    q_np = np.array([-2, -1, -0.0, 0, 1, 2], F)[rng.integers(0, 6, (q, d))]
    q_np[1::3] = rng.standard_normal((len(q_np[1::3]), d)).astype(F)
    table, queries = dev(torch, t_np), dev(torch, q_np)
    for metric in ("ip", "l2"):
        s = ref.scores(t_np, q_np, metric, width(table, queries))
        got_s, got_r = ops.table_topk(table, queries, k, metric=metric)
        rows = ref.order_all(s, metric)[:, :k]
        assert np.array_equal(rows[-40:], ref.topk(t_np, q_np[-40:], k, metric, 4, s=s[-40:])[1])
        assert np.array_equal(got_r.cpu().numpy(), rows)
        assert same_scores(got_s.cpu().numpy(), np.take_along_axis(s, rows, 1))
        target = rng.integers(0, n, q)
        got = ops.table_rank(table, queries, ids_dev(torch, target), metric=metric).cpu().numpy()
        st = np.take_along_axis(s, target[:, None], 1)
        with np.errstate(invalid="ignore"):
            hit = (s >= st) if ref.larger_is_better(metric) else (s <= st)
        want = hit.sum(1) - np.take_along_axis(hit, target[:, None], 1)[:, 0]
        assert np.array_equal(want[-40:], ref.rank(t_np, q_np[-40:], target[-40:], metric, 4, s=s[-40:]))
        assert np.array_equal(got, want.astype(np.int32))


def test_table_view_off_a_16_byte_boundary(torch_cuda, EA):
    """an fp32 table view 4 bytes past a 16-byte boundary: V = 1 on the device too"""
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(8)
    n, d = 1100, 64
    t_np = tie_table(rng, n, d, "f32")
    q_np, own = queries_for(rng, t_np, "f32")
    base = torch.empty(n * d + 1, device="cuda")
    assert base.data_ptr() % 16 == 0
    table = base[1:].view(n, d)
    table.copy_(torch.from_numpy(t_np))
    queries = dev(torch, q_np)
    assert width(table, queries) == 1 and width(dev(torch, t_np), queries) == 8
    for metric in METRICS:
        check(torch, ops, table, queries, t_np, q_np, metric, 10, None, own.tolist() + [0, 1, 2], tag=(metric,))


def test_same_bits_on_every_run_and_stream(torch_cuda, EA):
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(4)
    t_np = tie_table(rng, 3073, 64, "bf16")
    table = dev(torch, t_np, "bf16")
    queries = dev(torch, ref.to_dtype(rng.standard_normal((65, 64)), "bf16"), "bf16")
    target = ids_dev(torch, rng.integers(0, 3073, 65))
    first = ops.table_topk(table, queries, 17, metric="cos") + (ops.table_rank(table, queries, target, metric="cos"),)
    again = ops.table_topk(table, queries, 17, metric="cos") + (ops.table_rank(table, queries, target, metric="cos"),)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.table_topk(table, queries, 17, metric="cos") + (ops.table_rank(table, queries, target, metric="cos"),)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        a, b, c = (x.cpu().numpy() for x in (a, b, c))
        if a.dtype == np.float32:
            assert same_scores(a, b) and same_scores(a, c)
        else:
            assert np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.parametrize("metric", METRICS)
def test_distinct_rows_equal_topk_of_the_float64_scores(torch_cuda, EA, metric):
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(31)
    t_np, q_np = rng.standard_normal((3073, 64)).astype(F), rng.standard_normal((33, 64)).astype(F)
    exact, bound = ref.scores64(t_np, q_np, metric)
    want = torch.topk(torch.from_numpy(exact), 10, dim=1, largest=ref.larger_is_better(metric))
    best = np.sort(-exact if ref.larger_is_better(metric) else exact, 1)[:, :11]
    assert np.diff(best, axis=1).min() > 2 * bound.max()                 # (no pair among the best the rounding could swap)
    got_s, got_r = ops.table_topk(dev(torch, t_np), dev(torch, q_np), 10, metric=metric)
    assert np.array_equal(got_r.cpu().numpy(), want.indices.numpy())
    assert np.all(np.abs(got_s.cpu().numpy().astype(np.float64) - want.values.numpy()) <= bound.max())


def test_refused_call_leaves_both_outputs_untouched(torch_cuda, EA):
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    table, queries = torch.ones(50, 8, device="cuda"), torch.ones(4, 8, device="cuda")
    scores = torch.full((4, 3), 7.5, device="cuda")
    rows = torch.full((4, 3), -77, dtype=torch.int64, device="cuda")
    rank = torch.full((4,), -77, dtype=torch.int32, device="cuda")
    target = torch.zeros(4, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                               # noqa: E731
    for change in (dict(metric=4), dict(k=65), dict(k=0), dict(qdt=3), dict(queries=None), dict(n=1 << 31)):
        a = dict(dict(metric=0, k=3, qdt=0, queries=p(queries), n=50), **change)
        rc = L.euler_gpu_table_topk(None, a["metric"], p(table), 0, a["n"], 8, a["queries"], a["qdt"], 4, a["k"], None,
                                    p(scores), p(rows))
        assert rc == -1 and L.euler_gpu_last_error().decode().startswith("table_topk: ")
        if "k" not in change:
            rc = L.euler_gpu_table_rank(None, a["metric"], p(table), 0, a["n"], 8, a["queries"], a["qdt"], 4, p(target),
                                        None, p(rank))
            assert rc == -1 and L.euler_gpu_last_error().decode().startswith("table_rank: ")
    torch.cuda.synchronize()
    assert torch.all(scores == 7.5) and torch.all(rows == -77) and torch.all(rank == -77)


def test_ids_map_the_rows_and_keep_minus_one(torch_cuda, EA):
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(2)
    t_np, q_np = rng.standard_normal((5, 8)).astype(F), rng.standard_normal((3, 8)).astype(F)
    table, queries = dev(torch, t_np), dev(torch, q_np)
    ids = torch.arange(5, device="cuda") * 10 + 7
    exc = torch.tensor([0, -1, 4], device="cuda")
    s0, r0 = ops.table_topk(table, queries, 8, metric="l2", exclude=exc)
    s1, r1 = ops.table_topk(table, queries, 8, metric="l2", exclude=exc, ids=ids)
    r0, r1 = r0.cpu().numpy(), r1.cpu().numpy()
    assert np.array_equal(s0.cpu().numpy(), s1.cpu().numpy())
    assert np.array_equal(r1, np.where(r0 >= 0, r0 * 10 + 7, -1))
    assert (r0 >= 0).sum(1).tolist() == [4, 5, 4] and np.all(r1[r0 < 0] == -1) and np.all(np.isinf(s0.cpu().numpy()[r0 < 0]))
    with pytest.raises(ValueError):
        ops.table_topk(table, queries, 8, ids=ids[:4])


@pytest.mark.parametrize("metric", METRICS)
def test_empty_shapes(torch_cuda, EA, metric):
    torch, ops = torch_cuda, EA.ops
    queries = torch.ones(3, 8, device="cuda")
    s, r = ops.table_topk(torch.zeros(0, 8, device="cuda"), queries, 4, metric=metric)
    assert torch.all(r == -1) and torch.all(s == float(ref.fill(metric)))
    rank = ops.table_rank(torch.zeros(0, 8, device="cuda"), queries, torch.tensor([0, 1, -1], device="cuda"), metric=metric)
    assert rank.tolist() == [-1, -1, -1]
    s, r = ops.table_topk(torch.ones(5, 8, device="cuda"), queries[:0], 4, metric=metric)
    assert s.shape == (0, 4) and r.shape == (0, 4)
    assert ops.table_rank(torch.ones(5, 8, device="cuda"), queries[:0], torch.zeros(0, dtype=torch.int64, device="cuda"),
                          metric=metric).shape == (0,)


# ---- the slab rule: the clamp by the tiles, the shortest last slab, the cap ------------------------
def check_block(torch, ops, table, queries, s, metric, k, exclude, target, tag):
    """check() for many queries: against topk_of_scores / rank_of_scores of the block of scores s
    (test_table_search_host.py holds them against topk / rank)"""
    got_s, got_r = ops.table_topk(table, queries, k, metric=metric, exclude=ids_dev(torch, exclude))
    want = ref.topk_of_scores(s, k, metric, exclude)
    assert same_scores(got_s.cpu().numpy(), want[0]), tag + ("scores",)
    assert np.array_equal(got_r.cpu().numpy(), want[1]), tag + ("rows",)
    got = ops.table_rank(table, queries, ids_dev(torch, target), metric=metric, exclude=ids_dev(torch, exclude))
    assert got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), ref.rank_of_scores(s, target, metric, exclude)), tag + ("rank",)


@pytest.mark.parametrize("metric", ("ip", "l2"))
def test_slabs_clamped_by_the_number_of_tiles(torch_cuda, EA, metric):
    """Q = 32 * 100 + 1 is 101 tiles, so slabs = ceil(2048 / 101) = 21 although N = 30000 has 30
    slabs' worth of rows; N = 21 * 1024 - 1, 21 * 1024 and 21 * 1024 + 1 straddle the row count at
    which the clamp starts to bind (21 slabs of 1024, 1024 and 1025 rows, the last one shorter)"""
    torch, ops = torch_cuda, EA.ops
    d, q, k = 4, 32 * 100 + 1, 10
    tiles = ref.tiles_of(q, d)
    assert tiles == 101 and ref.slabs_of(30000, tiles) == 21 < -(-30000 // ref.MIN_SLAB_ROWS)
    ns = (21 * 1024 - 1, 21 * 1024, 21 * 1024 + 1)
    rng = np.random.default_rng(101)
    t_np = tie_table(rng, ns[-1], d, "bf16")
    q_np = np.array([-2, -1, -0.0, 0, 1, 2], F)[rng.integers(0, 6, (q, d))]
    q_np[1::3] = rng.standard_normal((len(q_np[1::3]), d)).astype(F)
    q_np[2::9] = t_np[rng.integers(0, ns[0], len(q_np[2::9]))]
    table, queries = dev(torch, t_np, "bf16"), dev(torch, q_np)
    assert width(table, queries) == 4
    s_all = ref.scores(t_np, q_np, metric, 4)
    for n in ns:
        assert ref.slabs_of(n, tiles) == 21
        exc, target = rng.integers(-2, n + 2, q), rng.integers(-1, n + 1, q)
        check_block(torch, ops, table[:n], queries, s_all[:, :n], metric, k, exc, target, (metric, n))


def big_flat_case(torch, n, seed, q=5):
    """a tie-heavy bf16 table [n, 4] (4 MiB at n = 2^19) with fp32 queries: small integers, rows of
    the table, random rows"""
    rng = np.random.default_rng(seed)
    t_np = tie_table(rng, n, 4, "bf16")
    small = np.array([-2, -1, -0.0, 0, 1, 2], F)
    q_np = np.concatenate([small[rng.integers(0, 6, (2, 4))], t_np[[n - 1, n // 2 + 7]],
                           rng.standard_normal((q - 4, 4))]).astype(F)
    return rng, t_np, q_np, dev(torch, t_np, "bf16"), dev(torch, q_np)


def test_shortest_last_slab(torch_cuda, EA):
    """N = 511 * 1024 + 1 with one tile: slabs = 512, slab_rows = ceil(N / 512) = 1023 and the last slab
    holds N - 511 * 1023 = 512 rows, the shortest against the others that the rule allows
    (test_table_search_host.py searches every N and tile count).  The best rows of two queries lie in
    the last slab, and the last row is a target."""
    torch, ops = torch_cuda, EA.ops
    n = 511 * 1024 + 1
    slabs = ref.slabs_of(n, 1)
    slab_rows = -(-n // slabs)
    assert (slabs, slab_rows, n - (slabs - 1) * slab_rows) == (512, 1023, 512)
    rng, t_np, q_np, table, queries = big_flat_case(torch, n, 511)
    assert ref.tiles_of(len(q_np), 4) == 1 and width(table, queries) == 4
    last = (slabs - 1) * slab_rows
    t_np[last + 5], t_np[n - 1], t_np[last - 1] = 64 * np.sign(q_np[0]) + (q_np[0] == 0), 64 * q_np[1], 32 * q_np[1]
    table = dev(torch, t_np, "bf16")
    exc = np.array([-1, n - 1, last, n, 5])
    target = np.array([last + 5, n - 1, last, n - 1, -1])
    for metric in ("ip", "l1"):
        s = ref.scores(t_np, q_np, metric, 4)
        if metric == "ip":
            fin = np.where(np.isfinite(s), s, -np.inf)                 # (the table has a NaN row and a row with an inf)
            assert np.argmax(fin[0]) == last + 5 and np.argmax(fin[1]) == n - 1 and np.argsort(fin[1])[-2] == last - 1
        check_block(torch, ops, table, queries, s, metric, 10, exc, target, (metric,))


def test_cap_of_512_slabs(torch_cuda, EA):
    """N = 512 * 1024 + 1 (a 4 MiB bf16 table), Q = 5, k = 64, tie-heavy: slabs = 512, the cap, for
    this and any larger N; the merge walks 512 * 64 entries a query, most of which tie"""
    torch, ops = torch_cuda, EA.ops
    n, k = 512 * 1024 + 1, 64
    assert ref.slabs_of(n, 1) == ref.MAX_SLABS == 512 and -(-n // ref.MIN_SLAB_ROWS) == 513
    assert all(ref.slabs_of(m, 1) == 512 for m in (n + 1, 2 * n, 10 ** 7, 2 ** 31 - 1))
    rng, t_np, q_np, table, queries = big_flat_case(torch, n, 512)
    assert ref.tiles_of(len(q_np), 4) == 1 and width(table, queries) == 4
    exc, target = rng.integers(0, n, 5), rng.integers(0, n, 5)
    exc[0], target[0], target[1] = -1, n - 1, 3
    for metric in ("ip", "cos", "l2"):
        s = ref.scores(t_np, q_np, metric, 4)
        top = ref.topk_of_scores(s, k, metric, exc)[0]
        assert min(len(np.unique(x[~np.isnan(x)])) for x in top) < k // 2, "the table must make ties among the best k"
        check_block(torch, ops, table, queries, s, metric, k, exc, target, (metric,))


# ---- views off a 16-byte boundary: the chunk width rule -----------------------------------------------
def view_at(torch, x_np, dt, off_bytes):
    """the values x_np in a device tensor of type dt that starts off_bytes past a 16-byte boundary"""
    item = ITEM[dt]
    assert off_bytes % item == 0
    base = torch.empty(x_np.size + 16 // item, dtype=_torch_dt(torch, dt), device="cuda")
    assert base.data_ptr() % 16 == 0
    at = off_bytes // item
    view = base[at:at + x_np.size].view(x_np.shape)
    view.copy_(dev(torch, x_np, dt))
    assert view.data_ptr() % 16 == off_bytes and view.is_contiguous()
    return view


@pytest.mark.parametrize("case", ref.ALIGN_CASES, ids=lambda c: "%s+%d-%s+%d-d%d-V%d" % c)
def test_views_off_a_16_byte_boundary(torch_cuda, EA, case):
    """every branch of KgChunkWidth a pair of aligned tables never takes, and V = 1 / 4 where the
    queries are read from memory (d > 3072): N = 1100 (two slabs), Q = 33 (two tiles), the four
    metrics, both ops"""
    torch, ops = torch_cuda, EA.ops
    dtt, off_t, dq, off_q, d, v = case
    n, q = ref.ALIGN_N, ref.ALIGN_Q
    rng = np.random.default_rng(1000 * d + off_t + off_q)
    t_np = tie_table(rng, n, d, dtt)
    q_np, own = queries_for(rng, t_np, dq, q=q)
    table, queries = view_at(torch, t_np, dtt, off_t), view_at(torch, q_np, dq, off_q)
    assert width(table, queries) == v == ref.align_case_width(case)
    assert ref.tiles_of(q, d) == 2 and ref.slabs_of(n, 2) == 2 and ref.wave_queries(d)[1] == (d <= 3072)
    exc = np.concatenate([own, rng.integers(-2, n + 2, q - len(own))])
    target = rng.integers(-1, n + 1, q)
    for metric in METRICS:
        check(torch, ops, table, queries, t_np, q_np, metric, 10, exc, target, tag=case + (metric,))


# ---- the list under chosen arrival orders -----------------------------------------------------------
@pytest.mark.parametrize("metric", ("ip", "l2"))
@pytest.mark.parametrize("kind", ref.ARRIVAL_ORDERS)
def test_arrival_orders(torch_cuda, EA, kind, metric):
    """scores chosen row by row (table_search_ref.arrival_case): every row entering at position 0,
    no row entering a full list, all rows tied, a sawtooth, +0 / -0; N = 2049 is three slabs;
    d = 1 offers 256 candidates a step, d = 64 four; k = 1, 63 and 64"""
    torch, ops = torch_cuda, EA.ops
    n = ref.ARRIVAL_N
    assert ref.slabs_of(n, 1) == 3
    exc = np.array([-1, n - 1, 0])
    target = np.array([0, 683, n - 1])
    for d in ref.ARRIVAL_DIMS:
        t_np, q_np = ref.arrival_case(kind, metric, d)
        table, queries = dev(torch, t_np), dev(torch, q_np)
        s = None
        for k in ref.ARRIVAL_KS:
            s = check(torch, ops, table, queries, t_np, q_np, metric, k, None, target if k == 1 else None, s=s,
                      tag=(kind, metric, d, k))
            check(torch, ops, table, queries, t_np, q_np, metric, k, exc, target if k == 64 else None, s=s,
                  tag=(kind, metric, d, k, "exclude"))


@pytest.mark.parametrize("metric", METRICS)
def test_query_with_a_nan(torch_cuda, EA, metric):
    """every score of the query is NaN: its list is rows 0 .. k - 1 in row order (without the
    excluded one), its rank 0; the query beside it in the same wave is not disturbed"""
    torch, ops = torch_cuda, EA.ops
    n = ref.ARRIVAL_N
    for d in ref.ARRIVAL_DIMS:
        rng = np.random.default_rng(d)
        t_np = rng.standard_normal((n, d)).astype(F)
        q_np = rng.standard_normal((3, d)).astype(F)
        q_np[0, d // 2], q_np[2, 0] = np.nan, np.nan
        table, queries = dev(torch, t_np), dev(torch, q_np)
        s = ref.scores(t_np, q_np, metric, width(table, queries))
        assert np.all(np.isnan(s[[0, 2]])) and not np.any(np.isnan(s[1]))
        for k in (1, 64):
            got_s, got_r = ops.table_topk(table, queries, k, metric=metric, exclude=ids_dev(torch, [-1, 0, 3]))
            got_s, got_r = got_s.cpu().numpy(), got_r.cpu().numpy()
            assert got_r[0].tolist() == list(range(k)) and got_r[2].tolist() == [r for r in range(k + 1) if r != 3][:k]
            assert np.all(np.isnan(got_s[[0, 2]]))
            check(torch, ops, table, queries, t_np, q_np, metric, k, [-1, 0, 3], [5, 700, n - 1], s=s, tag=(metric, d, k))
        got = ops.table_rank(table, queries, ids_dev(torch, [5, 700, n - 1]), metric=metric).cpu().numpy()
        assert got[0] == 0 and got[2] == 0 and got[1] == ref.rank(t_np, q_np, [5, 700, n - 1], metric, 0, s=s)[1]


@pytest.mark.parametrize("metric", ("ip", "l1"))
def test_row_that_scores_the_fill_value(torch_cuda, EA, metric):
    """a row holding -inf under ip (+inf under l1) against positive queries scores the fill value: it
    is a candidate like any other - returned with its own row number behind every other row and ahead
    of the -1 entries when N < k; when every row scores the fill, the list is the rows in order"""
    torch, ops = torch_cuda, EA.ops
    worst = F(-np.inf) if metric == "ip" else F(np.inf)
    rng = np.random.default_rng(6)
    for d in (1, 4, 64):
        n, k = 5, 8
        t_np = (np.abs(rng.standard_normal((n, d))) + 1).astype(F)
        q_np = (np.abs(rng.standard_normal((2, d))) + 1).astype(F)
        t_np[2, d // 2] = worst
        table, queries = dev(torch, t_np), dev(torch, q_np)
        s = check(torch, ops, table, queries, t_np, q_np, metric, k, None, [2, 0], tag=(metric, d, "one"))
        assert np.all(s[:, 2] == worst) and np.all(np.isfinite(np.delete(s, 2, 1)))
        got_s, got_r = (x.cpu().numpy() for x in ops.table_topk(table, queries, k, metric=metric))
        assert np.all(got_r[:, 4] == 2) and np.all(got_s[:, 4:] == worst) and np.all(got_r[:, 5:] == -1)
        # every row of three slabs scores the fill value
        n = ref.ARRIVAL_N
        t_np = (np.abs(rng.standard_normal((n, d))) + 1).astype(F)
        t_np[:, d // 2] = worst
        t_np[1000, :] = 1
        table = dev(torch, t_np)
        for k in (1, 64):
            s = check(torch, ops, table, queries, t_np, q_np, metric, k, [1000, 0], [1000, 7], tag=(metric, d, k, "all"))
            check(torch, ops, table, queries, t_np, q_np, metric, k, None, [1000, 7], s=s, tag=(metric, d, k, "all"))
        assert np.count_nonzero(s[0] == worst) == n - 1
        got_r = ops.table_topk(table, queries, 64, metric=metric)[1].cpu().numpy()
        assert got_r[0].tolist() == [1000] + list(range(63))


# ---- table_rank against float64 -----------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_rank_equals_the_float64_count(torch_cuda, EA, metric):
    """well-separated random fp32 rows (N = 3073, d = 64, Q = 33): no row's float64 score lies within
    2 * bound of a target's (scores64's bound of the fp32 arithmetic), so the rank is the float64
    count - a check that shares no arithmetic with the kernels or the restatement.  The metrics of
    rank_metric follow from it."""
    torch, ops = torch_cuda, EA.ops
    t_np, q_np, target, count, margin = ref.separated_rank_case(metric, **ref.SEPARATED)
    assert margin > 1 and count.min() == 0 and count.max() == 3072
    exact, _ = ref.scores64(t_np, q_np, metric)
    st = np.take_along_axis(exact, target[:, None], 1)
    assert np.array_equal(count, ((exact >= st) if ref.larger_is_better(metric) else (exact <= st)).sum(1) - 1)
    rank = ops.table_rank(dev(torch, t_np), dev(torch, q_np), ids_dev(torch, target), metric=metric)
    assert np.array_equal(rank.cpu().numpy(), count)
    want = torch.from_numpy(count)
    for name in ("mrr", "mr", "hit1", "hit10"):
        assert float(ops.rank_metric(name, rank.cpu())) == float(ops.rank_metric(name, want)), name
    # mr and hit@k are sums of integers and one division: the same on the device and in numpy
    assert float(ops.rank_metric("mr", rank)) == (count.astype(np.float64) + 1).sum() / len(count)
    assert float(ops.rank_metric("hit10", rank)) == np.count_nonzero(count < 10) / len(count)
