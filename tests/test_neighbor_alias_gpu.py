"""The alias neighbour mode on the GPU (euler_amd/csrc/nb_alias_kernels.hip): the device-built
tables and the draws against the numpy restatement tests/neighbor_alias_ref.py, bit for bit; the
exact mode untouched by it; and the output distribution against the exact probabilities with the
runners of tests/sampling_stats.py over a backend that forwards with method="alias".

Distribution.  The model p of every case is the exact mode's, from the f32 running sums.  What an
alias table draws, q, differs from p by the rounding of its build: at most
neighbor_alias_ref.mass_bound(d) per entry (derived there; (8 d + 5) 2^-24 to first order, 8.0e-6 at
d = 16).  The noncentrality that gives Pearson's statistic, N sum (q - p)^2 / p, at the N = 8.4 M
draws per row of these cases: entries that start on the small stack are off by a RELATIVE (d + 2)
2^-24, entries that were ever on the large stack (p > 1 / d) by the bound, so it is at most
N d^2 bound^2 = 0.14 at d = 16 - and tests/test_neighbor_alias_host.py computes it from the
restated tables of the very motifs used here: 9.2e-4 at most, the hub's 6 000-entry row in its 32
bins included.  A level-1e-7 test at these degrees of freedom needs a noncentrality above 100
(sampling_stats.lambda_needed) to reject reliably: a correct table cannot fail for its rounding.

Graphs have at most 4 096 rows, except where the runners fix the size (R_GPU copies of a 16-row
motif; the hub motif is 8 192 rows a copy)."""
import os

import numpy as np
import pytest

import neighbor_alias_ref as ref
import sampling_stats as S

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("SAMPLING_STATS_SEED", S.SEED))
REPORT = S.Report()
_CACHE = {}


def _graph_of(EA, csr):
    return EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w, csr.type_prefix,
                             csr.n_types, csr.node_type, csr.node_weight)


def _edge_case_raw():
    """T = 3, ids 10 .. : every kind of row the draw has a rule for."""
    rows = [
        [([11, 12, 13, 14], [1, 2, 3, 4]), ([15, 16], [1, 1]), ([17, 18, 19], [5, 1, 1])],
        [([], []), ([11, 12, 13], [1, 2, 3]), ([14, 15], [4, 4])],              # empty group 0
        [([10, 15], [1, 2]), ([16, 17], [0, 0]), ([18, 11, 12], [3, 1, 2])],    # all-zero group 1
        [([0], [1.0]), ([0, 13], [1, 1]), ([13], [2])],                         # neighbour id 0 (Q1)
        [([0, 12, 0, 14], [3, 1, 3, 1]), ([], []), ([0], [1])],                 # mostly id 0
        [([], []), ([], []), ([], [])],                                         # no neighbours
        [([12, 13, 14, 15, 16], [0, 3, 0, 1, 0]), ([10], [2.5]), ([11, 12], [1e3, 1e-3])],   # zeros first and last
        [([10 + i for i in range(20)], [2.0 ** -i for i in range(20)]), ([11], [0]), ([12, 13], [7, 7])],
    ]
    rid, seg, nbr, w = [], [0], [], []
    for i, row in enumerate(rows):
        rid.append(10 + i)
        for ids, ws in row:
            nbr += ids
            w += ws
            seg.append(len(nbr))
    # ids 18, 19: rows only some lists point at do not exist (unknown ids downstream)
    return (np.asarray(rid, np.uint64), np.asarray(seg, np.int64), np.asarray(nbr, np.uint64), np.asarray(w, np.float32))


def _pareto_raw(n=2048, deg=256):
    rng = np.random.default_rng(1613)
    rid = np.arange(1, n + 1, dtype=np.uint64)
    seg = np.arange(n + 1, dtype=np.int64) * deg
    r = np.repeat(np.arange(n, dtype=np.int64), deg)
    i = np.tile(np.arange(deg, dtype=np.int64), n)
    nbr = ((r + 1 + 7 * i) % n + 1).astype(np.uint64)            # 256 distinct ids per row
    w = ((rng.pareto(0.7, n * deg) + 1) * 0.5).astype(np.float32)
    return rid, seg, nbr, w


def graph(EA, O, name):
    """(csr, restated tables, euler_amd.Graph with its tables built) of a small graph, once per run"""
    if name not in _CACHE:
        if name == "fixture":
            from conftest import GOLDEN, load_csr
            csr = load_csr(O, os.path.join(GOLDEN, "fixture_graph.npz"))
        elif name == "edges":
            csr = O.csr_from_raw(*_edge_case_raw(), 3)
        elif name == "pareto":
            csr = O.csr_from_raw(*_pareto_raw(), 1)
        else:
            gname, R = name.split(":")
            rep = S.replicas(gname, int(R))
            rid, seg, nbr, w = rep.raw()
            csr = O.csr_from_raw(rid, seg, nbr, w, rep.T)
        G = _graph_of(EA, csr)
        G.build_neighbor_alias()
        _CACHE[name] = (csr, ref.Tables(csr), G)
    return _CACHE[name]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.int64 else a


def assert_draw_equal(got, want, what):
    """(ids, weights, types[, mask]) tensors == the restatement's arrays, bit for bit"""
    for g, w, name in zip(got, want, ("ids", "weights", "types", "mask")):
        g = g.cpu().numpy().reshape(w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name, np.argwhere(bits(g) != bits(w))[:6].tolist())


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("name", ["fixture", "edges", "typed:4", "hub:1", "hashed:8"])
def test_export_equals_the_restatement(EA, O, name):
    csr, T, G = graph(EA, O, name)
    ids = np.concatenate([csr.row_id, [np.uint64(2 ** 41 + 1)], csr.row_id[:2]])      # an unknown id, repeats
    got = G.neighbor_alias_rows(ids)
    want = T.rows(ids)
    for g, w, what in zip(got, want, ("row_ptr", "id_self", "id_alias", "prob", "w_self", "w_alias")):
        assert g.dtype == w.dtype and np.array_equal(bits(g), bits(w)), (name, what)
    assert np.array_equal(got[0], G.export_rows(ids)[0])
    zero = T.w_self[:len(csr.nbr)] == 0
    assert not T.prob[zero].any(), "an edge of weight 0 with prob != 0"


def test_bytes_and_no_other_index(EA, O):
    """neighbor_alias() is (0, 0) before the build and (32 E, E) after; device_bytes grows by exactly
    that - so nothing else was built - on the explicit build and, on a second graph, on the first
    alias call; a second build changes nothing."""
    import torch
    from euler_amd._lib import EulerGpuError
    csr = graph(EA, O, "plain:64")[0]
    E = len(csr.nbr)
    roots = torch.as_tensor(csr.row_id[:256].astype(np.int64)).cuda()
    for how in ("explicit", "first call"):
        G = _graph_of(EA, csr)
        assert G.neighbor_alias() == (0, 0)
        with pytest.raises(EulerGpuError):
            G.neighbor_alias_rows(csr.row_id[:1])
        before = G.device_bytes
        if how == "explicit":
            G.build_neighbor_alias()
        else:
            G.sample_neighbor(roots, [0], 5, method="alias")
        assert G.neighbor_alias() == (32 * E, E)
        assert G.device_bytes == before + 32 * E
        G.build_neighbor_alias()
        G.sample_fanout(roots, [[0], [0]], [3, 2], method="alias")
        torch.cuda.synchronize()
        assert G.device_bytes == before + 32 * E and G.neighbor_alias() == (32 * E, E)


def test_method_argument(EA, O):
    import torch
    _, _, G = graph(EA, O, "edges")
    r = torch.arange(10, 18).cuda()
    for bad in ("Alias", "", "cdf", 1):
        with pytest.raises(ValueError):
            G.sample_neighbor(r, [0], 2, method=bad)
        with pytest.raises(ValueError):
            G.sample_fanout(r, [[0], [0]], [2, 2], method=bad)
        with pytest.raises(ValueError):
            G.set_neighbor_method(bad)
    a = G.sample_neighbor(r, [0], 4, call_id=3, method="alias", dedup=False)        # dedup: accepted, ignored
    b = G.sample_neighbor(r, [0], 4, call_id=3, method="alias", dedup=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    G.set_neighbor_method("alias")
    try:
        c = G.sample_neighbor(r, [0], 4, call_id=3)
        f1 = G.sample_fanout(r, [[0], [2]], [3, 2], call_id=9)
    finally:
        G.set_neighbor_method("exact")
    f2 = G.sample_fanout(r, [[0], [2]], [3, 2], call_id=9, method="alias")
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    assert all(torch.equal(x, y) for p, q in zip(f1, f2) for x, y in zip(p, q))


def test_non_monotone_graph_is_refused(EA, O):
    """negative weights: EINVAL from the build and from a draw, the graph left as it was"""
    import torch
    from euler_amd._lib import EulerGpuError
    rid = np.arange(1, 5, dtype=np.uint64)
    pw = np.asarray([3, 1, 2, 4, 1, 2, 1, 2], np.float32)          # row 0's running sums decrease
    G = EA.Graph.from_csr(rid, np.arange(5, dtype=np.int64) * 2, np.full(4, 2, np.int32),
                          np.tile(np.asarray([1, 2], np.uint64), 4), pw, pw[1::2].copy(), 1)
    before = G.device_bytes
    for call in (G.build_neighbor_alias, lambda: G.sample_neighbor(torch.arange(1, 5).cuda(), [0], 3, method="alias")):
        with pytest.raises(EulerGpuError) as e:
            call()
        assert e.value.code == -1 and "negative" in str(e.value)
    assert G.neighbor_alias() == (0, 0) and G.device_bytes == before
    G.sample_neighbor(torch.arange(1, 5).cuda(), [0], 3)          # the exact mode still serves it


# ------------------------------------------------------------------ draws
TYPE_LISTS = [[0], [2], [1], [2, 0], [], [0, 1, 2], [1, 0, 2, 1], [3], [-1], [1, 5]]


@pytest.mark.parametrize("layout", ["tf", "core"])
@pytest.mark.parametrize("count", [1, 2, 25, 63, 64, 65])
def test_draws_equal_the_restatement(EA, O, count, layout):
    """k = 1, a 2-of-3 sub-list in non-ascending order, k = 0, k >= T, invalid types; unknown ids,
    an empty listed group, an all-zero group, rows whose first drawn id is 0 (Q1); duplicates."""
    import torch
    csr, T, G = graph(EA, O, "edges")
    roots = np.concatenate([csr.row_id, [0, 18, 19, 2 ** 40 + 7], csr.row_id[[3, 3, 0]]]).astype(np.uint64)
    rt = torch.as_tensor(roots.astype(np.int64)).cuda()
    G.set_seed(SEED)
    for c, et in enumerate(TYPE_LISTS):
        got = G.sample_neighbor(rt, et, count, default_node=-7, layout=layout, call_id=500 + c, return_mask=True,
                                method="alias")
        want = ref.sample_neighbor(T, O, SEED, 500 + c, roots, et, count, layout, -7)
        assert_draw_equal(got, want, (et, count, layout))
        # duplicate roots get identical rows
        assert torch.equal(got[0][3], got[0][-3]) and torch.equal(got[0][3], got[0][-2]) and \
            torch.equal(got[0][0], got[0][-1])
    if layout == "tf":
        first = ref.sample_neighbor(T, O, SEED, 500, roots, [0], count, "core", -7)[0][:, 0]
        assert (first[[3, 4]] == 0).any() or count == 0, "no row of this case starts with id 0"


def test_fixture_and_typed_graphs(EA, O):
    import torch
    for name in ("fixture", "typed:4", "hashed:8"):
        csr, T, G = graph(EA, O, name)
        roots = np.concatenate([csr.row_id[:48], [np.uint64(5 * 2 ** 33)]])
        rt = torch.as_tensor(roots.astype(np.int64)).cuda()
        G.set_seed(SEED + 1)
        for c, et in enumerate([[0], [csr.n_types - 1], [], [1, 0]]):
            for layout in ("tf", "core"):
                got = G.sample_neighbor(rt, et, 7, layout=layout, call_id=c, return_mask=True, method="alias")
                assert_draw_equal(got, ref.sample_neighbor(T, O, SEED + 1, c, roots, et, 7, layout), (name, et, layout))


def test_empty_calls(EA, O):
    import torch
    _, _, G = graph(EA, O, "edges")
    none = torch.zeros(0, dtype=torch.int64).cuda()
    a = G.sample_neighbor(none, [0], 5, method="alias")
    b = G.sample_neighbor(torch.arange(10, 14).cuda(), [0], 0, method="alias")
    assert a[0].shape == (0, 5) and b[0].shape == (4, 0)
    f = G.sample_fanout(none, [[0], [0]], [3, 2], method="alias")
    assert [x.numel() for x in f[0]] == [0, 0, 0]
    torch.cuda.synchronize()


@pytest.mark.parametrize("group", [1, 25])
def test_root_mask(EA, O, group):
    import torch
    csr, T, G = graph(EA, O, "edges")
    parents = 6
    rng = np.random.default_rng(group)
    roots = rng.choice(csr.row_id, parents * group).astype(np.uint64)
    mask = np.asarray([0, 1, 0, 0, 1, 1], np.uint8)
    G.set_seed(SEED)
    for layout in ("tf", "core"):
        got = G.sample_neighbor(torch.as_tensor(roots.astype(np.int64)).cuda(), [0, 2], 3, layout=layout, call_id=77,
                                return_mask=True, method="alias", root_mask=torch.as_tensor(mask).cuda(),
                                root_group=group)
        want = ref.sample_neighbor(T, O, SEED, 77, roots, [0, 2], 3, layout, -1, mask, group)
        assert_draw_equal(got, want, (group, layout))


def test_one_workgroup_past_the_grid_cap(EA, O):
    """The launcher caps its grid at 4 096 workgroups of 256 lanes (GridFor): 16 388 roots x 64
    samples are one workgroup more, taken by the grid-stride loop.  The roots repeat 64 ids, so the
    restatement of those 64 rows is the whole answer."""
    import torch
    csr, T, G = graph(EA, O, "plain:64")
    n, count = 4096 * 256 // 64 + 4, 64
    base = csr.row_id[:64]
    idx = (np.arange(n) * 37) % 64
    G.set_seed(SEED)
    got = G.sample_neighbor(torch.as_tensor(base[idx].astype(np.int64)).cuda(), [0], count, call_id=5, return_mask=True,
                            method="alias")
    want = ref.sample_neighbor(T, O, SEED, 5, base, [0], count)
    assert_draw_equal(got, [w[idx] for w in want], "grid cap")


@pytest.mark.parametrize("counts", [[3, 2], [25, 10]])
def test_fanout(EA, O, counts):
    """== hop-by-hop sample_neighbor(method="alias") chained by the documented mask rule (hop h's
    roots are hop h - 1's TF-layout ids; the rows under a default row sample as node id 0), and ==
    the restatement; the roots include rows without samples, unknown ids and a Q1 row."""
    import torch
    for name, types in (("edges", [[0], [2]]), ("edges", [[1, 0], [2, 0]]), ("edges", [[0, 1, 2], [2, 1, 0]]),
                        ("typed:4", [[0, 2], [2, 1]])):
        csr, T, G = graph(EA, O, name)
        roots = np.concatenate([csr.row_id[:24], [np.uint64(999999)]])
        rt = torch.as_tensor(roots.astype(np.int64)).cuda()
        G.set_seed(SEED)
        nb, w, t = G.sample_fanout(rt, types, counts, default_node=-1, call_id=30, method="alias")
        want = ref.sample_fanout(T, O, SEED, 30, roots, types, counts)
        cur, mask, group = rt, None, 1
        for h, c in enumerate(counts):
            step = G.sample_neighbor(cur, types[h], c, call_id=30 + h, return_mask=True, method="alias", root_mask=mask,
                                     root_group=group)
            for a, b in zip((nb[h + 1], w[h], t[h]), step):
                assert torch.equal(a.reshape(-1), b.reshape(-1)), (name, types, h)
            assert_draw_equal((nb[h + 1], w[h], t[h]), want[h], (name, types, h))
            cur, mask, group = step[0].reshape(-1), step[3], c
        if name == "edges":
            assert bool((nb[1] == -1).any()), "no default hop-1 row in this case"


def test_exact_mode_is_untouched(EA, O):
    """Fixed seeds: sample_neighbor / sample_fanout with the default method give the same bits before
    and after build_neighbor_alias(), and under set_neighbor_method("exact")."""
    import torch
    csr = graph(EA, O, "typed:4")[0]
    G = _graph_of(EA, csr)
    rt = torch.as_tensor(csr.row_id.astype(np.int64)).cuda()
    G.set_seed(SEED)

    def exact():
        out = []
        for et in ([0], [2, 0], []):
            out += list(G.sample_neighbor(rt, et, 8, call_id=11))
            out += list(G.sample_neighbor(rt, et, 5, call_id=12, layout="core"))
        for part in G.sample_fanout(rt, [[0], [2]], [4, 2], call_id=20):
            out += part
        return out

    before = exact()
    G.build_neighbor_alias()
    G.sample_neighbor(rt, [0], 8, call_id=11, method="alias")
    after = exact()
    G.set_neighbor_method("exact")
    named = exact()
    assert len(before) == len(after) == len(named)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(before, after, named))
    alias = G.sample_neighbor(rt, [0], 8, call_id=11, method="alias")[0]
    assert not torch.equal(alias, before[0]), "the alias mode returned the exact mode's neighbours"


# ------------------------------------------------------------------ distribution
class AliasBackend:
    """euler_amd.Graph behind the runners' call signatures, every draw with method="alias"."""

    def __init__(self, G):
        self.G = G

    def set_seed(self, seed, call_id=0):
        self.G.set_seed(seed, call_id)

    def sample_neighbor(self, nodes, edge_types, count, default_node=-1, layout="tf", call_id=None):
        return self.G.sample_neighbor(nodes, edge_types, count, default_node, layout=layout, call_id=call_id,
                                      method="alias")

    def sample_fanout(self, nodes, edge_types, counts, default_node=-1, call_id=None):
        return self.G.sample_fanout(nodes, edge_types, counts, default_node, call_id=call_id, method="alias")


_BIG = {}


def big(EA, O, name, R=S.R_GPU):
    if (name, R) not in _BIG:
        rep = S.replicas(name, R)
        rid, seg, nbr, w = rep.raw()
        G = _graph_of(EA, O.csr_from_raw(rid, seg, nbr, w, rep.T))
        _BIG[(name, R)] = (rep, AliasBackend(G))
    return _BIG[(name, R)]


ALIAS_CASES = ["nb_plain_tf_even", "nb_plain_core_odd", "nb_hashed_tf_odd", "nb_typed_one", "nb_typed_several_odd",
               "nb_typed_none_listed", "nb_uniform", "fanout_plain", "fanout_hashed", "fanout_typed_several"]


@pytest.mark.parametrize("name", ALIAS_CASES)
def test_neighbor_marginals(EA, O, torch_cuda, name):
    """gof per motif row against the exact model, then pooled; default rows must be the fill exactly
    and ids of weight 0 must never appear (tally / judge_rows assert both)."""
    case = next(c for c in S.NEIGHBOR_CASES if c["name"] == name)
    rep, B = big(EA, O, case["graph"])
    assert not S.run_neighbor_case(B, torch_cuda, "cuda", rep, case, SEED, REPORT)


def test_hub_neighbor(EA, O, torch_cuda):
    rep, B = big(EA, O, "hub", S.R_HUB)
    assert not S.run_hub_neighbor(B, torch_cuda, "cuda", rep, SEED, REPORT)


@pytest.mark.parametrize("parity", ["even", "odd"])
def test_pairs_draws(EA, O, torch_cuda, parity):
    """Samples j and j + 1 of one root (two Philox blocks each: type / column + coin)."""
    rep, B = big(EA, O, "plain")
    t = S.pairs_draws(B, torch_cuda, "cuda", rep, SEED, 0 if parity == "even" else 1)
    assert not S.judge_pairs(REPORT, "alias_pair_draws_" + parity, t)


@pytest.mark.parametrize("what", ["calls", "seeds"])
def test_pairs_calls_seeds(EA, O, torch_cuda, what):
    rep, B = big(EA, O, "plain")
    assert not S.judge_pairs(REPORT, "alias_pair_" + what, S.pairs_calls_or_seeds(B, torch_cuda, "cuda", rep, SEED, what))


def test_pairs_node_ids(EA, O, torch_cuda):
    rep, B = big(EA, O, "rowmajor")
    assert not S.judge_pairs(REPORT, "alias_pair_ids", S.pairs_ids(B, torch_cuda, "cuda", rep, SEED))


def test_long_marginal_of_one_row(EA, O, torch_cuda):
    """Column and coin are the two halves of ONE Philox block.  A coin that shared bits with the
    column would pick `self` more often in some columns than prob says, which bends the marginal:
    the row of weights 1 .. 16 at 4 x the marginal cases' N."""
    torch = torch_cuda
    rep, B = big(EA, O, "plain")
    x, roots = S._row_roots(torch, rep, "cuda", 0)
    B.set_seed(SEED)
    t = np.zeros(rep.M + 1, np.int64)
    calls = 16
    for c in range(calls):
        ids = B.sample_neighbor(roots, [0], 64, -1, call_id=61000 + c)[0]
        pos, _ = S._decode(torch, rep, ids, -1)
        t += torch.bincount(pos.reshape(-1), minlength=rep.M + 1).cpu().numpy()
    assert t[-1] == 0
    assert not S._judge_flat(REPORT, "alias_w1..16_long", t[:-1], rep.motif.model(0, [0]), rep.R * 64 * calls)


# ------------------------------------------------------------------ heavy tail
def test_heavy_tailed_graph(EA, O, torch_cuda):
    """2 048 rows of 256 Pareto(0.7) weights: the weight-bucket index overflows (asserted:
    index_overflow_rows() is non-empty, the condition under which the lean kernels decline it).
    Alias draws equal the restatement there, and the marginals of the 16 heaviest rows pass gof
    against the exact model."""
    torch = torch_cuda
    csr, T, G = graph(EA, O, "pareto")
    assert len(G.index_overflow_rows()) > 0
    roots = csr.row_id[:40]
    G.set_seed(SEED)
    got = G.sample_neighbor(torch.as_tensor(roots.astype(np.int64)).cuda(), [0], 25, call_id=1, return_mask=True,
                            method="alias")
    assert_draw_equal(got, ref.sample_neighbor(T, O, SEED, 1, roots, [0], 25), "pareto")
    deg = 256
    pw = csr.prefix_w.reshape(-1, deg).astype(np.float64)
    heavy = np.argsort(-pw[:, -1])[:16]
    count, calls = 4096, 8
    rt = torch.as_tensor(csr.row_id[heavy].astype(np.int64)).cuda()
    lut = torch.full((16, len(csr.row_id) + 1), -1, dtype=torch.int64, device="cuda")
    for a, r in enumerate(heavy):
        lut[a, torch.as_tensor(csr.nbr[r * deg:(r + 1) * deg].astype(np.int64)).cuda()] = torch.arange(deg, device="cuda")
    t = torch.zeros(16, deg, dtype=torch.int64, device="cuda")
    for c in range(calls):
        ids = G.sample_neighbor(rt, [0], count, call_id=100 + c, method="alias")[0]
        e = torch.gather(lut, 1, ids)
        assert int(e.min()) >= 0
        t += torch.zeros_like(t).scatter_add_(1, e, torch.ones_like(e))
    t = t.cpu().numpy()
    bad = []
    for a, r in enumerate(heavy):
        p = np.diff(np.concatenate([[0.0], pw[r]])) / pw[r, -1]
        bad += S._judge_flat(REPORT, "alias_pareto/row%d" % r, t[a], p, count * calls)
    assert not bad, bad
