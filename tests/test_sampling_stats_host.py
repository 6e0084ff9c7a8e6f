"""The sampling-distribution harness checked without a GPU (tests/sampling_stats.py).

1. Unit checks of chi2_sf, the merging rule and gof's hard assertions.
2. Power: every statistic of tests/test_sampling_distribution_gpu.py, taken from the one
   table both files import (sampling_stats.power_table), accepts samples that numpy's own
   generator draws from the exact `p` at the case's `N` and rejects samples drawn from each
   planted `q`.  That is what shows the GPU tests would fail on a subtly wrong kernel.
3. The same battery on the CPU oracle, through the runners the GPU file uses.  It tells a
   fault of the RNG contract (oracle and GPU both fail) from a kernel fault (GPU only).
   The GPU is bit-identical to the oracle, so a GPU case run at the same size prints the
   same statistic (not asserted).  Sizes: the pair cases on sample_neighbor run at the GPU
   file's size; everything else runs with R (copies) / batch rows / calls cut by the
   factor stated at each test, to keep the file near a minute.

Acceptance: p-value >= 1e-7 everywhere (sampling_stats.LEVEL).
"""
import math

import numpy as np
import pytest

import sampling_stats as S


# ------------------------------------------------------------------ 1. the harness itself
# (x, df, survival function) from standard chi-square tables / closed forms:
# df = 2: exp(-x / 2); df = 1: erfc(sqrt(x / 2)); the rest are the 1e-7 critical values
# and textbook percentage points
CHI2_TABLE = [
    (3.841458820694124, 1, 0.05),
    (6.634896601021213, 1, 0.01),
    (10.827566170662733, 1, 0.001),
    (5.991464547107979, 2, 0.05),
    (18.307038053275146, 10, 0.05),
    (23.209251158954356, 10, 0.01),
    (124.34211340400407, 100, 0.05),
    (2.0 * math.log(1e12), 2, 1e-12),
    (2.0 * math.log(1e7), 2, 1e-7),
]


@pytest.mark.parametrize("x,df,want", CHI2_TABLE)
def test_chi2_sf_table(x, df, want):
    assert S.chi2_sf(x, df) == pytest.approx(want, rel=1e-9)


def test_chi2_sf_closed_forms_far_tail():
    for x in (0.5, 5.0, 30.0, 60.0, 120.0):
        assert S.chi2_sf(x, 1) == pytest.approx(math.erfc(math.sqrt(x / 2)), rel=1e-10)
        assert S.chi2_sf(x, 2) == pytest.approx(math.exp(-x / 2), rel=1e-12)
        # df = 4: exp(-x/2) (1 + x/2)
        assert S.chi2_sf(x, 4) == pytest.approx(math.exp(-x / 2) * (1 + x / 2), rel=1e-10)
    assert S.chi2_sf(0.0, 7) == 1.0 and S.chi2_sf(10.0, 0) == 1.0


def test_chi2_sf_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    for df in (1, 2, 3, 15, 63, 255, 1023, 4000):
        for x in np.concatenate([np.linspace(0.01, 3 * df + 80, 60), [df, df + 1.0, df + 0.999]]):
            want = stats.chi2.sf(x, df)
            if want > 1e-280:
                assert S.chi2_sf(x, df) == pytest.approx(want, rel=2e-9, abs=1e-300), (x, df)
    # the critical values the sizing table quotes
    for df, crit in ((1, 28.4), (3, 35.4), (15, 62.3), (63, 139.6), (255, 390.2), (1023, 1275.8)):
        assert stats.chi2.isf(1e-7, df) == pytest.approx(crit, abs=0.06)
        assert 0.9e-7 < S.chi2_sf(crit, df) < 1.1e-7


def test_merging_never_drops_mass():
    rng = np.random.default_rng(5)
    for trial in range(200):
        k = int(rng.integers(1, 60))
        e = rng.random(k) * rng.choice([0.1, 5.0, 80.0, 400.0])
        groups = S.merge_cells(e, 50)
        flat = [i for g in groups for i in g]
        assert flat == list(range(k)), "every cell in exactly one group, in order"
        sums = [e[g].sum() for g in groups]
        assert sum(sums) == pytest.approx(e.sum(), rel=1e-12)
        if e.sum() >= 50:
            assert min(sums) >= 50


def test_gof_merges_light_cells_and_keeps_every_count():
    p = np.array([0.5, 0.25, 0.125, 0.0625, 0.0625 - 3e-6, 1e-6, 1e-6, 1e-6])
    N = 1_000_000
    counts = np.random.default_rng(6).multinomial(N, p)
    stat, df, pv = S.gof(counts, p, 50, N)
    assert df == 4 and pv > 1e-3          # the three cells of expectation 1 joined their neighbour
    # moving mass between two MERGED cells changes nothing; out of the group it does
    c2 = counts.copy()
    c2[-1] += c2[-2]
    c2[-2] = 0
    assert S.gof(c2, p, 50, N)[0] == stat
    c3 = counts.copy()
    c3[0] -= 5000
    c3[-1] += 5000
    assert S.gof(c3, p, 50, N)[2] < 1e-7


def test_gof_hard_assertions():
    p = np.array([0.0, 0.5, 0.5, 0.0])
    with pytest.raises(AssertionError, match="probability 0"):
        S.gof([0, 50, 49, 1], p, 50, 100)             # the zero-weight last entry was drawn
    with pytest.raises(AssertionError, match="unaccounted"):
        S.gof([0, 50, 49, 0], p, 50, 100)             # a draw went missing
    stat, df, pv = S.gof([0, 50, 50, 0], p, 50, 100)
    assert (stat, df) == (0.0, 1) and pv == 1.0
    # a single possible outcome: no statistic, all in the assertions
    assert S.gof([0, 100], [0.0, 1.0], 50, 100) == (0.0, 0, 1.0)


def test_noncentrality_and_sizing_figures():
    p = np.arange(1, 17) / 136.0
    q = S.planted_marginal(p)["light"]
    assert q[0] == pytest.approx(1.05 / 136) and q.sum() == pytest.approx(1.0)
    # the issue's figure: +5 % on the lightest of weights 1..16 gives ~76 at N = 4.2 M
    assert S.noncentrality(p, q, 4_194_304) == pytest.approx(77.7, abs=1.0)
    u = np.full(8, 0.125)
    lam = S.noncentrality(np.outer(u, u), S.planted_pair(u, u, 0.005), 1)
    assert lam == pytest.approx(1.75e-4, rel=1e-6)
    assert S.lambda_needed(15) == 143 and S.lambda_needed(16) == 201 and S.lambda_needed(63) == 201


def test_pair_independence_sees_marginal_bias_and_dependence():
    rng = np.random.default_rng(8)
    u = np.full(8, 0.125)
    N = S.PAIR_MIN_N
    ok = rng.multinomial(N, np.outer(u, u).reshape(-1)).reshape(8, 8)
    assert S.pair_independence(ok, u, u, 50, N)[2] >= S.LEVEL
    dep = rng.multinomial(N, S.planted_pair(u, u).reshape(-1)).reshape(8, 8)
    assert S.pair_independence(dep, u, u, 50, N)[2] < S.LEVEL
    # identical draws (two hops on one call id): everything on the diagonal
    same = np.diag(rng.multinomial(N, u))
    assert S.pair_independence(same, u, u, 50, N)[2] == 0.0


# ------------------------------------------------------------------ 2. power
POWER = S.power_table()


def test_power_table_is_sized():
    """Every planted bias of every statistic reaches the noncentrality its degrees of
    freedom need (node2vec rows: wherever the fault changes the row at all)."""
    assert len(POWER) > 300
    weak = []
    for label, p, N, planted in POWER:
        nz = p > 0
        df = max(len(S.merge_cells(p[nz] * N, S.MIN_EXPECTED)) - 1, 1)
        for name, q in planted.items():
            if (q[~nz] > 0).any():
                continue                                  # an id of probability 0: the hard assertion
            lam = S.noncentrality(p, q, N)
            if label.startswith("n2v_") and lam < S.lambda_needed(df):
                continue                                  # judged per fault below
            if lam < S.lambda_needed(df):
                weak.append((label, name, round(lam), S.lambda_needed(df), N))
    assert not weak, weak


def _rejected(counts, p, N):
    try:
        return S.gof(counts, p, S.MIN_EXPECTED, N)[2] < S.LEVEL
    except AssertionError as e:
        assert "probability 0" in str(e)
        return True


def test_every_case_accepts_its_exact_distribution_and_rejects_every_planted_bias():
    rng = np.random.default_rng(20240607)
    n2v_hits = {}
    for label, p, N, planted in POWER:
        pv = S.gof(rng.multinomial(N, p), p, S.MIN_EXPECTED, N)[2]
        assert pv >= S.LEVEL, (label, pv)
        nz = p > 0
        df = max(len(S.merge_cells(p[nz] * N, S.MIN_EXPECTED)) - 1, 1)
        for name, q in planted.items():
            hit = _rejected(rng.multinomial(N, q), p, N)
            if label.startswith("n2v_"):
                sized = (q[~nz] > 0).any() or S.noncentrality(p, q, N) >= S.lambda_needed(df)
                key = (label.split("/")[0], name, label.split("/")[1][:5])
                n2v_hits[key] = n2v_hits.get(key, 0) + int(sized)
                if not sized:
                    continue
            assert hit, (label, name)
    # every node2vec fault is caught in step 1 and in step 2 of every (lists, p, q)
    for g in ("plain", "sorted"):
        for p_, q_ in S.N2V_PQ:
            for v in ("swapped", "undivided"):
                for step in ("step1", "step2"):
                    assert n2v_hits.get(("n2v_%s_p%g_q%g" % (g, p_, q_), v, step), 0) >= 1, (g, p_, q_, v, step)


# ------------------------------------------------------------------ 3. the oracle battery
R_ORACLE = 256                       # copies: the GPU file's 32 768 cut by 128
REPORT = S.Report()
_BACKENDS = {}


def _backend(O, name, R):
    import torch
    if (name, R) not in _BACKENDS:
        rep = S.replicas(name, R)
        rid, seg, nbr, w = rep.raw()
        csr = O.csr_from_raw(rid, seg, nbr, w, rep.T)
        _BACKENDS[(name, R)] = (rep, S.OracleBackend(torch, O.OracleGraph(csr)), csr)
    return _BACKENDS[(name, R)]


@pytest.mark.parametrize("graph", sorted(S.GRAPHS))
def test_restated_running_sums_are_the_oracles(O, graph):
    """The models read the motif's fp32 running sums as restated in numpy; they must be,
    bit for bit, what Node::Init (the oracle's eo_build_prefix) stores for every copy."""
    rep, _, csr = _backend(O, graph, 4)
    m, (rid, seg, nbr, w) = rep.motif, rep.raw()
    for x in range(rep.n):
        j = int(rep.pos_from_x(x))
        b, e = csr.row_ptr[x], csr.row_ptr[x + 1]
        mb, me = m.seg[j * m.T], m.seg[(j + 1) * m.T]
        assert np.array_equal(csr.prefix_w[b:e].view(np.uint32), m.prefix[mb:me].view(np.uint32))
        assert np.array_equal(csr.type_prefix[x * m.T:(x + 1) * m.T].view(np.uint32),
                              m.type_prefix[j * m.T:(j + 1) * m.T].view(np.uint32))
        assert np.array_equal(csr.type_end[x * m.T:(x + 1) * m.T], m.type_end[j * m.T:(j + 1) * m.T])
        # and the neighbours are the motif's targets inside the node's own copy
        tx = rep.x_from_id(csr.nbr[b:e].astype(np.int64))
        assert np.array_equal(rep.pos_from_x(tx), m.tgt[mb:me])
        assert (S._copy_of(rep, tx) == S._copy_of(rep, x)).all()


@pytest.mark.parametrize("case", S.NEIGHBOR_CASES, ids=[c["name"] for c in S.NEIGHBOR_CASES])
def test_oracle_neighbor_marginals(O, case):
    """R cut by 128 (N = 65 536 per row)."""
    import torch
    rep, B, _ = _backend(O, case["graph"], R_ORACLE)
    assert not S.run_neighbor_case(B, torch, "cpu", rep, case, S.SEED, REPORT)


def _node_backend(O):
    import torch
    rep, (rid, seg, nbr, w) = S.node_graph_raw()
    OG = O.OracleGraph(O.csr_from_raw(rid, seg, nbr, w, 1, S.NODE_TYPES, S.NODE_WEIGHTS))
    OG.build_node_sampler()
    return S.OracleBackend(torch, OG)


@pytest.mark.parametrize("case", S.NODE_CASES, ids=[c["name"] for c in S.NODE_CASES])
def test_oracle_sample_node(O, case):
    """count cut by 8."""
    import torch
    assert not S.run_node_case(_node_backend(O), torch, dict(case, count=case["count"] // 8), S.SEED, REPORT)


def test_oracle_sample_n_with_types(O):
    """rows cut by 16."""
    import torch
    assert not S.run_nwt_case(_node_backend(O), torch, "cpu", S.SEED, REPORT, rows=S.NWT_ROWS // 16)


def test_oracle_sample_root(O):
    """batch rows cut by 16."""
    import torch

    def sample_root(roots, w, m, call_id):
        out = O.sample_root(S.SEED, call_id, roots.numpy().astype(np.uint64), w.numpy(), 16, m, -1)
        return torch.from_numpy(out.astype(np.int64)).reshape(-1, m)
    assert not S.run_root_case(sample_root, torch, "cpu", S.SEED, REPORT, batch=S.ROOT_BATCH // 16)


@pytest.mark.parametrize("graph", sorted(S.LAYER_TYPES))
def test_oracle_sample_layer(O, graph):
    """R cut by 128, calls by 4."""
    import torch
    rep, B, _ = _backend(O, graph, R_ORACLE)

    def sample_layer(roots, et, call_id):
        return torch.from_numpy(B.OG.sample_layer(S.SEED, call_id, roots.numpy().astype(np.uint64), et, -1)[0]
                                .astype(np.int64))
    assert not S.run_layer_case(sample_layer, torch, "cpu", rep, graph, S.SEED, REPORT, calls=S.LAYER_CALLS // 4)


@pytest.mark.parametrize("weight_func", S.LOCAL_FUNCS)
def test_oracle_local_sample_layer(O, weight_func):
    """batch rows cut by 16."""
    import torch
    _, B, _ = _backend(O, "plain", 4)

    def local(idx, ids, w, t, batch, n, m, f, call_id):
        oid, ow, ot = B.OG.local_sample_layer(S.SEED, call_id, idx.numpy(), ids.numpy().astype(np.uint64),
                                              w.numpy(), t.numpy(), n, m, f, -1)
        return torch.from_numpy(oid.astype(np.int64)), None, torch.from_numpy(ot)
    assert not S.run_local_layer_case(local, torch, "cpu", weight_func, S.SEED, REPORT, batch=S.LOCAL_BATCH // 16)


@pytest.mark.parametrize("case", S.WALK_CASES, ids=[c["name"] for c in S.WALK_CASES])
def test_oracle_random_walk(O, case):
    """R cut by 128, calls by 8; walkers on one node at one step move together (asserted)."""
    import torch
    rep, B, _ = _backend(O, case["graph"], R_ORACLE)
    assert not S.run_walk_case(B, torch, "cpu", rep, case, S.SEED, REPORT, calls=case["calls"] // 8)


@pytest.mark.parametrize("lists", ["plain", "sorted"])
@pytest.mark.parametrize("pq", S.N2V_PQ)
def test_oracle_node2vec(O, pq, lists):
    """R cut by 16."""
    import torch
    rep, B, _ = _backend(O, lists, S.R_GPU // 16)
    assert not S.run_n2v_case(B, torch, "cpu", rep, pq[0], pq[1], S.SEED, REPORT, S.N2V_PER_NODE,
                              "n2v_%s_p%g_q%g" % (lists, pq[0], pq[1]))


def test_oracle_pairs_on_sample_neighbor(O):
    """Draws d | d + 1, call ids, seeds, node ids: the GPU file's size."""
    import torch
    rep, B, _ = _backend(O, "plain", S.R_GPU)
    bad = []
    for parity in (0, 1):
        bad += S.judge_pairs(REPORT, "pair_draws_%s" % ("even", "odd")[parity],
                             S.pairs_draws(B, torch, "cpu", rep, S.SEED, parity))
    for what in ("calls", "seeds"):
        bad += S.judge_pairs(REPORT, "pair_" + what, S.pairs_calls_or_seeds(B, torch, "cpu", rep, S.SEED, what))
    rep, B, _ = _backend(O, "rowmajor", S.R_GPU)
    bad += S.judge_pairs(REPORT, "pair_ids", S.pairs_ids(B, torch, "cpu", rep, S.SEED))
    assert not bad, bad


def test_oracle_pairs_on_fanout_walk_and_domains(O):
    """R cut by 16 (and the required number of pairs with it); domains at the GPU file's size."""
    import torch
    rep, B, _ = _backend(O, "plain", S.R_GPU // 16)
    bad = []
    for mode in ("hops", "auto", "multi"):
        bad += S.judge_pairs(REPORT, "pair_" + mode,
                             S.pairs_fanout(B, torch, "cpu", rep, S.SEED, mode, calls=1 if mode == "multi" else 6),
                             min_n=S.PAIR_MIN_N // 16)
    bad += S.judge_pairs(REPORT, "pair_walk", S.pairs_walk(B, torch, "cpu", rep, S.SEED), min_n=S.PAIR_MIN_N // 16)
    drep, (rid, seg, nbr, w) = S.domain_graph_raw()
    OG = O.OracleGraph(O.csr_from_raw(rid, seg, nbr, w, 1))
    OG.build_node_sampler()
    bad += S.judge_pairs(REPORT, "pair_domains", S.pairs_domains(S.OracleBackend(torch, OG), torch, "cpu", drep, S.SEED))
    assert not bad, bad


def test_oracle_hub_neighbor(O):
    """calls cut by 8."""
    import torch
    rep, B, _ = _backend(O, "hub", S.R_HUB)
    assert not S.run_hub_neighbor(B, torch, "cpu", rep, S.SEED, REPORT, calls=S.HUB_CALLS // 8)


@pytest.mark.parametrize("lists", ["hub", "hubsorted"])
@pytest.mark.parametrize("pq", S.N2V_PQ)
def test_oracle_hub_node2vec(O, pq, lists):
    """walkers per start node cut by 8."""
    import torch
    rep, B, _ = _backend(O, lists, S.R_HUB)
    assert not S.run_hub_n2v(B, torch, "cpu", rep, pq[0], pq[1], S.SEED, REPORT,
                             "n2v_%s_p%g_q%g" % (lists, pq[0], pq[1]), per_node=S.HUB_N2V_PER_NODE // 8)


# ------------------------------------------------------------------ 4. contract faults, planted in a backend
class _FaultyBackend(S.OracleBackend):
    """The oracle with one fault of the RNG contract planted in how an entry hands out call
    ids - the kind of fault oracle and kernels would share and parity cannot see."""

    def __init__(self, torch, OG, fault):
        super().__init__(torch, OG)
        self.fault = fault

    def _take(self, n, call_id):
        return super()._take(1 if self.fault == "counter_by_one" else n, call_id)

    def sample_fanout(self, nodes, edge_types, counts, default_node=-1, call_id=None):
        if self.fault != "hops_share_an_id":
            return super().sample_fanout(nodes, edge_types, counts, default_node, call_id)
        cid = self._take(len(counts), call_id)
        h1 = self.sample_neighbor(nodes, edge_types[0], counts[0], default_node, "tf", cid)[0].reshape(-1)
        h2 = self.sample_neighbor(h1, edge_types[1], counts[1], default_node, "tf", cid)[0].reshape(-1)
        return [nodes, h1, h2], None, None

    def sample_fanout_multi(self, batches, edge_types, counts, default_node=-1, call_id=None):
        if self.fault != "tiles_one_apart":
            return super().sample_fanout_multi(batches, edge_types, counts, default_node, call_id)
        cid = self._take(len(counts) * len(batches), call_id)
        return [self.sample_fanout(b, edge_types, counts, default_node, cid + i) for i, b in enumerate(batches)]


@pytest.mark.parametrize("fault,mode", [("hops_share_an_id", "hops"), ("counter_by_one", "auto"),
                                        ("tiles_one_apart", "multi")])
def test_planted_contract_faults_are_caught(O, fault, mode):
    """The substitution check, run: with hop 2 on hop 1's call id, the automatic counter
    advancing by one per call, or tiles one call id apart, the pair test named for it in the
    GPU file rejects (R cut by 16) - and it accepts the same backend without the fault
    (test_oracle_pairs_on_fanout_walk_and_domains)."""
    import torch
    rep, B, _ = _backend(O, "plain", S.R_GPU // 16)
    F = _FaultyBackend(torch, B.OG, fault)
    tables = S.pairs_fanout(F, torch, "cpu", rep, S.SEED, mode, calls=1 if mode == "multi" else 6)
    bad = S.judge_pairs(S.Report(), "planted_" + fault, tables, min_n=S.PAIR_MIN_N // 16)
    assert len(bad) == len(S.PAIR_ROWS), bad
