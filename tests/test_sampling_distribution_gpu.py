"""Output distributions of every sampling entry, from the HIP kernels, against exact
probabilities (tests/sampling_stats.py has the models, the statistics and the case table).

The parity tests pin the kernels bit for bit to the CPU oracle, which proves they run the
oracle's algorithm on the oracle's random stream.  These tests prove what parity cannot:
that ids come out with the probabilities the reference defines, and that draws meant to be
independent are independent - a fault in the RNG contract of DESIGN section 3 (two hops on
one call id, the two draws of a Philox block sharing words, streams of neighbouring ids
overlapping, a tile's call id meeting the next hop's, a `u` that reaches the end of a row)
is reproduced by oracle and kernels alike and leaves every parity test green.

Every statistic is accepted iff its p-value >= 1e-7 (derived, sampling_stats.LEVEL).  Seeds
and call ids are fixed in the case table; to look into a failure rerun the case with
SAMPLING_STATS_SEED=<one of sampling_stats.RECHECK_SEEDS> - a 1e-7 fluke does not repeat, a
real bias fails all of them.  tests/test_sampling_stats_host.py shows with the same `p`, `N`
and statistic that each case rejects its planted bias, and runs the battery on the oracle;
the GPU is bit-identical to the oracle, so a case run there at the same size prints the
same statistic (not asserted).

Which test fails if ...
  sample_neighbor returned a row's first entry 5 % too often   test_neighbor_marginals
      (every graph / layout / count parity), and the same bias in any other entry fails
      that entry's marginal test below
  hop 2 reused hop 1's call id                                  test_pairs_fanout[hops]
  the auto counter advanced by one per call                     test_pairs_fanout[auto]
  a tile's call ids were one apart in sample_fanout_multi       test_pairs_fanout[multi]
  the two draws of a Philox block shared words                  test_pairs_draws[even]
  neighbouring draw indices / call ids / seeds / node ids overlapped
      test_pairs_draws[odd], test_pairs_calls_seeds, test_pairs_node_ids
  walk steps shared a call id                                   test_pairs_walk_steps
  domains 0 and 1 shared a key                                  test_pairs_domains

Which fanout kernel each graph reaches (sample_kernels.hip, the 2-hop dispatch; the kernel
is asserted through euler_gpu_last_fanout_kernel, the build inside it is read from the code):
  mild        T = 1, identity ids, weighted, every row fits its buckets of the weight-bucket
              index                               SampleFanoutPlainKernel (fanout_plain.h)
  side        the same with rows of at most nine entries per bucket, so that the header +
              window side index exists (asserted): SampleFanoutPlainKernel, hop 2 through
              wb_hw2.h - the build the benchmark's step runs
  plain       the same with the full geometric row, which overflows a bucket (wb_lean_ok = 0:
              the lean kernels keep the pivot levels)   SampleFanoutLeanKernel, WB = 0
  hashedmild  irregular ids (hash lookup)         SampleFanoutLeanKernel, WB = 2 (lean_g)
  hashed      irregular ids, index declined       SampleFanoutLocalKernel (the general path)
  typed       T = 3, one listed type per hop      SampleFanoutLeanKernel, WB = 2 (lean_g)
  typed       T = 3, two listed types per hop     WB = 4 (row record in registers); with
                                                  tuning key 48 = 0: WB = 3
  uniform     T = 1, every weight 1               SampleFanoutLeanKernel, UNIFORM
  utyped      T = 3 uniform, one listed type      WB = 6 (lean_gu); two listed types WB = 5
"""
import os

import numpy as np
import pytest

import sampling_stats as S

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("SAMPLING_STATS_SEED", S.SEED))
REPORT = S.Report()
_GRAPHS = {}


def _graph(EA, O, name, R=S.R_GPU):
    """(Replicas, euler_amd.Graph) of a motif graph, built once per run."""
    if (name, R) not in _GRAPHS:
        rep = S.replicas(name, R)
        rid, seg, nbr, w = rep.raw()
        csr = O.csr_from_raw(rid, seg, nbr, w, rep.T)
        G = EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w, csr.type_prefix,
                              csr.n_types, csr.node_type, csr.node_weight)
        assert G.id_range()[1] == (not rep.jitter), "the id map this graph was built to reach"
        _GRAPHS[(name, R)] = (rep, G)
    return _GRAPHS[(name, R)]


@pytest.mark.parametrize("case", S.NEIGHBOR_CASES, ids=[c["name"] for c in S.NEIGHBOR_CASES])
def test_neighbor_marginals(EA, O, torch_cuda, case):
    """sample_neighbor (one / several / no listed types, both layouts, even and odd counts -
    the default build samples pairs per lane for even counts), sample_neighbor_sets,
    sample_fanout [8, 8] on both hops and sample_fanout_multi with 8 tiles: gof per motif
    row against the running-sum model, then pooled.  Rows without neighbours must be the
    default fill, exactly; ids of weight 0 must never appear; every draw is counted."""
    from euler_amd import _lib
    rep, G = _graph(EA, O, case["graph"])
    key = case.get("tuning")
    if key:
        _lib.check(_lib.lib().euler_gpu_set_tuning(key[0], key[1]))
    try:
        bad = S.run_neighbor_case(G, torch_cuda, "cuda", rep, case, SEED, REPORT)
        if "kernel" in case:
            assert _lib.lib().euler_gpu_last_fanout_kernel().decode() == case["kernel"]
        if "side" in case:
            assert G.side_index()[0] > 0 and G.side_index_format() == case["side"]
    finally:
        if key:
            _lib.lib().euler_gpu_set_tuning(key[0], key[2])
    assert not bad, bad


@pytest.fixture(scope="module")
def node_graph(EA, O, torch_cuda):
    rep, (rid, seg, nbr, w) = S.node_graph_raw()
    csr = O.csr_from_raw(rid, seg, nbr, w, 1, S.NODE_TYPES, S.NODE_WEIGHTS)
    return EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w, csr.type_prefix,
                             csr.n_types, csr.node_type, csr.node_weight)


@pytest.mark.parametrize("case", S.NODE_CASES, ids=[c["name"] for c in S.NODE_CASES])
def test_sample_node(node_graph, torch_cuda, case):
    """sample_node: one type, type -1 (the type by its weight sum first) and a list of types."""
    assert not S.run_node_case(node_graph, torch_cuda, case, SEED, REPORT)


def test_sample_n_with_types(node_graph, torch_cuda):
    assert not S.run_nwt_case(node_graph, torch_cuda, "cuda", SEED, REPORT)


@pytest.mark.parametrize("edge_type", [0, 2, -1])
def test_sample_edge(EA, O, torch_cuda, edge_type):
    """sample_edge over the records of the typed motif (zero-weight records included: never
    drawn): w / sum(w) within the type, -1 draws the type by its weight sum first."""
    torch = torch_cuda
    _, G = _graph(EA, O, "typed", 1)
    src, dst, ty, w = S.typed_edge_records()
    G.set_edges(src, dst, ty, w)
    G.set_edge_sampler()
    G.set_seed(SEED)
    out = G.sample_edge(S.EDGE_COUNT, edge_type, call_id=S.EDGE_CALL + edge_type + 1)
    lut = np.full(17 * 17 * 3, len(src), np.int64)
    lut[(src.astype(np.int64) * 17 + dst.astype(np.int64)) * 3 + ty] = np.arange(len(src))
    rec = torch.as_tensor(lut, device="cuda")[(out[:, 0] * 17 + out[:, 1]) * 3 + out[:, 2]]
    assert int(rec.max()) < len(src), "a triple that is no record was drawn"
    counts = torch.bincount(rec, minlength=len(src)).cpu().numpy()
    assert not S._judge_flat(REPORT, "sample_edge/type%d" % edge_type, counts, S.edge_model(ty, w, edge_type),
                             S.EDGE_COUNT)


def test_sample_graph_label(EA, O, torch_cuda):
    """sample_graph_label: uniform over the L = 37 labels."""
    torch = torch_cuda
    rep, G = _graph(EA, O, "plain", 3)
    G.set_graph_labels(np.arange(1, S.LABELS + 1), ["g%02d" % i for i in range(S.LABELS)])
    G.set_seed(SEED)
    out = G.sample_graph_label(S.LABEL_COUNT, call_id=S.LABEL_CALL)
    assert int(out.min()) >= 0 and int(out.max()) < S.LABELS
    counts = torch.bincount(out, minlength=S.LABELS).cpu().numpy()
    assert not S._judge_flat(REPORT, "sample_graph_label", counts, np.full(S.LABELS, 1.0 / S.LABELS), S.LABEL_COUNT)


def test_sample_root(EA, O, torch_cuda):
    _, G = _graph(EA, O, "plain", 3)
    G.set_seed(SEED)
    assert not S.run_root_case(lambda r, w, m, c: G.sample_root(r, w, m, -1, call_id=c), torch_cuda, "cuda",
                               SEED, REPORT)


@pytest.mark.parametrize("graph", ["plain", "typed"])
def test_sample_layer(EA, O, torch_cuda, graph):
    rep, G = _graph(EA, O, graph)
    G.set_seed(SEED)
    assert not S.run_layer_case(lambda r, et, c: G.sample_layer(r, et, -1, call_id=c)[0], torch_cuda, "cuda",
                                rep, graph, SEED, REPORT)


@pytest.mark.parametrize("weight_func", S.LOCAL_FUNCS)
def test_local_sample_layer(EA, O, torch_cuda, weight_func):
    _, G = _graph(EA, O, "plain", 3)
    G.set_seed(SEED)
    assert not S.run_local_layer_case(
        lambda idx, ids, w, t, b, n, m, f, c: G.local_sample_layer(idx, ids, w, t, b, n, m, f, -1, call_id=c),
        torch_cuda, "cuda", weight_func, SEED, REPORT)


@pytest.mark.parametrize("case", S.WALK_CASES, ids=[c["name"] for c in S.WALK_CASES])
def test_random_walk(EA, O, torch_cuda, case):
    """random_walk with p = q = 1.  The unit of independence: a step is a count-1 neighbour
    draw keyed by the CURRENT NODE and call_id + step (walk_kernels.hip: CwDraw / the
    per-walker kernel), so walkers standing on the same node at the same
    step take the same move.  That is asserted, and one transition is counted per distinct
    (call, step, node).  'merged' cases start 524 288 walkers (>= 262 144: the Cw* kernels
    that walk groups of merged walkers), 'per_walker' 131 072 (one lane per walker)."""
    rep, G = _graph(EA, O, case["graph"])
    assert (rep.n >= 262144) and (case["walkers"] != "quarter" or rep.n // 4 < 262144)
    assert not S.run_walk_case(G, torch_cuda, "cuda", rep, case, SEED, REPORT)


@pytest.mark.parametrize("key7,key25", [(0, 8192), (1, 8192), (2, 8192), (3, 8192), (3, 2)])
@pytest.mark.parametrize("lists", ["stored", "ascending"])
@pytest.mark.parametrize("pq", S.N2V_PQ)
def test_node2vec(EA, O, torch_cuda, pq, lists, key7, key25):
    """node2vec steps against RWCallback::BuildWeights restated, on lists in storage order
    (the reference's quirk) and in ascending order (true node2vec), through every launch
    mode of tuning key 7 and, with key 25 = 2, the workgroup kernel for every row of two or
    more entries.  Step 1 (empty parent list) and step 2 are separate statistics."""
    from euler_amd import _lib
    rep, G = _graph(EA, O, "plain" if lists == "stored" else "sorted")
    L = _lib.lib()
    _lib.check(L.euler_gpu_set_tuning(7, key7))
    _lib.check(L.euler_gpu_set_tuning(25, key25))
    try:
        bad = S.run_n2v_case(G, torch_cuda, "cuda", rep, pq[0], pq[1], SEED, REPORT, S.N2V_PER_NODE,
                             "n2v_%s_p%g_q%g_k%d_%d" % (lists, pq[0], pq[1], key7, key25))
    finally:
        L.euler_gpu_set_tuning(7, 2)
        L.euler_gpu_set_tuning(25, 8192)
    assert not bad, bad


@pytest.mark.parametrize("parity", ["even", "odd"])
def test_pairs_draws(EA, O, torch_cuda, parity):
    """Draws d and d + 1 of one root: even d (the two halves of one Philox block) and odd d."""
    rep, G = _graph(EA, O, "plain")
    t = S.pairs_draws(G, torch_cuda, "cuda", rep, SEED, 0 if parity == "even" else 1)
    assert not S.judge_pairs(REPORT, "pair_draws_" + parity, t)


@pytest.mark.parametrize("what", ["calls", "seeds"])
def test_pairs_calls_seeds(EA, O, torch_cuda, what):
    """The same root and draw under call ids c, c + 1 and under seeds s, s + 1."""
    rep, G = _graph(EA, O, "plain")
    assert not S.judge_pairs(REPORT, "pair_" + what, S.pairs_calls_or_seeds(G, torch_cuda, "cuda", rep, SEED, what))


def test_pairs_node_ids(EA, O, torch_cuda):
    """Node ids x and x + 1 (one motif row at consecutive ids), same call and draw."""
    rep, G = _graph(EA, O, "rowmajor")
    assert not S.judge_pairs(REPORT, "pair_ids", S.pairs_ids(G, torch_cuda, "cuda", rep, SEED))


@pytest.mark.parametrize("mode", ["hops", "auto", "multi"])
def test_pairs_fanout(EA, O, torch_cuda, mode):
    """hops: a node's hop-1 row as a root against its hop-2 row as a child of one
    sample_fanout; auto: hop 2 of a call against hop 1 of the next under call_id=None;
    multi: tile b hop 2 against tile b + 1 hop 1 of sample_fanout_multi."""
    rep, G = _graph(EA, O, "plain")
    t = S.pairs_fanout(G, torch_cuda, "cuda", rep, SEED, mode, calls=1 if mode == "multi" else 6)
    assert not S.judge_pairs(REPORT, "pair_" + mode, t)


def test_pairs_walk_steps(EA, O, torch_cuda):
    """The move from node x at step s against the move from x at step s + 1."""
    rep, G = _graph(EA, O, "plain")
    assert not S.judge_pairs(REPORT, "pair_walk", S.pairs_walk(G, torch_cuda, "cuda", rep, SEED))


def test_pairs_domains(EA, O, torch_cuda):
    """sample_n_with_types (domain 1, stream = row index i, draws 2 j and 2 j + 1 for sample
    j) against sample_neighbor of the node whose id is i (domain 0, stream = node id, draw
    2 j) under the same seed and call id: the column draw of the alias method and the
    neighbour draw would read the same uniform if the domain salt were dropped.  (sample_node
    itself draws on stream 0, the one id no node can have; sample_n_with_types is the same
    draw on a stream that a node id can equal.)"""
    assert not S.judge_pairs(REPORT, "pair_domains", S.pairs_domains(*_domain_backends(EA, O, torch_cuda), SEED))


def _domain_backends(EA, O, torch):
    rep, (rid, seg, nbr, w) = S.domain_graph_raw()
    csr = O.csr_from_raw(rid, seg, nbr, w, 1)
    G = EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w, csr.type_prefix,
                          csr.n_types, csr.node_type, csr.node_weight)
    return G, torch, "cuda", rep


def test_hub_neighbor(EA, O, torch_cuda):
    """sample_neighbor on the hub motif (64 copies): a row of 6 000 heavy-tailed entries -
    the weight-bucket index's second-chance path and pivot levels deeper than one block - in
    32 bins of equal expected mass, and the two rows of 600 entries by neighbour id."""
    rep, G = _graph(EA, O, "hub", S.R_HUB)
    assert not S.run_hub_neighbor(G, torch_cuda, "cuda", rep, SEED, REPORT)


@pytest.mark.parametrize("lists", ["hub", "hubsorted"])
@pytest.mark.parametrize("pq", S.N2V_PQ)
def test_hub_node2vec(EA, O, torch_cuda, pq, lists):
    """node2vec where child and parent lists have 600 and 6 000 entries (several 256-entry
    chunks), stepwise launches (key 7 = 3) with key 25 = 256, so that these rows go to the
    workgroup kernel; lists in storage order and ascending."""
    from euler_amd import _lib
    rep, G = _graph(EA, O, lists, S.R_HUB)
    L = _lib.lib()
    _lib.check(L.euler_gpu_set_tuning(7, 3))
    _lib.check(L.euler_gpu_set_tuning(25, 256))
    try:
        bad = S.run_hub_n2v(G, torch_cuda, "cuda", rep, pq[0], pq[1], SEED, REPORT,
                            "n2v_%s_p%g_q%g" % (lists, pq[0], pq[1]))
    finally:
        L.euler_gpu_set_tuning(7, 2)
        L.euler_gpu_set_tuning(25, 8192)
    assert not bad, bad
