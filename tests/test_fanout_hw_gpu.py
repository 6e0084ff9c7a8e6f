"""Hop 2 of the plain-graph fanout step through the header + window side index (csrc/wb_hw.h,
tuning key 75): both kernels that run it - SampleFanoutPlainKernel for a caller on one stream,
SampleFanoutLeanKernel for one that alternates streams - give, bit for bit, what the
weight-bucket blocks give (key 75 = 0) and what the CPU oracle gives (oracle/step_check.py), on
partial tiles, hub rows, unknown roots and roots without edges; a graph whose side index is
declined is served as before."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, E, SEED = 20000, 260000, 5150
FANOUTS = ([25, 10], [3, 2], [5, 4])
EMPTY = (777, 12345)          # node ids whose rows are emptied


def t2n(t):
    return t.detach().cpu().numpy()


def _lib(EA):
    from euler_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def world(EA, O, torch_cuda):
    """The synthetic plain graph of euler_amd.synth_params (degree 1 .. > 4 000), and the same
    graph with two rows emptied (a root without edges), as device graphs + the host CSR."""
    p = EA.synth_params(SEED, N, E, weighted=True)
    po = O.SynthParams()
    for f, _ in po._fields_:
        setattr(po, f, getattr(p, f))
    csr = O.synth_csr(po)
    deg = np.diff(csr.row_ptr)
    assert (deg > 4000).sum() >= 1 and (deg > 64).sum() > 100 and deg.min() >= 1
    keep = np.ones(len(csr.nbr), bool)
    te = csr.type_end.copy()
    tp = csr.type_prefix.copy()
    for node in EMPTY:
        r = node - 1
        keep[csr.row_ptr[r]:csr.row_ptr[r + 1]] = False
        te[r] = 0
        tp[r] = 0
    d2 = deg.copy()
    d2[[n - 1 for n in EMPTY]] = 0
    rp2 = np.concatenate([[0], np.cumsum(d2)]).astype(np.int64)
    csr2 = O.CSR(csr.row_id, rp2, te, csr.nbr[keep], csr.prefix_w[keep], tp, 1)
    L = _lib(EA)
    L.euler_gpu_set_tuning(33, 0)            # the one-kernel step for every batch size
    G = EA.Graph.synthetic(p)
    G2 = EA.Graph.from_csr(csr2.row_id, csr2.row_ptr, csr2.type_end, csr2.nbr, csr2.prefix_w,
                           csr2.type_prefix, 1, csr2.node_type, csr2.node_weight)
    for g in (G, G2):
        g.set_seed(SEED)
    hubs = (np.argsort(-deg)[:40] + 1).astype(np.int64)      # the > 4 000 row first, then the > 1 000 ones
    yield {"G": G, "G2": G2, "csr": csr, "csr2": csr2, "hubs": hubs, "deg": deg}
    L.euler_gpu_set_tuning(33, 32768)
    L.euler_gpu_set_tuning(75, 1)


def _roots(world, n, rng):
    """hub rows first, then an unknown id, a root without edges, small rows and random ones"""
    special = [int(world["hubs"][0]), int(world["hubs"][1]), N + 5, EMPTY[0], 3, int(world["hubs"][7]), EMPTY[1]]
    r = special[:n] + [int(x) for x in rng.integers(1, N + 1, max(0, n - len(special)))]
    if n > 64:
        r[40:40 + 30] = [int(h) for h in world["hubs"][:30]]      # hubs share tiles with small rows
        r[-1] = N + 1
    return np.asarray(r[:n], np.int64)


def _run(EA, torch, G, roots, fanout, call_id, key, alternate):
    """(outputs as numpy, kernel name) of one step with key 75 = `key` on one stream or on the
    second of two alternating streams"""
    L = _lib(EA)
    assert L.euler_gpu_set_tuning(75, key) == 0
    dn = N + 1
    try:
        if not alternate:
            G.sample_fanout(roots[:1], [[0], [0]], fanout, dn, call_id=1)      # (this stream was the last one)
            out = G.sample_fanout(roots, [[0], [0]], fanout, dn, call_id=call_id)
        else:
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(s1):
                G.sample_fanout(roots[:1], [[0], [0]], fanout, dn, call_id=1)
            with torch.cuda.stream(s2):
                out = G.sample_fanout(roots, [[0], [0]], fanout, dn, call_id=call_id)
        name = (L.euler_gpu_last_fanout_kernel() or b"").decode()
        torch.cuda.synchronize()
    finally:
        L.euler_gpu_set_tuning(75, 1)
    return out, name


def _same(a, b):
    import torch
    for hop in range(2):
        if not (torch.equal(a[0][hop + 1], b[0][hop + 1]) and torch.equal(a[2][hop], b[2][hop])
                and torch.equal(a[1][hop].view(torch.int32), b[1][hop].view(torch.int32))):
            return False
    return True


def test_side_index_is_built_and_counted(EA, world):
    for g in (world["G"], world["G2"]):
        b0 = g.device_bytes
        nbytes, lines, ovf = g.side_index()
        deg = world["deg"] if g is world["G"] else None
        assert nbytes == lines * 128 and lines > 0 and ovf <= 0.002 * lines
        assert g.device_bytes >= b0 and g.device_bytes > nbytes
        if deg is not None:
            assert lines == int(np.where(deg <= 10, 1, (deg + 3) // 4).sum())
    L = _lib(EA)
    for bad in (2, -1, 7):
        assert L.euler_gpu_set_tuning(75, bad) != 0        # EINVAL, like the other keys
    assert L.euler_gpu_set_tuning(75, 1) == 0


@pytest.mark.parametrize("n", [1, 7, 1024])
@pytest.mark.parametrize("fanout", FANOUTS, ids=lambda f: "x".join(map(str, f)))
def test_hop2_side_index_equals_blocks_and_oracle(EA, O, torch_cuda, world, fanout, n):
    torch = torch_cuda
    from oracle.step_check import check_fanout_step
    rng = np.random.default_rng(100 * n + fanout[0])
    G = world["G2"]
    roots = torch.as_tensor(_roots(world, n, rng)).cuda()
    call_id = 40 + 2 * fanout[0]
    ref, name = _run(EA, torch, G, roots, fanout, call_id, 1, False)
    assert name == "SampleFanoutPlainKernel"
    edges, distinct = check_fanout_step(G, O.OracleGraph, O.CSR, SEED, call_id, roots, ref[0], ref[1], ref[2],
                                        fanout, N + 1, N)
    assert edges == n * fanout[0] * (1 + fanout[1])
    # ... and against the oracle over the whole host graph (default fill included)
    on, ow, ot = O.OracleGraph(world["csr2"]).sample_fanout(SEED, call_id, t2n(roots), [[0], [0]], fanout, N + 1)
    for hop in range(2):
        assert np.array_equal(t2n(ref[0][hop + 1]), np.asarray(on[hop]).reshape(-1))
        assert np.array_equal(t2n(ref[1][hop]).view(np.uint32),
                              np.asarray(ow[hop], np.float32).reshape(-1).view(np.uint32))
        assert np.array_equal(t2n(ref[2][hop]), np.asarray(ot[hop]).reshape(-1))
    for key, alternate, want in ((0, False, "SampleFanoutPlainKernel"), (1, True, "SampleFanoutLeanKernel"),
                                 (0, True, "SampleFanoutLeanKernel")):
        out, name = _run(EA, torch, G, roots, fanout, call_id, key, alternate)
        assert name == want, (key, alternate, name)
        assert _same(ref, out), (key, alternate)


def test_synthetic_graph_both_kernels(EA, O, torch_cuda, world):
    """the graph exactly as euler_amd.synth_params describes it (no emptied rows), 1 000 roots"""
    torch = torch_cuda
    from oracle.step_check import check_fanout_step
    G = world["G"]
    rng = np.random.default_rng(9)
    roots = torch.as_tensor(np.concatenate([world["hubs"][:20], rng.integers(1, N + 1, 979), [0]])).cuda()
    ref, name = _run(EA, torch, G, roots, [25, 10], 70, 1, False)
    assert name == "SampleFanoutPlainKernel"
    check_fanout_step(G, O.OracleGraph, O.CSR, SEED, 70, roots, ref[0], ref[1], ref[2], [25, 10], N + 1, N)
    for key, alternate in ((0, False), (1, True), (0, True)):
        out, _ = _run(EA, torch, G, roots, [25, 10], 70, key, alternate)
        assert _same(ref, out), (key, alternate)


def test_multi_with_per_minibatch_call_ids(EA, torch_cuda, world):
    torch = torch_cuda
    L = _lib(EA)
    G = world["G2"]
    rng = np.random.default_rng(21)
    batches = torch.as_tensor(np.stack([_roots(world, 64, rng) for _ in range(3)])).cuda()
    ids = torch.tensor([90, 50, 61], dtype=torch.int32, device="cuda")
    outs = {}
    try:
        for key in (1, 0):
            L.euler_gpu_set_tuning(75, key)
            G.sample_fanout(batches[0][:1], [[0], [0]], [5, 4], N + 1, call_id=1)
            outs[key] = G.sample_fanout_multi(batches, [[0], [0]], [5, 4], N + 1, call_ids=ids)
            assert (L.euler_gpu_last_fanout_kernel() or b"").decode() == "SampleFanoutPlainKernel"
    finally:
        L.euler_gpu_set_tuning(75, 1)
    for b in range(3):
        assert _same(outs[1][b], outs[0][b])
        one, _ = _run(EA, torch, G, batches[b], [5, 4], int(ids[b]), 1, False)
        assert _same(outs[1][b], one)


def test_declined_side_index_same_outputs(EA, torch_cuda, world):
    """index budget 0: neither index is built - no side index among the graph's bytes - and the
    step's outputs are what the graph with both indexes gives"""
    torch = torch_cuda
    L = _lib(EA)
    csr2 = world["csr2"]
    rng = np.random.default_rng(33)
    roots = torch.as_tensor(_roots(world, 1024, rng)).cuda()
    ref, _ = _run(EA, torch, world["G2"], roots, [25, 10], 80, 1, False)
    try:
        assert L.euler_gpu_set_index_budget(0, -1.0) == 0
        Gd = EA.Graph.from_csr(csr2.row_id, csr2.row_ptr, csr2.type_end, csr2.nbr, csr2.prefix_w,
                               csr2.type_prefix, 1, csr2.node_type, csr2.node_weight)
        Gd.set_seed(SEED)
        b0 = Gd.device_bytes
        assert Gd.side_index() == (0, 0, 0)
        out, name = _run(EA, torch, Gd, roots, [25, 10], 80, 1, False)
        assert _same(ref, out)
        assert Gd.side_index()[0] == 0
        nbytes = world["G2"].side_index()[0]
        assert Gd.device_bytes - b0 < nbytes          # (what it did build - the block search - is smaller)
        del Gd
    finally:
        L.euler_gpu_set_index_budget(-1, 0.5)
        L.euler_gpu_set_index_budget(2 ** 62, 0.5)


# ---- cold draws in both hops of both kernels ------------------------------------------------
# Draws the index does not settle replay the reference's bisection (fanout_local.h:
# ColdReplayPair).  On the synthetic graph that happens by accident of the data; this graph makes
# it certain.  A "bad" row has 44 edges - 40 of weight 1, then 4 of weight 100 - so 11 buckets of
# width 40: all forty unit edges fall into bucket 0, which overflows a block and a header line,
# and every draw that lands there (one in eleven) is cold on both paths.  The unit edges point at
# other bad rows, the heavy ones at ordinary rows (1 - 12 edges of weight in [0.5, 8)), and 200
# ordinary rows have an edge into a bad row, so hop 2 meets bad rows from ordinary roots as well.
# The 40 overflowing lines must stay within 2 in a thousand for the launcher to keep the graph on
# the index: 18 000 rows give about 25 000 lines, and no ordinary row may overflow its own.
CN, N_BAD, N_FEED = 18000, 40, 200
C_EMPTY = 9001                # a node without edges


@pytest.fixture(scope="module")
def cold_world(EA, O, torch_cuda):
    rng = np.random.default_rng(4401)
    ids = (1 + np.arange(CN)).astype(np.uint64)
    bad_rows = 100 + 400 * np.arange(N_BAD)
    is_bad = np.zeros(CN, bool)
    is_bad[bad_rows] = True
    deg = rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12], CN)     # (a row of exactly 10 edges overflows its 9-entry line)
    deg[bad_rows] = 44
    deg[C_EMPTY - 1] = 0
    seg = np.zeros(CN + 1, np.int64)
    seg[1:] = np.cumsum(deg)
    E = int(seg[-1])
    ordinary = ids[~is_bad]
    nbr = rng.choice(ordinary, E).astype(np.uint64)
    w = (rng.random(E) * 7.5 + 0.5).astype(np.float32)
    bad_ids = ids[bad_rows]
    for i, r in enumerate(bad_rows):
        lo = int(seg[r])
        nbr[lo:lo + 40] = bad_ids[(i + 1 + np.arange(40) % (N_BAD - 1)) % N_BAD]     # never itself
        w[lo:lo + 40] = 1.0
        w[lo + 40:lo + 44] = 100.0            # (their targets stay ordinary rows)
    cand = np.flatnonzero(~is_bad & (deg > 0))
    feed_rows = rng.choice(cand, N_FEED, replace=False)
    nbr[seg[feed_rows]] = bad_ids[np.arange(N_FEED) % N_BAD]
    csr = O.csr_from_raw(ids, seg, nbr, w, 1, np.zeros(CN, np.int32), np.ones(CN, np.float32))
    L = _lib(EA)
    L.euler_gpu_set_tuning(33, 0)            # the one-kernel step serves 1 024 roots
    G = EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w,
                          csr.type_prefix, 1, csr.node_type, csr.node_weight)
    G.set_seed(SEED)
    roots = np.concatenate([bad_ids.astype(np.int64), ids[feed_rows].astype(np.int64),
                            rng.integers(1, CN + 1, 1024 - N_BAD - N_FEED - 2), [N + 5, C_EMPTY]]).astype(np.int64)
    yield {"G": G, "OG": O.OracleGraph(csr), "roots": roots, "bad_ids": bad_ids.astype(np.int64)}
    L.euler_gpu_set_tuning(33, 32768)
    L.euler_gpu_set_tuning(75, 1)


def test_cold_graph_stays_on_the_index(cold_world):
    nbytes, lines, ovf = cold_world["G"].side_index()
    print("side index: %d lines, %d overflow" % (lines, ovf))
    assert 0 < ovf <= 0.002 * lines           # (else the launcher keeps the graph off the index)


@pytest.mark.parametrize("fanout", ([25, 10], [3, 2]), ids=lambda f: "x".join(map(str, f)))
def test_cold_draws_in_both_hops_of_both_kernels(EA, torch_cuda, cold_world, fanout):
    torch = torch_cuda
    G, roots_np, bad = cold_world["G"], cold_world["roots"], cold_world["bad_ids"]
    assert len(roots_np) == 1024
    call_id = 300 + fanout[0]
    on, ow, ot = cold_world["OG"].sample_fanout(SEED, call_id, roots_np, [[0], [0]], fanout, N + 1)
    on = [np.asarray(x).reshape(-1).astype(np.int64) for x in on]
    # the oracle's own draws: from a bad row, a unit-edge target (= a bad row) was drawn only
    # through bucket 0 - cold by construction; expected share 1 / 11
    src = roots_np
    for hop in range(2):
        from_bad = np.repeat(np.isin(src, bad), fanout[hop])
        cold = int((from_bad & np.isin(on[hop], bad)).sum())
        print("hop %d: %d cold draws of %d from bad rows" % (hop + 1, cold, int(from_bad.sum())))
        assert from_bad.sum() > 0 and cold >= 0.01 * from_bad.sum(), (hop, cold, int(from_bad.sum()))
        src = on[hop]
    roots = torch.as_tensor(roots_np).cuda()
    first = None
    for key, alternate, want in ((1, False, "SampleFanoutPlainKernel"), (0, False, "SampleFanoutPlainKernel"),
                                 (1, True, "SampleFanoutLeanKernel"), (0, True, "SampleFanoutLeanKernel")):
        out, name = _run(EA, torch, G, roots, fanout, call_id, key, alternate)
        assert name == want, (key, alternate, name)
        if first is None:
            first = out
            for hop in range(2):
                assert np.array_equal(t2n(out[0][hop + 1]).reshape(-1), on[hop]), (key, alternate, hop)
                assert np.array_equal(t2n(out[1][hop]).reshape(-1).view(np.uint32),
                                      np.asarray(ow[hop], np.float32).reshape(-1).view(np.uint32)), (key, alternate, hop)
                assert np.array_equal(t2n(out[2][hop]).reshape(-1), np.asarray(ot[hop]).reshape(-1)), (key, alternate, hop)
        else:
            assert _same(first, out), (key, alternate)
