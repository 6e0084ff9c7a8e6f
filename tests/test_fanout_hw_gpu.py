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
