"""Hop 2 of the plain-graph fanout step through the 12-bit side lines (csrc/wb_hw2.h: two index
requests per draw; tuning key 76 = 2 when the graph's index is built): both kernels that run it -
SampleFanoutPlainKernel for a caller on one stream, SampleFanoutLeanKernel for one that
alternates streams - give, bit for bit, what the weight-bucket blocks give (key 75 = 0) and what
the CPU oracle gives, on partial tiles, hub rows, unknown roots and roots without edges, through
sample_fanout, sample_fanout_multi and sample_fanout_unique; and on rows of heavy-tailed weights,
where the header's guess is often wrong and many draws go cold."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, E, SEED = 20000, 260000, 6260
FANOUTS = ([25, 10], [3, 2], [1, 2])
EMPTY = (777, 12345)          # node ids whose rows are emptied
DEFAULT_FORMAT = 2            # what key 76 is when nobody sets it (the measured choice)


def t2n(t):
    return t.detach().cpu().numpy()


def _lib(EA):
    from euler_amd import _lib
    return _lib.lib()


def _emptied(O, csr, nodes):
    deg = np.diff(csr.row_ptr)
    keep = np.ones(len(csr.nbr), bool)
    te, tp, d2 = csr.type_end.copy(), csr.type_prefix.copy(), deg.copy()
    for node in nodes:
        r = node - 1
        keep[csr.row_ptr[r]:csr.row_ptr[r + 1]] = False
        te[r] = 0
        tp[r] = 0
        d2[r] = 0
    rp2 = np.concatenate([[0], np.cumsum(d2)]).astype(np.int64)
    return O.CSR(csr.row_id, rp2, te, csr.nbr[keep], csr.prefix_w[keep], tp, 1)


def _graph(EA, csr):
    G = EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w,
                          csr.type_prefix, 1, csr.node_type, csr.node_weight)
    G.set_seed(SEED)
    return G


@pytest.fixture(scope="module")
def world(EA, O, torch_cuda):
    """The synthetic plain graph of euler_amd.synth_params (degree 1 .. > 4 000) with two rows
    emptied (isolated nodes), its side index built in the 12-bit format."""
    p = EA.synth_params(SEED, N, E, weighted=True)
    po = O.SynthParams()
    for f, _ in po._fields_:
        setattr(po, f, getattr(p, f))
    csr = O.synth_csr(po)
    deg = np.diff(csr.row_ptr)
    assert (deg > 1600).sum() >= 1 and (deg > 64).sum() > 100
    csr2 = _emptied(O, csr, EMPTY)
    L = _lib(EA)
    L.euler_gpu_set_tuning(33, 0)            # the one-kernel step for every batch size
    assert L.euler_gpu_set_tuning(76, 2) == 0
    G = _graph(EA, csr2)
    assert G.side_index_format() == 2        # (built here, while key 76 says so)
    hubs = (np.argsort(-deg)[:40] + 1).astype(np.int64)
    yield {"G": G, "OG": O.OracleGraph(csr2), "hubs": hubs, "deg": deg, "csr2": csr2}
    L.euler_gpu_set_tuning(33, 32768)
    L.euler_gpu_set_tuning(75, 1)
    L.euler_gpu_set_tuning(76, DEFAULT_FORMAT)


def _roots(world, n, rng):
    """hub rows first, then an unknown id, a root without edges, small rows and random ones"""
    special = [int(world["hubs"][0]), int(world["hubs"][1]), N + 5, EMPTY[0], 3, int(world["hubs"][7]), EMPTY[1]]
    r = special[:n] + [int(x) for x in rng.integers(1, N + 1, max(0, n - len(special)))]
    if n > 64:
        r[40:40 + 30] = [int(h) for h in world["hubs"][:30]]      # hubs share tiles with small rows
        r[-1] = N + 1
    return np.asarray(r[:n], np.int64)


def _run(EA, torch, G, roots, fanout, call_id, key, alternate, dn=N + 1):
    """(outputs, kernel name) of one step with key 75 = `key` on one stream or on the second of
    two alternating streams"""
    L = _lib(EA)
    assert L.euler_gpu_set_tuning(75, key) == 0
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


def _equals_oracle(out, on, ow, ot):
    for hop in range(2):
        assert np.array_equal(t2n(out[0][hop + 1]).reshape(-1), np.asarray(on[hop]).reshape(-1).astype(np.int64)), hop
        assert np.array_equal(t2n(out[1][hop]).reshape(-1).view(np.uint32),
                              np.asarray(ow[hop], np.float32).reshape(-1).view(np.uint32)), hop
        assert np.array_equal(t2n(out[2][hop]).reshape(-1), np.asarray(ot[hop]).reshape(-1)), hop


def test_format_key_and_same_size(EA, O, world):
    """key 76 takes 1 and 2 only; the 12-bit index has the lines, bytes and overflow count of the
    8-bit one over the same graph (same buckets, same nine entries): the side index does not grow"""
    L = _lib(EA)
    for bad in (0, 3, -1):
        assert L.euler_gpu_set_tuning(76, bad) != 0
    nbytes, lines, ovf = world["G"].side_index()
    assert nbytes == lines * 128 and lines > 0 and ovf <= 0.002 * lines
    try:
        assert L.euler_gpu_set_tuning(76, 1) == 0
        G1 = _graph(EA, world["csr2"])
        assert G1.side_index_format() == 1
        assert G1.side_index() == (nbytes, lines, ovf)
        assert G1.device_bytes == world["G"].device_bytes
    finally:
        L.euler_gpu_set_tuning(76, 2)
    assert world["G"].side_index_format() == 2          # a graph keeps the format it was built in


def test_default_format_and_the_8_bit_lines_beside_it(EA, torch_cuda, world):
    """a graph built while nobody has set key 76 gets the default format; one built with key 76 = 1
    draws through the lines of wb_hw.h - both kernels, same outputs as the 12-bit graph"""
    torch = torch_cuda
    L = _lib(EA)
    rng = np.random.default_rng(31)
    roots = torch.as_tensor(_roots(world, 1029, rng)).cuda()
    ref, _ = _run(EA, torch, world["G"], roots, [25, 10], 88, 1, False)
    try:
        assert L.euler_gpu_set_tuning(76, DEFAULT_FORMAT) == 0
        assert _graph(EA, world["csr2"]).side_index_format() == DEFAULT_FORMAT
        assert L.euler_gpu_set_tuning(76, 1) == 0
        G1 = _graph(EA, world["csr2"])
        assert G1.side_index_format() == 1
    finally:
        L.euler_gpu_set_tuning(76, 2)
    for alternate, want in ((False, "SampleFanoutPlainKernel"), (True, "SampleFanoutLeanKernel")):
        out, name = _run(EA, torch, G1, roots, [25, 10], 88, 1, alternate)
        assert name == want and _same(ref, out), (alternate, name)


@pytest.mark.parametrize("n", [1, 7, 4096])
@pytest.mark.parametrize("fanout", FANOUTS, ids=lambda f: "x".join(map(str, f)))
def test_hop2_two_requests_equals_blocks_and_oracle(EA, torch_cuda, world, fanout, n):
    torch = torch_cuda
    rng = np.random.default_rng(100 * n + fanout[0])
    G = world["G"]
    roots_np = _roots(world, n, rng)
    roots = torch.as_tensor(roots_np).cuda()
    call_id = 40 + 2 * fanout[0]
    ref, name = _run(EA, torch, G, roots, fanout, call_id, 1, False)
    assert name == "SampleFanoutPlainKernel"
    on, ow, ot = world["OG"].sample_fanout(SEED, call_id, roots_np, [[0], [0]], fanout, N + 1)
    _equals_oracle(ref, on, ow, ot)
    for key, alternate, want in ((0, False, "SampleFanoutPlainKernel"), (1, True, "SampleFanoutLeanKernel"),
                                 (0, True, "SampleFanoutLeanKernel")):
        out, name = _run(EA, torch, G, roots, fanout, call_id, key, alternate)
        assert name == want, (key, alternate, name)
        assert _same(ref, out), (key, alternate)


def test_default_node_fill(EA, torch_cuda, world):
    """rows without samples (unknown root, isolated node, children of a filled row) carry the
    caller's default node, whatever it is"""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    roots_np = _roots(world, 7, rng)
    roots = torch.as_tensor(roots_np).cuda()
    for dn in (-1, 424242):
        ref, _ = _run(EA, torch, world["G"], roots, [3, 2], 77, 1, False, dn=dn)
        on, ow, ot = world["OG"].sample_fanout(SEED, 77, roots_np, [[0], [0]], [3, 2], dn)
        _equals_oracle(ref, on, ow, ot)
        assert (t2n(ref[0][1]).reshape(7, 3)[2] == dn).all()          # the unknown root's row
        out, _ = _run(EA, torch, world["G"], roots, [3, 2], 77, 0, False, dn=dn)
        assert _same(ref, out)


def test_multi(EA, torch_cuda, world):
    torch = torch_cuda
    L = _lib(EA)
    G = world["G"]
    rng = np.random.default_rng(21)
    batches_np = np.stack([_roots(world, 64, rng) for _ in range(3)])
    batches = torch.as_tensor(batches_np).cuda()
    ids = torch.tensor([90, 50, 61], dtype=torch.int32, device="cuda")
    outs = {}
    try:
        for key in (1, 0):
            L.euler_gpu_set_tuning(75, key)
            G.sample_fanout(batches[0][:1], [[0], [0]], [25, 10], N + 1, call_id=1)
            outs[key] = G.sample_fanout_multi(batches, [[0], [0]], [25, 10], N + 1, call_ids=ids)
            assert (L.euler_gpu_last_fanout_kernel() or b"").decode() == "SampleFanoutPlainKernel"
    finally:
        L.euler_gpu_set_tuning(75, 1)
    for b in range(3):
        assert _same(outs[1][b], outs[0][b])
        on, ow, ot = world["OG"].sample_fanout(SEED, int(ids[b]), batches_np[b], [[0], [0]], [25, 10], N + 1)
        _equals_oracle(outs[1][b], on, ow, ot)


def test_unique(EA, torch_cuda, world):
    """the (unique rows, index) form: rows[row_index] is the step's hop 2"""
    torch = torch_cuda
    L = _lib(EA)
    G = world["G"]
    rng = np.random.default_rng(22)
    roots_np = _roots(world, 263, rng)
    roots = torch.as_tensor(roots_np).cuda()
    on, ow, ot = world["OG"].sample_fanout(SEED, 130, roots_np, [[0], [0]], [25, 10], N + 1)
    try:
        for key in (1, 0):
            L.euler_gpu_set_tuning(75, key)
            G.sample_fanout(roots[:1], [[0], [0]], [25, 10], N + 1, call_id=1)
            id1, w1, t1, idx, rid, rw, rt = G.sample_fanout_unique(roots, [[0], [0]], [25, 10], N + 1, call_id=130)
            out = ([None, id1.reshape(-1), rid[idx].reshape(-1)], [w1.reshape(-1), rw[idx].reshape(-1)],
                   [t1.reshape(-1), rt[idx].reshape(-1)])
            _equals_oracle(out, on, ow, ot)
    finally:
        L.euler_gpu_set_tuning(75, 1)


# ---- heavy-tailed rows: wrong guesses and cold draws ------------------------------------------
# A whole graph of Pareto(0.7) weights (tests/test_gpu_parity.py: the family of tuning key 51's
# test) overflows 5 lines in a hundred and gets no side index at all.  Here 12 rows of 60 edges
# carry such weights - dust among giants: the dust's sums share a 12-bit code, so the guess is too
# high by one (second window) or by more (cold), and lines overflow - inside a graph of ordinary
# rows that keeps the overflowing lines under 2 in a thousand.  Their edges point at each other and
# at ordinary rows, and 400 ordinary rows have an edge into one of them.
HN, H_BAD, H_FEED, H_DEG = 18000, 12, 400, 60


@pytest.fixture(scope="module")
def heavy_world(EA, O, torch_cuda):
    rng = np.random.default_rng(7701)
    ids = (1 + np.arange(HN)).astype(np.uint64)
    bad_rows = 100 + 400 * np.arange(H_BAD)
    is_bad = np.zeros(HN, bool)
    is_bad[bad_rows] = True
    deg = rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12], HN)
    deg[bad_rows] = H_DEG
    seg = np.zeros(HN + 1, np.int64)
    seg[1:] = np.cumsum(deg)
    ne = int(seg[-1])
    nbr = rng.choice(ids[~is_bad], ne).astype(np.uint64)
    w = (rng.random(ne) * 7.5 + 0.5).astype(np.float32)
    bad_ids = ids[bad_rows]
    for i, r in enumerate(bad_rows):
        lo = int(seg[r])
        w[lo:lo + H_DEG] = (rng.pareto(0.7, H_DEG) + 1e-3).astype(np.float32)
        nbr[lo:lo + H_DEG:2] = bad_ids[(i + 1 + np.arange(H_DEG // 2)) % H_BAD]
    feed_rows = rng.choice(np.flatnonzero(~is_bad), H_FEED, replace=False)
    nbr[seg[feed_rows]] = bad_ids[np.arange(H_FEED) % H_BAD]
    csr = O.csr_from_raw(ids, seg, nbr, w, 1, np.zeros(HN, np.int32), np.ones(HN, np.float32))
    L = _lib(EA)
    L.euler_gpu_set_tuning(33, 0)
    L.euler_gpu_set_tuning(76, 2)
    G = _graph(EA, csr)
    roots = np.concatenate([bad_ids.astype(np.int64), ids[feed_rows].astype(np.int64),
                            rng.integers(1, HN + 1, 1024 - H_BAD - H_FEED - 1), [HN + 5]]).astype(np.int64)
    yield {"G": G, "OG": O.OracleGraph(csr), "roots": roots, "bad_ids": bad_ids.astype(np.int64)}
    L.euler_gpu_set_tuning(33, 32768)
    L.euler_gpu_set_tuning(75, 1)
    L.euler_gpu_set_tuning(76, DEFAULT_FORMAT)


@pytest.mark.parametrize("fanout", ([25, 10], [3, 2]), ids=lambda f: "x".join(map(str, f)))
def test_heavy_tailed_rows(EA, torch_cuda, heavy_world, fanout):
    torch = torch_cuda
    G, roots_np, bad = heavy_world["G"], heavy_world["roots"], heavy_world["bad_ids"]
    nbytes, lines, ovf = G.side_index()
    assert G.side_index_format() == 2 and 0 < ovf <= 0.002 * lines, (lines, ovf)
    call_id = 500 + fanout[0]
    on, ow, ot = heavy_world["OG"].sample_fanout(SEED, call_id, roots_np, [[0], [0]], fanout, HN + 1)
    hop1 = np.asarray(on[0]).reshape(-1).astype(np.int64)
    assert np.isin(hop1, bad).sum() >= 100          # hop 2 draws from heavy-tailed rows
    roots = torch.as_tensor(roots_np).cuda()
    first = None
    for key, alternate, want in ((1, False, "SampleFanoutPlainKernel"), (0, False, "SampleFanoutPlainKernel"),
                                 (1, True, "SampleFanoutLeanKernel"), (0, True, "SampleFanoutLeanKernel")):
        out, name = _run(EA, torch, G, roots, fanout, call_id, key, alternate, dn=HN + 1)
        assert name == want, (key, alternate, name)
        if first is None:
            first = out
            _equals_oracle(out, on, ow, ot)
        else:
            assert _same(first, out), (key, alternate)
