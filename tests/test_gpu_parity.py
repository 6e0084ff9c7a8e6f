"""Parity of the HIP path (through the C ABI) against the CPU oracle and the
committed golden vectors.  Bit-exact for ids / types / weights / indices;
scatter results are bit-exact too (order-faithful segment reduce), which is
stronger than the 1e-5 fp32 tolerance north_star allows.  Needs an MI355X."""
import os

import numpy as np
import pytest

from conftest import make_random_graph
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SEED = 20240521


@pytest.fixture(params=["blockpivot", "blockpivot1", "pivot", "dedup", "typedloop", "generic"])
def k1_variant(request, EA):
    """The sample_neighbor kernels a call can be served by - block pivots (the default:
    pairs of samples per lane for even counts, the one-kernel fanout, type draws on the
    pivots), the same with one sample per lane, pivot levels over the flat arrays, the
    duplicate-root machinery forced for every batch size, type draws by the reference
    loop, and the reference loop for everything: all must match the oracle bit for bit."""
    from euler_amd import _lib
    L = _lib.lib()
    v = request.param
    L.euler_gpu_set_tuning(0, 0 if v == "generic" else 5 if v == "pivot" else 6)
    L.euler_gpu_set_tuning(4, 0 if v == "blockpivot1" else 1)     # pairs per lane
    L.euler_gpu_set_tuning(5, 2 if v == "dedup" else 1)           # duplicate path always
    L.euler_gpu_set_tuning(27, 0 if v in ("dedup", "blockpivot1") else 1)   # one-kernel fanout
    L.euler_gpu_set_tuning(37, 0 if v == "typedloop" else 1)
    yield v
    L.euler_gpu_set_tuning(0, 6)
    L.euler_gpu_set_tuning(4, 1)
    L.euler_gpu_set_tuning(5, 1)
    L.euler_gpu_set_tuning(27, 1)
    L.euler_gpu_set_tuning(37, 1)


def gpu_graph(EA, csr, order=None, **kw):
    return EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr,
                             csr.prefix_w, csr.type_prefix, csr.n_types,
                             csr.node_type, csr.node_weight, sampler_order=order,
                             **kw)


def t2n(t):
    return t.detach().cpu().numpy()


def _check_pack(EA, O, torch, csr, s):
    """Same battery as tests/test_oracle.py::_check_pack, on the GPU, against
    vectors produced by the reference sampler."""
    G = gpu_graph(EA, csr, order=s["node_order"])
    seed = int(s["seed"]) if "seed" in s.files else SEED
    G.set_seed(seed)
    q = s["query_ids"]
    qt = torch.as_tensor(q.astype(np.int64)).cuda()
    n = 0
    while "nb_%d_1_et" % n in s.files:
        for count in (1, 5):
            key = "nb_%d_%d_" % (n, count)
            ids, w, t = G.sample_neighbor(qt, s[key + "et"], count, layout="core",
                                          call_id=11 + n)
            assert np.array_equal(t2n(ids).reshape(-1).astype(np.uint64), s[key + "id"]), key
            assert np.array_equal(t2n(w).reshape(-1), s[key + "w"]), key
            assert np.array_equal(t2n(t).reshape(-1), s[key + "t"]), key
        n += 1
    assert n >= 7
    n = 0
    while "full_%d_et" % n in s.files:
        key = "full_%d_" % n
        idx, ids, w, t = G.get_full_neighbor(qt, s[key + "et"])
        assert np.array_equal(t2n(idx), s[key + "idx"])
        assert np.array_equal(t2n(ids).astype(np.uint64), s[key + "id"])
        assert np.array_equal(t2n(w), s[key + "w"])
        assert np.array_equal(t2n(t), s[key + "t"])
        n += 1
    for n in range(4):
        got = G.sample_node(64, s["sn_%d_types" % n], call_id=100 + n)
        assert np.array_equal(t2n(got).astype(np.uint64), s["sn_%d" % n]), n
    et = s["walk_et"]
    L = et.shape[0]
    assert np.array_equal(t2n(G.random_walk(qt, et.tolist(), 1.0, 1.0, -1, call_id=200)),
                          s["walk_11"])
    assert np.array_equal(t2n(G.random_walk(qt, et.tolist(), 0.25, 4.0, -1, call_id=300)),
                          s["walk_n2v"])
    assert np.array_equal(t2n(G.random_walk(qt, et.tolist(), 2.0, 0.5, 777, call_id=400)),
                          s["walk_n2v_b"])
    assert L == 6


def test_fixture_goldens_gpu(EA, O, torch_cuda, fixture_csr, fixture_samples):
    _check_pack(EA, O, torch_cuda, fixture_csr, fixture_samples)


def test_random_graph_goldens_gpu(EA, O, torch_cuda, random_csr, random_samples):
    _check_pack(EA, O, torch_cuda, random_csr, random_samples)


@pytest.fixture(scope="module")
def big_pair(EA, O):
    rng = np.random.default_rng(77)
    ids, seg, nbr, w, nt, nw = make_random_graph(rng, 20000, 4, max_deg=40,
                                                 id_space=10 ** 12)
    csr = O.csr_from_raw(ids, seg, nbr, w, 4, nt, nw)
    return gpu_graph(EA, csr), O.OracleGraph(csr), ids, rng


@pytest.mark.parametrize("et", [[0], [3], [1, 2], [3, 0, 1], [0, 1, 2, 3], [],
                                [2, 2], [9], [1, 9]])
def test_sample_neighbor_vs_oracle(EA, O, torch_cuda, big_pair, et, k1_variant):
    torch = torch_cuda
    G, OG, ids, rng = big_pair
    q = np.concatenate([rng.choice(ids, 5000), [0, 2 ** 63 + 5]]).astype(np.uint64)
    qt = torch.as_tensor(q.astype(np.int64)).cuda()
    for count in (1, 10, 25):
        G.set_seed(99)
        idx, oid, ow, ot = OG.sample_neighbor_core(99, 5, q, et, count)
        ids_g, w_g, t_g = G.sample_neighbor(qt, et, count, layout="core", call_id=5)
        assert np.array_equal(t2n(ids_g).reshape(-1).astype(np.uint64), oid)
        assert np.array_equal(t2n(w_g).reshape(-1), ow)
        assert np.array_equal(t2n(t_g).reshape(-1), ot)
        on, ow2, ot2 = OG.sample_neighbor(99, 5, q.astype(np.int64), et, count, -7)
        ids_g, w_g, t_g = G.sample_neighbor(qt, et, count, default_node=-7, call_id=5)
        assert np.array_equal(t2n(ids_g), on)
        assert np.array_equal(t2n(w_g), ow2)
        assert np.array_equal(t2n(t_g), ot2)


def test_sample_fanout_vs_oracle(EA, O, torch_cuda, big_pair, k1_variant):
    torch = torch_cuda
    G, OG, ids, rng = big_pair
    q = np.concatenate([rng.choice(ids, 1024), [0, 12345]]).astype(np.int64)
    G.set_seed(7)
    for et, counts in (([[0, 1, 2, 3], [0, 1, 2, 3]], [25, 10]),
                       ([[1], [2]], [10, 5]), ([[0, 2], [3, 1]], [4, 3])):
        ns, ws, ts = OG.sample_fanout(7, 40, q, et, counts, 10 ** 13)
        gn, gw, gt = G.sample_fanout(torch.as_tensor(q).cuda(), et, counts,
                                     10 ** 13, call_id=40)
        assert np.array_equal(t2n(gn[0]), q)
        for h in range(len(counts)):
            assert np.array_equal(t2n(gn[h + 1]), ns[h]), (et, h)
            assert np.array_equal(t2n(gw[h]), ws[h])
            assert np.array_equal(t2n(gt[h]), ts[h])


def test_sample_node_and_walks_vs_oracle(EA, O, torch_cuda, big_pair):
    torch = torch_cuda
    G, OG, ids, rng = big_pair
    OG.build_node_sampler()
    G.set_seed(5)
    for call, types in enumerate([[-1], [0], [1], [0, 1]]):
        a = OG.sample_node(5, call, types, 4096)
        b = G.sample_node(4096, types, call_id=call)
        assert np.array_equal(t2n(b).astype(np.uint64), a)
    starts = np.concatenate([rng.choice(ids, 2000), [0]]).astype(np.int64)
    st = torch.as_tensor(starts).cuda()
    L = 12
    et = [[0, 1, 2, 3]] * L
    for p, q, dn in ((1.0, 1.0, -1), (0.5, 2.0, -1), (4.0, 0.25, 4242)):
        a = OG.random_walk(5, 1000, starts, et, L, p, q, dn)
        b = G.random_walk(st, et, p, q, dn, call_id=1000)
        assert np.array_equal(t2n(b), a), (p, q)
    et1 = [[2]] * L
    assert np.array_equal(t2n(G.random_walk(st, et1, 1.0, 1.0, -1, call_id=50)),
                          OG.random_walk(5, 50, starts, et1, L, 1.0, 1.0, -1))


def test_graph_with_node_zero_sentinel_quirk(EA, O, torch_cuda, k1_variant):
    """Q1: a live row whose first sample is node id 0 is dropped by the TF
    layout; the kernel's slow check must reproduce it."""
    torch = torch_cuda
    ids = np.array([0, 1, 2, 3], np.uint64)
    seg = np.array([0, 2, 4, 6, 7], np.int64)
    nbr = np.array([1, 2, 0, 2, 0, 3, 0], np.uint64)
    w = np.array([1, 1, 5, 1, 1, 1, 2], np.float32)
    csr = O.csr_from_raw(ids, seg, nbr, w, 1)
    G, OG = gpu_graph(EA, csr), O.OracleGraph(csr)
    q = np.array([0, 1, 2, 3, 9], np.int64)
    G.set_seed(1)
    for call in range(30):
        on, ow, ot = OG.sample_neighbor(1, call, q, [0], 3, -1)
        gn, gw, gt = G.sample_neighbor(torch.as_tensor(q).cuda(), [0], 3, -1,
                                       call_id=call)
        assert np.array_equal(t2n(gn), on)
        assert np.array_equal(t2n(gw), ow)
        assert np.array_equal(t2n(gt), ot)
    ns, ws, ts = OG.sample_fanout(1, 0, q, [[0], [0]], [3, 2], -1)
    gn, gw, gt = G.sample_fanout(torch.as_tensor(q).cuda(), [[0], [0]], [3, 2], -1,
                                 call_id=0)
    for h in range(2):
        assert np.array_equal(t2n(gn[h + 1]), ns[h])


def test_empty_and_ragged_inputs(EA, O, torch_cuda, fixture_csr):
    torch = torch_cuda
    G = gpu_graph(EA, fixture_csr)
    e = torch.zeros(0, dtype=torch.int64).cuda()
    n, w, t = G.sample_neighbor(e, [0], 5)
    assert tuple(n.shape) == (0, 5)
    n, w, t = G.sample_neighbor(torch.tensor([1, 2]).cuda(), [0], 0)
    assert tuple(n.shape) == (2, 0)
    assert tuple(G.random_walk(e, [[0]] * 3).shape) == (0, 4)
    idx, ids, w, t = G.get_full_neighbor(e, [0, 1])
    assert ids.numel() == 0
    assert G.sample_node(0, -1).numel() == 0
    # the multi-GPU pieces on empty inputs (a rank may own none of a batch's ids)
    assert tuple(G.sample_neighbor_packed(e, [0], 5).shape) == (0, 18)
    assert tuple(G.sample_neighbor_packed(e, [0, 1], 5).shape) == (0, 22)
    off, sid, pos = EA.ops.dedup_split(e, 4, 4)
    assert off == [0] * 5 and sid.numel() == 0 and pos.numel() == 0
    table = torch.zeros(9, dtype=torch.int32, device="cuda")
    off, sid, pos = EA.ops.dedup_split(e, 4, 4, dense_table=table)
    assert off == [0] * 5 and sid.numel() == 0
    rows = torch.zeros((0, 22), dtype=torch.int32, device="cuda")
    o = EA.ops.expand_packed(torch.zeros(0, dtype=torch.int32, device="cuda"), rows, 5)
    assert tuple(o[0].shape) == (0, 5)
    # one id, one shard
    off, sid, pos = EA.ops.dedup_split(torch.tensor([7]).cuda(), 1, 1, dense_table=table)
    assert off == [0, 1] and t2n(sid).tolist() == [7] and t2n(pos).tolist() == [0]
    # zero-weight type -> EEMPTY error, no output (sample_node_op.cc:118-122)
    from euler_amd._lib import EulerGpuError
    with pytest.raises(EulerGpuError):
        G.sample_node(4, 7)


def test_mp_ops_goldens_and_oracle(EA, O, torch_cuda, ref_tests):
    torch = torch_cuda
    ops = EA.ops
    t = ref_tests
    x = torch.as_tensor(t["scatter_add_x"]).cuda()
    idx = torch.as_tensor(t["scatter_idx"]).cuda()
    assert np.array_equal(t2n(ops.scatter_add(x, idx, 2)), t["scatter_add_out"])
    assert np.abs(t2n(ops.scatter_mean(x, idx, 2)) - t["scatter_mean_out"]).sum() < 1e-6
    xm = torch.as_tensor(t["scatter_max_x"]).cuda()
    assert np.array_equal(t2n(ops.scatter_max(xm, idx, 2)), t["scatter_max_out"])
    assert np.all(t2n(ops.scatter_max(xm, idx, 3))[2] == np.float32(-1e9))
    g = ops.gather(torch.as_tensor(t["gather_x"]).cuda(),
                   torch.as_tensor(t["gather_idx"]).cuda())
    assert np.array_equal(t2n(g), t["gather_out"])
    pairs = ops.gen_pair(torch.as_tensor(t["gen_pair_in"]).cuda(), 2, 2)
    assert np.array_equal(t2n(pairs), t["gen_pair_out"])
    # random shapes: bit-exact vs the sequential reference loop, sorted and
    # unsorted indices, D multiple of 4 or not
    rng = np.random.default_rng(3)
    for e, d, size, sort in ((5000, 32, 700, False), (4096, 100, 512, True),
                             (777, 7, 50, False), (1, 3, 4, False)):
        u = (rng.standard_normal((e, d)) * 100).astype(np.float32)
        i = rng.integers(0, size, e).astype(np.int32)
        if sort:
            i = np.sort(i)
        ut, it = torch.as_tensor(u).cuda(), torch.as_tensor(i).cuda()
        assert np.array_equal(t2n(ops.scatter_add(ut, it, size)), O.scatter_add(u, i, size))
        assert np.array_equal(t2n(ops.scatter_max(ut, it, size)), O.scatter_max(u, i, size))
        p = rng.standard_normal((size, d)).astype(np.float32)
        assert np.array_equal(t2n(ops.gather(torch.as_tensor(p).cuda(), it)), O.gather(p, i))
        assert np.allclose(t2n(ops.scatter_mean(ut, it, size)), O.scatter_mean(u, i, size),
                           rtol=0, atol=1e-5)


def test_gather_scatter_fused_equals_composition(EA, O, torch_cuda):
    """ops.gather_scatter(op, x, gi, si, size) - the aggregation of a message-passing step
    in one pass (euler_gpu_gather_scatter) - has the bits of scatter_(op, gather(x, gi),
    si, size) and of the oracle's sequential loops, forward, and the composition's
    gradient; sorted (sampled blocks) and unsorted destinations, D a multiple of 4 or
    not, empty destinations, repeated sources."""
    torch = torch_cuda
    ops = EA.ops
    rng = np.random.default_rng(8)
    for e, d, n, size, sort in ((6000, 128, 900, 600, True), (5000, 32, 300, 700, False),
                                (777, 7, 40, 50, False), (1, 3, 2, 4, True), (0, 8, 5, 3, True)):
        x = (rng.standard_normal((n, d)) * 50).astype(np.float32)
        gi = rng.integers(0, n, e).astype(np.int32)
        si = rng.integers(0, size, e).astype(np.int32)
        if sort:
            si = np.sort(si)
        xt = torch.as_tensor(x).cuda()
        git, sit = torch.as_tensor(gi).cuda(), torch.as_tensor(si).cuda()
        for op, oracle in (("add", O.scatter_add), ("max", O.scatter_max), ("mean", None)):
            fused = ops.gather_scatter(op, xt, git, sit, size)
            comp = ops.scatter_(op, ops.gather(xt, git), sit, size)
            assert np.array_equal(t2n(fused), t2n(comp)), (op, e, d)
            if oracle is not None and e > 0:
                assert np.array_equal(t2n(fused), oracle(O.gather(x, gi), si, size)), (op, e, d)
        if e > 1:
            for op in ("add", "mean", "max"):
                g = torch.as_tensor(rng.standard_normal((size, d)).astype(np.float32)).cuda()
                a = xt.clone().requires_grad_(True)
                b = xt.clone().requires_grad_(True)
                (ops.gather_scatter(op, a, git, sit, size) * g).sum().backward()
                (ops.scatter_(op, ops.gather(b, git), sit, size) * g).sum().backward()
                assert np.array_equal(t2n(a.grad), t2n(b.grad)), (op, e, d)
    with pytest.raises(IndexError):
        ops.gather_scatter("add", xt, torch.as_tensor([7], dtype=torch.int32).cuda(),
                           torch.as_tensor([0], dtype=torch.int32).cuda(), 2, validate=True)
    # the segmented form (a sampled block): fixed fan-out and CSR offsets, no key column
    for d, n, size, count in ((128, 5000, 700, 10), (64, 300, 90, 25), (6, 50, 33, 3), (128, 40, 5, 1)):
        x = (rng.standard_normal((n, d)) * 50).astype(np.float32)
        xt = torch.as_tensor(x).cuda()
        gi = rng.integers(0, n, size * count).astype(np.int32)
        git = torch.as_tensor(gi).cuda()
        dst = torch.arange(size, dtype=torch.int32).repeat_interleave(count).cuda()
        lens = rng.integers(0, 2 * count + 1, size)
        lens[-1] = 0
        ptr = np.zeros(size + 1, np.int64); ptr[1:] = np.cumsum(lens)
        gi2 = rng.integers(0, n, int(ptr[-1])).astype(np.int32)
        gi2t, ptrt = torch.as_tensor(gi2).cuda(), torch.as_tensor(ptr).cuda()
        dst2 = torch.as_tensor(np.repeat(np.arange(size, dtype=np.int32), lens)).cuda()
        for op in ("add", "max", "mean"):
            a = ops.gather_segment_reduce(op, xt, git, size, count=count)
            assert np.array_equal(t2n(a), t2n(ops.scatter_(op, ops.gather(xt, git), dst, size))), (op, d)
            b = ops.gather_segment_reduce(op, xt, gi2t, size, seg_ptr=ptrt)
            assert np.array_equal(t2n(b), t2n(ops.scatter_(op, ops.gather(xt, gi2t), dst2, size))), (op, d)
            g = torch.as_tensor(rng.standard_normal((size, d)).astype(np.float32)).cuda()
            p1 = xt.clone().requires_grad_(True)
            p2 = xt.clone().requires_grad_(True)
            (ops.gather_segment_reduce(op, p1, gi2t, size, seg_ptr=ptrt) * g).sum().backward()
            (ops.scatter_(op, ops.gather(p2, gi2t), dst2, size) * g).sum().backward()
            assert np.array_equal(t2n(p1.grad), t2n(p2.grad)), (op, d)
            # the indices as the int64 ids a sampler returns (read in place, low word = index;
            # euler_gpu_gather_segment_reduce_ids): same bits forward and backward
            a64 = ops.gather_segment_reduce(op, xt, git.to(torch.int64), size, count=count)
            b64 = ops.gather_segment_reduce(op, xt, gi2t.to(torch.int64), size, seg_ptr=ptrt)
            assert torch.equal(a64, a) and torch.equal(b64, b), (op, d)
            p3 = xt.clone().requires_grad_(True)
            (ops.gather_segment_reduce(op, p3, gi2t.to(torch.int64), size, seg_ptr=ptrt) * g).sum().backward()
            assert torch.equal(p3.grad, p1.grad), (op, d)
            # ids that are not rows of the table - a neighbour outside the graph, default_node = -1 -
            # read the table's LAST row forward, and the gradient flows to that same row
            bad = gi2t.to(torch.int64).clone()
            if bad.numel() > 3:
                bad[0] = -1; bad[1] = n + 12345; bad[2] = n
                ok = gi2t.clone(); ok[0] = n - 1; ok[1] = n - 1; ok[2] = n - 1
                p4 = xt.clone().requires_grad_(True)
                p5 = xt.clone().requires_grad_(True)
                f4 = ops.gather_segment_reduce(op, p4, bad, size, seg_ptr=ptrt)
                f5 = ops.gather_segment_reduce(op, p5, ok, size, seg_ptr=ptrt)
                assert torch.equal(f4, f5), (op, d)
                (f4 * g).sum().backward(); (f5 * g).sum().backward()
                assert torch.equal(p4.grad, p5.grad), (op, d)


def test_index_builds_declined(EA, O, torch_cuda):
    """Both search indexes are optimisations: with the weight-bucket index declined
    (budget 0) AND the EdgeBlocks' build failing the way an allocation failure would (tuning key
    56), the samplers run on the flat running sums - same results as the oracle for sampling,
    fanout, walks and block construction; what the failed build allocated is returned
    (graph_bytes unchanged), and the build is not retried on every call."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    p = EA.synth_params(411, 20000, 300000, n_types=2, weighted=True)
    po = O.SynthParams()
    for f, _ in po._fields_:
        setattr(po, f, getattr(p, f))
    OG = O.OracleGraph(O.synth_csr(po))
    q = np.concatenate([np.random.default_rng(3).integers(1, 20001, 3000), [0, 20001, 5, 5]]).astype(np.int64)
    qt = torch.as_tensor(q).cuda()
    try:
        _lib.check(L.euler_gpu_set_index_budget(0, -1.0))      # the weight-bucket index: never
        _lib.check(L.euler_gpu_set_tuning(56, 1))              # the next EdgeBlocks build fails
        G = EA.Graph.synthetic(p)
        G.set_seed(17)
        bytes0 = G.device_bytes
        for et, cnt in (([0], 10), ([1], 7), ([0, 1], 6)):
            gn, gw, gt = G.sample_neighbor(qt, et, cnt, -1, call_id=40)
            on, ow, ot = OG.sample_neighbor(17, 40, q, et, cnt, -1)
            assert np.array_equal(t2n(gn), on) and np.array_equal(t2n(gw), ow) and np.array_equal(t2n(gt), ot)
        assert G.device_bytes == bytes0, "the failed build's allocations were not returned"
        # (the failure was consumed by the first call and the decision remembered: a second
        # injected failure is still pending afterwards - nothing tried to build again)
        _lib.check(L.euler_gpu_set_tuning(56, 1))
        gn, gw, gt = G.sample_fanout(qt, [[0], [1]], [25, 10], -1, call_id=44)
        on, ow, ot = OG.sample_fanout(17, 44, q, [[0], [1]], [25, 10], -1)
        for h in range(2):
            assert np.array_equal(t2n(gn[h + 1]), on[h]) and np.array_equal(t2n(gw[h]), ow[h])
        walk = G.random_walk(qt[:1000], [[0, 1]] * 6, 1.0, 1.0, -1, call_id=60)
        assert np.array_equal(t2n(walk), OG.random_walk(17, 60, q[:1000], [[0, 1]] * 6, 6, 1.0, 1.0, -1))
        assert G.device_bytes == bytes0
        G2 = EA.Graph.synthetic(p)          # the pending failure meets this graph's first call
        G2.set_seed(17)
        gn, _, _ = G2.sample_neighbor(qt, [0], 4, -1, call_id=41)
        assert np.array_equal(t2n(gn), OG.sample_neighbor(17, 41, q, [0], 4, -1)[0])
    finally:
        L.euler_gpu_set_tuning(56, 0)
        L.euler_gpu_set_index_budget(-1, 0.5)
        # (-1 leaves max_bytes unchanged: put "no absolute cap" back through the environment's default)
        L.euler_gpu_set_index_budget(2 ** 62, 0.5)


def test_sparse_gather(EA, O, torch_cuda):
    """ops.sparse_gather == the restatement of tf_euler/kernels/sparse_gather_op.cc: rows of a
    row-sorted SparseTensor gathered (repeats, any order), 2 and 3 index columns, float / int64
    values, rows without entries, an empty gather, the sparse features of a graph's nodes."""
    torch = torch_cuda
    ops = EA.ops
    rng = np.random.default_rng(12)
    for rows, cols, dt in ((50, 2, np.float32), (7, 3, np.int64), (300, 2, np.int64), (1, 2, np.float32)):
        lens = rng.integers(0, 6, rows)
        r = np.repeat(np.arange(rows), lens)
        ind = np.zeros((len(r), cols), np.int64)
        ind[:, 0] = r
        for k in range(1, cols):
            ind[:, k] = rng.integers(0, 9, len(r))
        val = rng.integers(0, 1000, len(r)).astype(dt)
        shape = [rows] + [9] * (cols - 1)
        for gi in (rng.integers(0, rows, 40), np.arange(rows)[::-1].copy(), np.zeros(0, np.int64), np.array([rows - 1] * 3)):
            want = O.sparse_gather(gi, ind, val, shape)
            got = ops.sparse_gather(torch.as_tensor(gi).cuda(), torch.as_tensor(ind).cuda(),
                                    torch.as_tensor(val).cuda(), shape)
            assert np.array_equal(t2n(got[0]), want[0]) and np.array_equal(t2n(got[1]), want[1])
            assert np.array_equal(t2n(got[2]), want[2])
    with pytest.raises(IndexError):
        ops.sparse_gather(torch.as_tensor([5]).cuda(), torch.zeros((1, 2), dtype=torch.int64).cuda(),
                          torch.zeros(1).cuda(), [5, 2])
    from euler_amd.euler_ops import util_ops
    assert util_ops.sparse_gather is ops.sparse_gather


def test_inflate_idx(EA, O, torch_cuda):
    """ops.inflate_idx == the restatement of tf_euler/kernels/inflate_idx_op.cc: the two
    expectations of the reference's util_ops_test.py:44-58, random index vectors (every value
    0 .. U-1 present, heavy repeats, one value only, 1M entries), an empty vector; values outside
    [0, unique_cnt) - a hole, a negative - raise as the reference's InvalidArgument."""
    torch = torch_cuda
    ops = EA.ops
    for idx, want in (([0, 2, 1, 3], [0, 2, 1, 3]), ([0, 1, 0, 2, 1], [0, 2, 1, 4, 3])):
        assert O.inflate_idx(idx).tolist() == want
        assert t2n(ops.inflate_idx(torch.as_tensor(idx, dtype=torch.int32).cuda())).tolist() == want
    rng = np.random.default_rng(31)
    for n, u in ((1, 1), (64, 64), (257, 5), (5000, 1), (70000, 999), (1 << 20, 40000)):
        idx = np.concatenate([np.arange(u), rng.integers(0, u, n - u)]).astype(np.int32)
        rng.shuffle(idx)
        got = t2n(ops.inflate_idx(torch.as_tensor(idx).cuda()))
        if n <= 70000:
            assert np.array_equal(got, O.inflate_idx(idx))
        # the place after a stable sort by value, whatever the size
        order = np.argsort(idx, kind="stable")
        want = np.empty(n, np.int32)
        want[order] = np.arange(n, dtype=np.int32)
        assert np.array_equal(got, want)
    assert ops.inflate_idx(torch.zeros(0, dtype=torch.int32).cuda()).numel() == 0
    for bad in ([0, 2], [1, 2, 3], [0, -1], [0, 1, 1, 5]):
        with pytest.raises(ValueError):
            O.inflate_idx(bad)
        with pytest.raises(ValueError):
            ops.inflate_idx(torch.as_tensor(bad, dtype=torch.int32).cuda())
    with pytest.raises(ValueError):
        ops.inflate_idx(torch.zeros((2, 2), dtype=torch.int32).cuda())
    from euler_amd.euler_ops import util_ops
    assert util_ops.inflate_idx is ops.inflate_idx


def test_mp_gradients(EA, torch_cuda):
    """mp_ops_test.py:38-94 check compute_gradient_error < 1e-4; here the
    registered gradients are compared with torch's own autograd of the same
    math (index_add / index_select / amax)."""
    torch = torch_cuda
    ops = EA.ops
    x = torch.tensor([[1., 2., 7.], [3., 4., 8.], [5., 6., 7.]], device="cuda",
                     requires_grad=True)
    idx = torch.tensor([1, 0, 1], device="cuda")
    g = torch.tensor([[1., 2., 3.], [4., 5., 6.]], device="cuda")
    ops.scatter_add(x, idx, 2).backward(g)
    assert torch.allclose(x.grad, g[idx])
    x.grad = None
    ops.scatter_mean(x, idx, 2).backward(g)
    cnt = torch.tensor([[1.], [2.]], device="cuda") + 1e-7
    assert torch.allclose(x.grad, (g / cnt)[idx], atol=1e-6)
    x.grad = None
    ops.scatter_max(x, idx, 2).backward(g)
    ref = torch.zeros_like(x)
    ref[1] = g[0]
    ref[2, 0:2] = g[1, 0:2]
    ref[0, 2] = g[1, 2] / 2
    ref[2, 2] = g[1, 2] / 2
    assert torch.allclose(x.grad, ref)
    p = torch.tensor([[1., 2.], [3., 4.], [5., 6.]], device="cuda", requires_grad=True)
    gi = torch.tensor([1, 0, 1, 2], device="cuda")
    go = torch.arange(8, dtype=torch.float32, device="cuda").reshape(4, 2)
    ops.gather(p, gi).backward(go)
    ref = torch.zeros_like(p).index_add_(0, gi, go)
    assert torch.allclose(p.grad, ref)


def test_unique_gather_split_merge(EA, O, torch_cuda):
    torch = torch_cuda
    ops = EA.ops
    uq, gi = ops.id_unique(torch.tensor([1, 2, 3, 3, 2, 2, 4]).cuda())
    assert t2n(uq).tolist() == [1, 2, 3, 4]
    assert t2n(gi).tolist() == [0, 1, 2, 2, 1, 1, 3]
    idx = torch.tensor([[0, 2], [2, 5], [5, 6]], dtype=torch.int32).cuda()
    gidx = torch.tensor([0, 1, 0, 2, 1], dtype=torch.int32).cuda()
    oi, tot = ops.idx_gather(idx, gidx)
    assert t2n(oi).reshape(-1).tolist() == [0, 2, 2, 5, 5, 7, 7, 8, 8, 11]
    data = torch.tensor([11, 12, 21, 22, 23, 31]).cuda()
    assert t2n(ops.data_gather(data, idx, gidx)).tolist() == [
        11, 12, 21, 22, 23, 11, 12, 31, 21, 22, 23]
    rng = np.random.default_rng(11)
    ids = rng.integers(0, 5000, 40000).astype(np.uint64)
    ids[::97] = np.uint64(2 ** 64 - 1)
    uq_o, gi_o = O.id_unique(ids)
    uq, gi = ops.id_unique(torch.as_tensor(ids.astype(np.int64)).cuda())
    assert np.array_equal(t2n(uq).astype(np.uint64), uq_o)
    assert np.array_equal(t2n(gi), gi_o)
    for parts, shards in ((8, 3), (1024, 8), (8, 8), (5, 1)):
        off_o, sid_o, mi_o = O.id_split(ids, parts, shards)
        off, sid, mi = ops.id_split(torch.as_tensor(ids.astype(np.int64)).cuda(),
                                    parts, shards)
        assert list(off) == off_o.tolist()
        assert np.array_equal(t2n(sid).astype(np.uint64), sid_o)
        assert np.array_equal(t2n(mi), mi_o)
        rows = torch.as_tensor(rng.integers(0, 9, (len(ids), 3)).astype(np.int32)).cuda()
        merged = ops.merge_rows(rows, mi)
        assert np.array_equal(t2n(merged)[mi_o], t2n(rows))


def test_synthetic_graph_matches_host_generator(EA, O, torch_cuda, k1_variant):
    torch = torch_cuda
    for weighted, T in ((True, 1), (False, 1), (True, 3)):
        p = EA.synth_params(4242, 30000, 300000, n_types=T, weighted=weighted)
        po = O.SynthParams()
        for f, _ in po._fields_:
            setattr(po, f, getattr(p, f))
        csr = O.synth_csr(po)
        G = EA.Graph.synthetic(p)
        assert G.num_nodes == 30000 and G.num_edges == len(csr.nbr)
        ids = np.arange(1, 30001, dtype=np.uint64)
        row_ptr, type_end, nbr, pw, tp = G.export_rows(ids)
        assert np.array_equal(row_ptr, csr.row_ptr)
        assert np.array_equal(type_end, csr.type_end)
        assert np.array_equal(nbr, csr.nbr)
        assert np.array_equal(pw, csr.prefix_w)
        assert np.array_equal(tp, csr.type_prefix)
        OG = O.OracleGraph(csr)
        q = np.random.default_rng(1).integers(1, 30001, 4096).astype(np.int64)
        G.set_seed(3)
        et = [[0]] * 2 if T == 1 else [[0, 2], [2, 1]]
        ns, ws, ts = OG.sample_fanout(3, 0, q, et, [25, 10], 30001)
        gn, gw, gt = G.sample_fanout(torch.as_tensor(q).cuda(), et, [25, 10], 30001,
                                     call_id=0)
        for h in range(2):
            assert np.array_equal(t2n(gn[h + 1]), ns[h])
            assert np.array_equal(t2n(gw[h]), ws[h])
            assert np.array_equal(t2n(gt[h]), ts[h])
        # sharded build: shard s of 4 owns ids == s (mod 4); same samples
        shards = [EA.Graph.synthetic(p, partitions=4, shard_index=s, shards=4)
                  for s in range(4)]
        assert sum(g.num_nodes for g in shards) == 30000
        for s, g in enumerate(shards):
            own = q[q % 4 == s]
            g.set_seed(3)
            a, b, c = g.sample_neighbor(torch.as_tensor(own).cuda(), et[0], 25,
                                        30001, call_id=0)
            ref = t2n(gn[1]).reshape(-1, 25)[q % 4 == s]
            assert np.array_equal(t2n(a), ref)


def test_synthetic_hashed_ids_two_types(EA, O, torch_cuda):
    """The synthetic graph with hashed u64 ids (node x known outside as mix64(x): hash id map)
    and two edge-type groups - what a dataset converted by euler/tools looks like, and what
    bench.py's metric_hashed_T2 leg runs: device generator == host generator, the id map finds
    every row and nothing else, and the 2-hop fanout (SampleFanoutLocalKernel: the general
    build of the one-kernel step) == hop by hop == the oracle."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    p = EA.synth_params(4242, 30000, 300000, n_types=2, weighted=True, hashed_ids=True)
    po = O.SynthParams()
    for f, _ in po._fields_:
        setattr(po, f, getattr(p, f))
    csr = O.synth_csr(po)
    G = EA.Graph.synthetic(p)
    assert G.num_nodes == 30000 and G.num_edges == len(csr.nbr)
    assert len(np.unique(csr.row_id)) == 30000 and csr.row_id.min() > 0
    row_ptr, type_end, nbr, pw, tp = G.export_rows(csr.row_id)
    assert np.array_equal(row_ptr, csr.row_ptr) and np.array_equal(type_end, csr.type_end)
    assert np.array_equal(nbr, csr.nbr) and np.array_equal(pw, csr.prefix_w)
    assert np.array_equal(tp, csr.type_prefix)
    # ids that are not in the graph (the internal numbers themselves) find nothing
    rp0 = G.export_rows(np.arange(1, 200, dtype=np.uint64))[0]
    assert rp0[-1] == 0
    OG = O.OracleGraph(csr)
    rng = np.random.default_rng(1)
    q = np.concatenate([rng.choice(csr.row_id, 40000), [0, 5, 2 ** 63 + 9]]).astype(np.uint64).view(np.int64)
    qt = torch.as_tensor(q).cuda()
    try:
        for et, counts in (([[0], [0]], [25, 10]), ([[1], [0]], [5, 4]), ([[0, 1], [1, 0]], [6, 3])):
            G.set_seed(3)
            ns, ws, ts = OG.sample_fanout(3, 10, q, et, counts, -1)
            res = []
            # the one-kernel step with the record in the 64-byte hash slot (key 49 = 1) / through
            # the 16-byte slot and the row's record / hop by hop
            for key27, key49 in ((1, 1), (1, 0), (0, 1)):
                L.euler_gpu_set_tuning(27, key27)
                L.euler_gpu_set_tuning(49, key49)
                gn, gw, gt = G.sample_fanout(qt, et, counts, -1, call_id=10)
                for h in range(2):
                    assert np.array_equal(t2n(gn[h + 1]), ns[h]), (et, counts, key27, key49, h)
                    assert np.array_equal(t2n(gw[h]), ws[h]) and np.array_equal(t2n(gt[h]), ts[h])
        # the other graphs that get fat slots: uniform weights (row records alone, no buckets) and
        # one edge-type group behind a hash id map
        for n_types, weighted in ((2, False), (1, True), (1, False)):
            p2 = EA.synth_params(77, 30000, 300000, n_types=n_types, weighted=weighted, hashed_ids=True)
            po2 = O.SynthParams()
            for f, _ in po2._fields_:
                setattr(po2, f, getattr(p2, f))
            csr2 = O.synth_csr(po2)
            G2 = EA.Graph.synthetic(p2)
            G2.set_seed(3)
            OG2 = O.OracleGraph(csr2)
            q2 = np.concatenate([rng.choice(csr2.row_id, 40000), [0, 5]]).astype(np.uint64).view(np.int64)
            q2t = torch.as_tensor(q2).cuda()
            ets = [[[0], [0]]] + ([[[1], [0]], [[0, 1], [0, 1]]] if n_types == 2 else [])
            for et in ets:
                ns, ws, ts = OG2.sample_fanout(3, 10, q2, et, [25, 10], -1)
                for key49 in (1, 0):
                    L.euler_gpu_set_tuning(49, key49)
                    gn, gw, gt = G2.sample_fanout(q2t, et, [25, 10], -1, call_id=10)
                    for h in range(2):
                        assert np.array_equal(t2n(gn[h + 1]), ns[h]), (n_types, weighted, et, key49, h)
                        assert np.array_equal(t2n(gw[h]), ws[h]) and np.array_equal(t2n(gt[h]), ts[h])
    finally:
        L.euler_gpu_set_tuning(27, 1)
        L.euler_gpu_set_tuning(49, 1)


def test_op_registry_and_dat_loader(EA, O, torch_cuda, fixture_csr, tmp_path):
    """The plugin-API mirror dispatches API_SAMPLE_NB to the GPU; the .dat
    reader loads what euler/tools writes."""
    import ctypes as C
    from euler_amd import _lib
    L = _lib.lib()
    for op in (b"API_SAMPLE_NB", b"API_SAMPLE_NODE", b"ID_UNIQUE", b"IDX_GATHER",
               b"DATA_GATHER", b"API_GET_NB_NODE"):
        assert L.euler_op_registered(op) == 1
    G = gpu_graph(EA, fixture_csr)
    OG = O.OracleGraph(fixture_csr)
    q = np.array([1, 2, 3, 4, 5, 6, 42], np.uint64)
    et = np.array([0, 1], np.int32)
    n, count = len(q), 4
    idx = np.zeros((n, 2), np.int32)
    oid = np.zeros(n * count, np.uint64)
    ow = np.zeros(n * count, np.float32)
    ot = np.zeros(n * count, np.int32)
    got = L.euler_op_run_sample_nb(G._h, 77, q.ctypes.data_as(_lib.u64p), n,
                                   et.ctypes.data_as(_lib.i32p), 2, count,
                                   idx.ctypes.data_as(_lib.i32p),
                                   oid.ctypes.data_as(_lib.u64p),
                                   ow.ctypes.data_as(_lib.f32p),
                                   ot.ctypes.data_as(_lib.i32p))
    assert got == n * count
    ridx, rid, rw, rt = OG.sample_neighbor_core(77, 0, q, et, count)
    assert np.array_equal(idx, ridx) and np.array_equal(oid, rid)
    assert np.array_equal(ow, rw) and np.array_equal(ot, rt)
    # API_GET_NB_NODE through the plugin API, with the post-process strings the
    # TF top-k op compiles to (get_top_k_neighbor_op.cc:36-44)
    cap = 64
    idx = np.zeros((n, 2), np.int32); oid = np.zeros(cap, np.uint64)
    ow = np.zeros(cap, np.float32); ot = np.zeros(cap, np.int32)
    got = L.euler_op_run_get_nb(G._h, q.ctypes.data_as(_lib.u64p), n,
                                et.ctypes.data_as(_lib.i32p), 2,
                                b"order_by weight desc;limit 2", cap,
                                idx.ctypes.data_as(_lib.i32p), oid.ctypes.data_as(_lib.u64p),
                                ow.ctypes.data_as(_lib.f32p), ot.ctypes.data_as(_lib.i32p))
    want = O.neighbor_post_process(*OG.get_full_neighbor(q, et), order_by="weight",
                                   desc=True, limit=2)
    assert got == len(want[1])
    assert np.array_equal(idx, want[0]) and np.array_equal(oid[:got], want[1])
    assert np.array_equal(ow[:got], want[2]) and np.array_equal(ot[:got], want[3])
    # .dat round trip written with the record layout of node.cc:414-526
    from test_host import write_dat_dir
    write_dat_dir(tmp_path, fixture_csr, partitions=2)
    G2 = EA.Graph.load(str(tmp_path))
    assert G2.num_nodes == 6 and G2.num_edges == 12
    assert G2.partitions == 2 and G.partitions == 0       # euler.meta's partitions_num
    rp, te, nb, pw, tp = G2.export_rows(fixture_csr.row_id)
    assert np.array_equal(nb, fixture_csr.nbr) and np.array_equal(pw, fixture_csr.prefix_w)
    assert np.array_equal(te, fixture_csr.type_end) and np.array_equal(tp, fixture_csr.type_prefix)
    assert EA.initialize_embedded_graph(str(tmp_path))
    EA.set_seed(9)
    nb_ids, _, _ = EA.sample_neighbor(torch_cuda.tensor([1, 6]).cuda(), [0, 1], 3)
    exp, _, _ = OG.sample_neighbor(9, 0, np.array([1, 6], np.int64), [0, 1], 3, -1)
    assert np.array_equal(t2n(nb_ids), exp)


def test_full_size_properties(EA, O, torch_cuda):
    """At a size no CPU structure is asked to hold (2M nodes / 20M edges here;
    bench.py does the same at 100M / 1B): determinism, membership (every
    sampled (id, weight) is an edge of the root) and a bit-exact spot check of
    1000 roots against the oracle fed with the exported rows."""
    torch = torch_cuda
    p = EA.synth_params(20240521, 2_000_000, 20_000_000, weighted=True)
    G = EA.Graph.synthetic(p)
    rng = np.random.default_rng(5)
    q = rng.integers(1, 2_000_001, 200_000).astype(np.int64)
    qt = torch.as_tensor(q).cuda()
    G.set_seed(123)
    a = G.sample_neighbor(qt, [0], 25, 2_000_001, call_id=9)
    b = G.sample_neighbor(qt, [0], 25, 2_000_001, call_id=9)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    sel = rng.choice(len(q), 1000, replace=False)
    rows = np.unique(q[sel]).astype(np.uint64)
    row_ptr, type_end, nbr, pw, tp = G.export_rows(rows)
    csr = O.CSR(rows, row_ptr, type_end, nbr, pw, tp, 1)
    OG = O.OracleGraph(csr)
    on, ow, ot = OG.sample_neighbor(123, 9, q[sel], [0], 25, 2_000_001)
    assert np.array_equal(t2n(a[0])[sel], on)
    assert np.array_equal(t2n(a[1])[sel], ow)
    assert np.array_equal(t2n(a[2])[sel], ot)


def test_node2vec_on_the_metric_graph_hub_rows(EA, O, torch_cuda):
    """node2vec (p = 0.25, q = 4) on the 100M-node / 1B-edge graph of the headline metric,
    walkers started on its largest rows (578 088 and 182 555 neighbours: 2 259 chunks of
    256, checkpoints 8 chunks apart, long runs of integer running sums): the one-launch
    kernel and the per-step launch agree, and both equal the oracle fed with the rows
    exported from HBM for every node the walks visit."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    N = 100_000_000
    G = EA.Graph.synthetic(EA.synth_params(20240521, N, 10 * N, weighted=True))
    G.set_seed(99)
    rng = np.random.default_rng(12)
    starts = np.concatenate([[1, 2, 3, 5, 9, 17, 33, 1, 2], rng.integers(1, N + 1, 23)]).astype(np.int64)
    st = torch.as_tensor(starts).cuda()
    steps = 4
    et = [[0]] * steps
    try:
        L.euler_gpu_set_tuning(7, 2)
        a = G.random_walk(st, et, 0.25, 4.0, N + 1, call_id=7)
        L.euler_gpu_set_tuning(7, 3)
        b = G.random_walk(st, et, 0.25, 4.0, N + 1, call_id=7)
    finally:
        L.euler_gpu_set_tuning(7, 2)
    assert torch.equal(a, b)
    walks = t2n(a)
    rows = np.unique(walks[walks <= N]).astype(np.uint64)
    row_ptr, type_end, nbr, pw, tp = G.export_rows(rows)
    assert int(np.diff(row_ptr).max()) == 578088
    OG = O.OracleGraph(O.CSR(rows, row_ptr, type_end, nbr, pw, tp, 1))
    want = OG.random_walk(99, 7, starts, et, steps, 0.25, 4.0, N + 1)
    assert np.array_equal(walks, want)
    # DeepWalk (configs[3]: length 40, p = q = 1) from the same graph, same check
    dw = t2n(G.random_walk(st[:16], [[0]] * 40, 1.0, 1.0, N + 1, call_id=100))
    rows = np.unique(dw[dw <= N]).astype(np.uint64)
    row_ptr, type_end, nbr, pw, tp = G.export_rows(rows)
    OG = O.OracleGraph(O.CSR(rows, row_ptr, type_end, nbr, pw, tp, 1))
    assert np.array_equal(dw, OG.random_walk(99, 100, starts[:16], [[0]] * 40, 40, 1.0, 1.0, N + 1))


def test_non_monotone_rows_use_reference_loop(EA, O, torch_cuda):
    """Negative weights make the running sums non-monotone; the reference's
    RandomSelect then reads outside the row (size_t underflow of `mid - 1`,
    compact_weighted_collection.h:45), so there is no oracle answer to compare
    with.  The builder detects such rows (GraphView::monotone = 0), K1 stays on
    the bounded reference loop, and the call must stay memory-safe and
    deterministic and return neighbours of the right row."""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    n = 400
    ids = np.arange(1, n + 1).astype(np.uint64)
    deg = rng.integers(1, 30, n)
    seg = np.zeros(n + 1, np.int64)
    seg[1:] = np.cumsum(deg)
    nbr = rng.choice(ids, int(seg[-1])).astype(np.uint64)
    w = (rng.random(int(seg[-1])) * 4 - 1).astype(np.float32)   # some negative
    csr = O.csr_from_raw(ids, seg, nbr, w, 1)
    G = gpu_graph(EA, csr)
    G.set_seed(2)
    q = rng.choice(ids, 3000).astype(np.int64)
    a = G.sample_neighbor(torch.as_tensor(q).cuda(), [0], 8, -1, call_id=1)
    b = G.sample_neighbor(torch.as_tensor(q).cuda(), [0], 8, -1, call_id=1)
    assert np.array_equal(t2n(a[0]), t2n(b[0]))
    got = t2n(a[0]).astype(np.uint64)
    for i in range(0, 3000, 97):
        r = int(q[i]) - 1
        row = set(nbr[seg[r]:seg[r + 1]].tolist()) | {2 ** 64 - 1}
        assert set(got[i].tolist()) <= row


@pytest.fixture(params=[(2, 0), (2, 1), (1, 0), (0, 0)],
                ids=["onepass", "onepass_resolve_in_expand", "blocknum", "scan"])
def dedup_numbering(request):
    """Every way of numbering the distinct roots (tuning key 14): one pass with
    workgroup-level atomics (the default; with the expansion reading the owner table
    itself, or with the separate resolve kernel: key 20), per-workgroup counts + one
    small scan, and the device-wide scan over the positions."""
    from euler_amd import _lib
    _lib.lib().euler_gpu_set_tuning(14, request.param[0])
    _lib.lib().euler_gpu_set_tuning(20, request.param[1])
    yield request.param
    _lib.lib().euler_gpu_set_tuning(14, 2)
    _lib.lib().euler_gpu_set_tuning(20, 0)


@pytest.mark.parametrize("et", [[0], [1, 2], []])
@pytest.mark.parametrize("count", [10, 7])
def test_duplicate_roots_take_the_unique_path(EA, O, torch_cuda, big_pair, et, count,
                                              dedup_numbering):
    """40 000 roots drawn from 300 nodes (plus unknown ids and the sentinel):
    the launcher counts duplicates on device, samples each distinct node once
    and expands - ID_UNIQUE -> sample -> GATHER of the reference
    (parser/compiler.cc:76-90).  Results must equal the oracle's row by row, in
    both layouts, with the row mask."""
    torch = torch_cuda
    G, OG, ids, rng = big_pair
    pool = np.concatenate([rng.choice(ids, 300), [0, 2 ** 63 + 5, 12345]]).astype(np.uint64)
    q = rng.choice(pool, 40000).astype(np.uint64)
    qt = torch.as_tensor(q.astype(np.int64)).cuda()
    G.set_seed(4)
    idx, oid, ow, ot = OG.sample_neighbor_core(4, 9, q, et, count)
    ids_g, w_g, t_g = G.sample_neighbor(qt, et, count, layout="core", call_id=9)
    assert np.array_equal(t2n(ids_g).reshape(-1).astype(np.uint64), oid)
    assert np.array_equal(t2n(w_g).reshape(-1), ow)
    assert np.array_equal(t2n(t_g).reshape(-1), ot)
    on, ow2, ot2 = OG.sample_neighbor(4, 9, q.astype(np.int64), et, count, -7)
    ids_g, w_g, t_g, m_g = G.sample_neighbor(qt, et, count, default_node=-7, call_id=9,
                                             return_mask=True)
    assert np.array_equal(t2n(ids_g), on)
    assert np.array_equal(t2n(w_g), ow2)
    assert np.array_equal(t2n(t_g), ot2)
    assert np.array_equal(t2n(m_g) != 0, (on[:, 0] == -7) & (ot2[:, 0] == -1))


def test_fanout_second_hop_dedup(EA, O, torch_cuda, big_pair):
    """26 000 roots, fanout [8, 6]: hop 2 has 208 000 roots with many repeats and
    goes through the duplicate-root path automatically (>= 200 000 roots)."""
    torch = torch_cuda
    G, OG, ids, rng = big_pair
    q = np.concatenate([rng.choice(ids, 25998), [0, 777]]).astype(np.int64)
    G.set_seed(12)
    gn, gw, gt = G.sample_fanout(torch.as_tensor(q).cuda(), [[0], [1]], [8, 6], -1,
                                 call_id=3)
    on, ow, ot = OG.sample_fanout(12, 3, q, [[0], [1]], [8, 6], -1)
    for h in range(2):
        assert np.array_equal(t2n(gn[h + 1]), on[h])
        assert np.array_equal(t2n(gw[h]), ow[h])
        assert np.array_equal(t2n(gt[h]), ot[h])


def test_gpu_sharded_sampler_single_rank(EA, O, torch_cuda, big_pair):
    """The multi-GPU sampler with its real HIP pieces (id_unique, id_split,
    merge_rows, gather) and RCCL, on a one-rank group: ids and rows go through
    unique -> split -> all-to-all -> sample -> all-to-all -> merge -> gather and
    must come back equal to the oracle's fanout and walk (the N > 1 host logic
    is covered with gloo in test_distributed_cpu.py)."""
    torch = torch_cuda
    import torch.distributed as dist
    from euler_amd.distributed import gpu_sharded_sampler
    G, OG, ids, rng = big_pair
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        G.set_seed(31)
        q = np.concatenate([rng.choice(ids, 3000), rng.choice(ids[:50], 3000),
                            [0, 999]]).astype(np.int64)
        # type draws take the reference loop (sample, then pack); single-type
        # hops are written as wire rows by the sampling kernel itself
        for ets, cnts in (([[0, 1], [2, 3]], [6, 4]), ([[0], [1]], [6, 5]), ([[2], [2]], [3, 4])):
            on, ow, ot = OG.sample_fanout(31, 8, q, ets, cnts, -1)
            for dedup, packed in ((True, True), (True, False), ("ops", True), (False, True)):
                S = gpu_sharded_sampler(G, partitions=1, dedup=dedup, packed=packed)
                gn, gw, gt = S.sample_fanout(torch.as_tensor(q).cuda(), ets, cnts, -1, call_id=8)
                for h in range(2):
                    assert np.array_equal(t2n(gn[h + 1]), on[h]), (ets, dedup, packed, h)
                    assert np.array_equal(t2n(gw[h]), ow[h])
                    assert np.array_equal(t2n(gt[h]), ot[h])
        # A lone rank's ids never leave it, so the hops above made no exchange at all.  With the
        # exchanges MADE - the rank sends itself what N ranks send one another - RCCL's all-to-all
        # executes on this box: the Python orchestration (dist.all_to_all_single on nccl) and the C
        # entries over the callback transport (tuning key 52), fanout and walk.
        from euler_amd.distributed import c_sharded_sample_fanout, c_sharded_random_walk
        from euler_amd import _lib
        qt = torch.as_tensor(q).cuda()
        ets, cnts = [[0], [1]], [6, 5]
        on, ow, ot = OG.sample_fanout(31, 8, q, ets, cnts, -1)
        S = gpu_sharded_sampler(G, partitions=1)
        S.force_exchange = True
        x0 = S.exchanges
        gn, gw, gt = S.sample_fanout(qt, ets, cnts, -1, call_id=8)
        assert S.exchanges > x0
        for h in range(2):
            assert np.array_equal(t2n(gn[h + 1]), on[h]) and np.array_equal(t2n(gw[h]), ow[h])
        walk_ref = G.random_walk(qt, [[0]] * 5, 1.0, 1.0, -1, call_id=90)
        _lib.check(_lib.lib().euler_gpu_set_tuning(52, 1))
        try:
            gn, gw, gt = c_sharded_sample_fanout(G, S.c_transport, qt, ets, cnts, -1, call_id=8, partitions=1)
            for h in range(2):
                assert np.array_equal(t2n(gn[h + 1]), on[h]) and np.array_equal(t2n(gw[h]), ow[h])
                assert np.array_equal(t2n(gt[h]), ot[h])
            walk = c_sharded_random_walk(G, S.c_transport, qt, [[0]] * 5, -1, 90, 1, 1, S.dense_table)
            assert torch.equal(walk, walk_ref)
        finally:
            _lib.lib().euler_gpu_set_tuning(52, 0)
        S = gpu_sharded_sampler(G, partitions=1)
        # full neighbours through the exchange (variable-length merge)
        qf = torch.as_tensor(q).cuda()
        for et_ in ([0, 1, 2, 3], [2], [3, 1]):
            gi_, gd_, gw_, gt_ = S.get_full_neighbor(qf, et_)
            wi_, wd_, ww_, wt_ = OG.get_full_neighbor(q.astype(np.uint64), et_)
            assert np.array_equal(t2n(gi_), wi_) and np.array_equal(t2n(gd_).astype(np.uint64), wd_)
            assert np.array_equal(t2n(gw_), ww_) and np.array_equal(t2n(gt_), wt_)
        # SampleNode over the (single) shard: split + local draw + append
        G.set_seed(31)
        for nt, cnt in ((-1, 300), (0, 40), (1, 7)):
            assert torch.equal(S.sample_node(cnt, nt, call_id=60),
                               G.sample_node(cnt, nt, call_id=60))
        # dense features through the exchange
        n_f = 3000
        f_ids = np.arange(5, 5 + n_f).astype(np.uint64)
        f_csr = O.csr_from_raw(f_ids, np.arange(n_f + 1, dtype=np.int64),
                               rng.choice(f_ids, n_f), np.ones(n_f, np.float32), 1)
        f_val = rng.standard_normal((n_f, 48)).astype(np.float32)
        Ff = O.DenseFeatures(2, np.arange(n_f + 1) * 48, np.tile([32, 48], n_f),
                             f_val.reshape(-1))
        Gf = gpu_graph(EA, f_csr, features=(2, Ff.feat_ptr, Ff.feat_idx, Ff.feat_val))
        Sf = gpu_sharded_sampler(Gf, partitions=1)
        fq = np.concatenate([rng.choice(f_ids, 20000), [0, 1]]).astype(np.int64)
        got_f = Sf.get_dense_feature(torch.as_tensor(fq).cuda(), [0, 1], [32, 16])
        want_f = O.OracleGraph(f_csr).get_dense_feature(Ff, fq, [0, 1], [32, 16])
        assert np.array_equal(t2n(got_f[0]), want_f[0])
        assert np.array_equal(t2n(got_f[1]), want_f[1])
        assert Sf.dense_table is not None and S.dense_table is None
        # layerwise sampling through the exchange == the single-GPU op == the oracle
        for batch_l, n_l, cnt_l, et_l in ((8, 25, 10, [0, 1]), (1, 400, 64, [2]), (5, 1, 3, [0, 1, 2, 3])):
            nodes_l = rng.choice(ids, (batch_l, n_l)).astype(np.uint64)
            nodes_l[0, 0] = nodes_l[0, -1]
            nt_l = torch.as_tensor(nodes_l.view(np.int64)).cuda()
            got_nb, (gi_, gv_, gs_) = S.sample_neighbor_layerwise(nt_l, et_l, cnt_l, -1, call_id=71)
            one_nb, (oi_, ov_, os_) = G.sample_neighbor_layerwise(nt_l, et_l, cnt_l, -1, call_id=71)
            wnb, wi_, wv_, ws_ = OG.sample_neighbor_layerwise(31, 71, nodes_l, et_l, cnt_l, -1)
            assert np.array_equal(t2n(got_nb), wnb) and np.array_equal(t2n(one_nb), wnb)
            assert np.array_equal(t2n(gi_), wi_) and np.array_equal(t2n(gv_), wv_)
            assert np.array_equal(t2n(oi_), wi_) and list(gs_) == list(ws_) == list(os_)
            got_nb, (gi_, gv_, gs_) = S.sample_neighbor_layerwise(nt_l, et_l, cnt_l, -1, call_id=72,
                                                                  weight_func="sqrt")
            wf_ = OG.sample_neighbor_layerwise_func(31, 72, nodes_l, et_l, cnt_l, "sqrt", -1)
            assert np.array_equal(t2n(got_nb), wf_[0]) and np.array_equal(t2n(gi_), wf_[3])
            assert np.array_equal(t2n(gv_), wf_[4])
        # sparse (uint64) features through the exchange: variable-length answers +
        # the TF kernel's default entries on the requester
        sper = [[list(rng.integers(0, 2 ** 63, int(rng.integers(0, 5)), dtype=np.uint64)),
                 [int(v)] * (i % 3)] if i % 7 else [[]] for i, v in enumerate(f_ids)]
        SF = O.SparseFeatures.from_lists(sper)
        Gs = gpu_graph(EA, f_csr, sparse_features=(SF.n_u64, SF.feat_ptr, SF.feat_idx,
                                                    SF.feat_val))
        Ss = gpu_sharded_sampler(Gs, partitions=1)
        got_s = Ss.get_sparse_feature(torch.as_tensor(fq).cuda(), [0, 1, 4], [0, 11, -1])
        want_s = O.OracleGraph(f_csr).get_sparse_feature(SF, fq.astype(np.uint64), [0, 1, 4],
                                                         [0, 11, -1])
        direct = Gs.get_sparse_feature(torch.as_tensor(fq).cuda(), [0, 1, 4], [0, 11, -1])
        for (gi_, gv_, gs_), (wi_, wv_, ws_), (di_, dv_, ds_) in zip(got_s, want_s, direct):
            assert np.array_equal(t2n(gi_), wi_) and np.array_equal(t2n(gv_), wv_)
            assert list(gs_) == list(ws_) == list(ds_)
            assert np.array_equal(t2n(di_), wi_) and np.array_equal(t2n(dv_), wv_)
        # a fanout through the id-indexed front end (ids base + stride * row)
        n_i = 20000
        i_ids = (7 + 3 * np.arange(n_i)).astype(np.uint64)
        i_deg = rng.integers(0, 25, n_i)
        i_seg = np.zeros(n_i + 1, np.int64)
        i_seg[1:] = np.cumsum(i_deg)
        i_nbr = rng.choice(i_ids, int(i_seg[-1])).astype(np.uint64)
        i_nbr[rng.random(len(i_nbr)) < 0.02] += 1          # no such node
        i_csr = O.csr_from_raw(i_ids, i_seg, i_nbr,
                               (rng.random(len(i_nbr)) * 5 + 0.5).astype(np.float32), 1)
        Gi = gpu_graph(EA, i_csr)
        Gi.set_seed(31)
        Si = gpu_sharded_sampler(Gi, partitions=1)
        assert Si.dense_table is not None
        qi = np.concatenate([rng.choice(i_ids, 4000), [0, 8, 7 + 3 * n_i, 2 ** 40]]).astype(np.int64)
        on_i, ow_i, ot_i = O.OracleGraph(i_csr).sample_fanout(31, 70, qi, [[0], [0]], [8, 5], -1)
        gn_i, gw_i, gt_i = Si.sample_fanout(torch.as_tensor(qi).cuda(), [[0], [0]], [8, 5], -1,
                                            call_id=70)
        for h in range(2):
            assert np.array_equal(t2n(gn_i[h + 1]), on_i[h])
            assert np.array_equal(t2n(gw_i[h]), ow_i[h])
            assert np.array_equal(t2n(gt_i[h]), ot_i[h])
        # differential fuzz: the sharded hop (front end, wire rows, expansion) against
        # the single-GPU fanout on random graphs with both kinds of id map
        for trial in range(10):
            n_z = int(rng.integers(300, 30000))
            if trial % 2:
                z_ids = (int(rng.integers(0, 9)) + int(rng.integers(1, 4)) * np.arange(n_z)).astype(np.uint64)
            else:
                z_ids = np.unique(rng.integers(1, 10 ** 10, 2 * n_z)).astype(np.uint64)[:n_z]
                n_z = len(z_ids)
            z_deg = rng.integers(0, 40, size=(n_z, 2))
            z_deg[rng.random((n_z, 2)) < 0.3] = 0
            z_seg = np.zeros(2 * n_z + 1, np.int64)
            z_seg[1:] = np.cumsum(z_deg.reshape(-1))
            z_nbr = rng.choice(z_ids, int(z_seg[-1])).astype(np.uint64)
            z_nbr[rng.random(len(z_nbr)) < 0.02] = 10 ** 12 + 3
            z_csr = O.csr_from_raw(z_ids, z_seg, z_nbr,
                                   (rng.random(len(z_nbr)) * 3 + 0.5).astype(np.float32), 2)
            Gz = gpu_graph(EA, z_csr)
            Gz.set_seed(500 + trial)
            Sz = gpu_sharded_sampler(Gz, partitions=int(rng.integers(1, 9)), packed=bool(trial % 3))
            assert (Sz.dense_table is not None) == bool(trial % 2)
            cnts = [int(c) for c in rng.integers(1, 8, 2)]
            ets = [[int(rng.integers(0, 2))], [int(rng.integers(0, 2))]] if trial % 4 else [[0, 1], [0, 1]]
            qz = torch.as_tensor(np.concatenate([rng.choice(z_ids, int(rng.integers(1, 5000))), [0]])
                                 .astype(np.int64)).cuda()
            want = Gz.sample_fanout(qz, ets, cnts, -1, call_id=9)
            got = Sz.sample_fanout(qz, ets, cnts, -1, call_id=9)
            for h in range(2):
                assert torch.equal(got[0][h + 1], want[0][h + 1]), (trial, h)
                assert torch.equal(got[1][h], want[1][h]) and torch.equal(got[2][h], want[2][h])
        L = 5
        et = [[0, 1, 2, 3]] * L
        walk = S.random_walk(torch.as_tensor(q).cuda(), et, default_node=-1, call_id=20)
        assert np.array_equal(t2n(walk), OG.random_walk(31, 20, q, et, L, 1.0, 1.0, -1))
        assert np.array_equal(
            t2n(walk), t2n(G.random_walk(torch.as_tensor(q).cuda(), et, 1.0, 1.0, -1,
                                         call_id=20)))
        # node2vec through the sampler: rows fetched step by step, the draw on explicit
        # lists (euler_gpu_node2vec_step) == the single-GPU kernels == the oracle
        for p_, q_ in ((0.25, 4.0), (2.0, 0.5)):
            w2 = S.random_walk(torch.as_tensor(q).cuda(), et, p_, q_, default_node=-1, call_id=30)
            assert np.array_equal(t2n(w2), OG.random_walk(31, 30, q, et, L, p_, q_, -1)), (p_, q_)
            assert torch.equal(w2, G.random_walk(torch.as_tensor(q).cuda(), et, p_, q_, -1, call_id=30))
        # the ENQUEUED walk (round 6: slab levels, no host wait per step) over shapes: one walker, sizes
        # around the slab's 2 048-word chunk, walks shorter / longer than the two-pass paths' split and
        # than the 120 level pointers a launch carries, up to 16 cohorts, the hash front end, levels
        # sent as they are from step `tail`, the exchanges made with itself; unknown and duplicate starts
        import itertools
        Gw = EA.Graph.synthetic(EA.synth_params(77, 200_000, 2_400_000, weighted=True))
        Gw.set_seed(77)
        Sw = gpu_sharded_sampler(Gw, partitions=1)
        try:
            for n_w, L_w, K_w, dense, tail, split, selfx in itertools.chain(
                    [(1, 1, 1, True, 16, 10, 0), (2047, 17, 1, True, 16, 10, 0), (2048, 18, 2, False, 16, 10, 0),
                     (2049, 19, 1, True, 3, 5, 1), (5000, 130, 1, True, 16, 10, 0), (5000, 130, 3, False, 0, 100, 0),
                     (70000, 40, 16, True, 16, 10, 1), (3, 40, 2, False, 1, 1, 0), (100000, 26, 1, False, 16, 17, 1)],
                    [(int(rng.integers(1, 30000)), int(rng.integers(0, 60)), int(rng.integers(1, 5)),
                      bool(rng.integers(0, 2)), int(rng.integers(0, 30)), int(rng.integers(0, 30)),
                      int(rng.integers(0, 2))) for _ in range(12)]):
                for key, v in ((63, 1), (66, tail), (67, split), (52, selfx)):
                    _lib.check(_lib.lib().euler_gpu_set_tuning(key, v))
                st_w = rng.integers(1, 200_001, n_w).astype(np.int64)
                if n_w > 4:
                    st_w[1] = st_w[0]; st_w[2] = 0; st_w[3] = 200_005
                st_t = torch.as_tensor(st_w).cuda()
                want_w = Gw.random_walk(st_t, [[0]] * L_w, 1.0, 1.0, 200_001, call_id=11) if L_w else st_t.reshape(-1, 1)
                got_w = c_sharded_random_walk(Gw, Sw.c_transport, st_t, [[0]] * L_w, 200_001, 11, 1, K_w,
                                              Sw.dense_table if dense else None)
                assert torch.equal(got_w.reshape(want_w.shape), want_w), (n_w, L_w, K_w, dense, tail, split, selfx)
        finally:
            for key, v in ((66, 16), (67, 10), (52, 0)):
                _lib.lib().euler_gpu_set_tuning(key, v)
    finally:
        dist.destroy_process_group()


def test_dense_feature_vs_goldens_and_oracle(EA, O, torch_cuda, fixture_csr, random_csr):
    """get_dense_feature on device == the reference's rows (features.npz) for
    the fixture and the random graph, through from_csr and through the .dat
    loader; plus a 100-dimension uniform table (the fixed-stride fast path)."""
    torch = torch_cuda
    fg = np.load(os.path.join(ROOT, "tests", "golden", "features.npz"))
    for prefix, csr in (("fx_", fixture_csr), ("rg_", random_csr)):
        feats = (int(fg[prefix + "n_float"]), fg[prefix + "feat_ptr"],
                 fg[prefix + "feat_idx"], fg[prefix + "feat_val"])
        G = EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr,
                              csr.prefix_w, csr.type_prefix, csr.n_types,
                              csr.node_type, csr.node_weight, features=feats)
        assert G.num_float_features == feats[0]
        got = G.get_dense_feature(torch.as_tensor(fg[prefix + "query"]).cuda(),
                                  fg[prefix + "fids"].tolist(), fg[prefix + "dims"].tolist())
        for k, o in enumerate(got):
            assert np.array_equal(t2n(o), fg[prefix + "dense_%d" % k]), (prefix, k)
    G = EA.Graph.load(os.path.join(ROOT, "tests", "golden", "fixture_dat"))
    got = G.get_dense_feature(torch.as_tensor(fg["fx_query"]).cuda(),
                              fg["fx_fids"].tolist(), fg["fx_dims"].tolist())
    for k, o in enumerate(got):
        assert np.array_equal(t2n(o), fg["fx_dense_%d" % k])
    # uniform table: 5000 nodes x (100 + 28) floats
    rng = np.random.default_rng(3)
    n = 5000
    ids = np.arange(10, 10 + n).astype(np.uint64)
    seg = np.arange(n + 1, dtype=np.int64)
    csr = O.csr_from_raw(ids, seg, rng.choice(ids, n), np.ones(n, np.float32), 1)
    val = rng.standard_normal((n, 128)).astype(np.float32)
    F = O.DenseFeatures(2, np.arange(n + 1) * 128, np.tile([100, 128], n), val.reshape(-1))
    G = gpu_graph(EA, csr, features=(2, F.feat_ptr, F.feat_idx, F.feat_val))
    q = np.concatenate([rng.choice(ids, 20000), [0, 3]]).astype(np.int64)
    want = O.OracleGraph(csr).get_dense_feature(F, q, [0, 1], [100, 32])
    got = G.get_dense_feature(torch.as_tensor(q).cuda(), [0, 1], [100, 32])
    assert np.array_equal(t2n(got[0]), want[0]) and np.array_equal(t2n(got[1]), want[1])
    assert np.array_equal(want[0][:-2], val[(q[:-2] - 10), :100])


def test_sample_fanout_with_feature(EA, O, torch_cuda):
    """TF SampleFanoutWithFeature (sample_fanout_with_feature_op.cc:135-233) as one
    enqueue (euler_gpu_sample_fanout_with_feature): neighbours / weights / types == the
    oracle's fanout, dense_features[layer * F + j] == the oracle's get_dense_feature of that
    layer's nodes (roots first) - zero rows for default_node, unknown ids and missing
    slots; the operator-surface wrapper (euler_ops.sample_fanout_with_feature) adds the
    sparse features per layer."""
    torch = torch_cuda
    rng = np.random.default_rng(11)
    n = 3000
    ids = np.arange(5, 5 + n).astype(np.uint64)
    deg = rng.integers(0, 12, n)
    seg = np.zeros(n + 1, np.int64)
    seg[1:] = np.cumsum(deg)
    E = int(seg[-1])
    nbr = rng.choice(ids, E).astype(np.uint64)
    nbr[rng.random(E) < 0.03] = 10 ** 9          # no such node
    w = (rng.random(E) * 3 + 0.5).astype(np.float32)
    csr = O.csr_from_raw(ids, seg, nbr, w, 1)
    # two float slots: 6 values, then 3 (some rows leave the second empty)
    per = [[list(np.float32(rng.standard_normal(6))),
            list(np.float32(rng.standard_normal(3))) if i % 4 else []] for i in range(n)]
    F = O.DenseFeatures.from_lists(per)
    G = gpu_graph(EA, csr, features=(F.n_float, F.feat_ptr, F.feat_idx, F.feat_val))
    OG = O.OracleGraph(csr)
    q = np.concatenate([rng.choice(ids, 700), [0, 3, 10 ** 9]]).astype(np.int64)
    qt = torch.as_tensor(q).cuda()
    G.set_seed(5)
    for counts in ([4, 3], [5], [2, 2, 2]):
        et = [[0]] * len(counts)
        nb, ww, tt, dense = G.sample_fanout_with_feature(qt, et, counts, -1, [0, 1], [6, 3],
                                                         call_id=17)
        on, ow, ot = OG.sample_fanout(5, 17, q, et, counts, -1)
        assert len(dense) == (len(counts) + 1) * 2
        layer_nodes = [q] + [np.asarray(x) for x in on]
        for h in range(len(counts)):
            assert np.array_equal(t2n(nb[h + 1]), on[h]) and np.array_equal(t2n(ww[h]), ow[h])
            assert np.array_equal(t2n(tt[h]), ot[h])
        for layer, nodes_l in enumerate(layer_nodes):
            want = OG.get_dense_feature(F, nodes_l, [0, 1], [6, 3])
            for j in range(2):
                got = t2n(dense[layer * 2 + j])
                assert got.shape == (len(nodes_l), [6, 3][j])
                assert np.array_equal(got, want[j]), (counts, layer, j)
                # default_node / unknown ids: zero rows
                bad = ~np.isin(nodes_l.astype(np.uint64), ids)
                assert not got[bad].any()
    # the operator surface (tf_euler/python/euler_ops/neighbor_ops.py:49-70)
    from euler_amd import euler_ops
    from euler_amd.euler_ops import base as _base
    prev = _base._default
    _base.set_default_graph(G)
    try:
        G.set_seed(5, 40)
        nb, ww, tt, dense, sparse = euler_ops.sample_fanout_with_feature(
            qt, [[0], [0]], [4, 3], -1, ["0", "1"], [6, 3])
        on, _, _ = OG.sample_fanout(5, 40, q, [[0], [0]], [4, 3], -1)
        assert np.array_equal(t2n(nb[1]), on[0]) and np.array_equal(t2n(nb[2]), on[1])
        assert len(dense) == 6 and sparse == []
        want = OG.get_dense_feature(F, np.asarray(on[1]), [0, 1], [6, 3])
        assert np.array_equal(t2n(dense[4]), want[0]) and np.array_equal(t2n(dense[5]), want[1])
    finally:
        _base._default = prev


def test_sorted_and_top_k_neighbors(EA, O, torch_cuda, fixture_csr, big_pair):
    """get_sorted_full_neighbor / get_top_k_neighbor / order_by+limit on device
    == the reference tests' expectations on the fixture and == the oracle on a
    20 000-node heterogeneous graph (ties included: both keep storage order)."""
    torch = torch_cuda
    G = gpu_graph(EA, fixture_csr)
    idx, ids, w, t = G.get_sorted_full_neighbor(torch.tensor([1, 2]).cuda(), [0, 1])
    assert t2n(idx).tolist() == [[0, 3], [3, 5]] and t2n(ids).tolist() == [2, 3, 4, 3, 5]
    assert t2n(t).tolist() == [0, 1, 0, 1, 1]
    di, dw, dt = G.get_top_k_neighbor(torch.tensor([1, 2]).cuda(), [0, 1], 2)
    assert t2n(di).tolist() == [[4, 3], [5, 3]] and t2n(dt).tolist() == [[0, 1], [1, 1]]
    assert t2n(dw).tolist() == [[4.0, 3.0], [5.0, 3.0]]
    G, OG, node_ids, rng = big_pair
    q = np.concatenate([rng.choice(node_ids, 3000), [0, 11]]).astype(np.uint64)
    qt = torch.as_tensor(q.astype(np.int64)).cuda()
    for et in ([0, 1, 2, 3], [2], [3, 1]):
        full = OG.get_full_neighbor(q, et)
        for order_by, desc, limit in (("id", False, None), ("weight", True, 4),
                                      ("id", True, 2), ("weight", False, None),
                                      (None, False, 3)):
            want = O.neighbor_post_process(*full, order_by=order_by, desc=desc, limit=limit)
            got = G.get_full_neighbor(qt, et, order_by=order_by, desc=desc, limit=limit)
            assert np.array_equal(t2n(got[0]), want[0]), (et, order_by, desc, limit)
            assert np.array_equal(t2n(got[1]).astype(np.uint64), want[1])
            assert np.array_equal(t2n(got[2]), want[2])
            assert np.array_equal(t2n(got[3]), want[3])
        want = O.neighbor_to_dense(*O.neighbor_post_process(*full, order_by="weight",
                                                            desc=True, limit=6), 6, -9)
        got = G.get_top_k_neighbor(qt, et, 6, default_node=-9)
        for x, y in zip(got, want):
            assert np.array_equal(t2n(x), y)
    # rows longer than a wave (k rounds of selection), heavy ties, k > row length
    n_l = 400
    l_ids = np.arange(1, n_l + 1).astype(np.uint64)
    l_deg = rng.integers(0, 700, size=(n_l, 2))
    l_deg[rng.random((n_l, 2)) < 0.2] = 0
    l_seg = np.zeros(2 * n_l + 1, np.int64)
    l_seg[1:] = np.cumsum(l_deg.reshape(-1))
    l_nbr = rng.choice(l_ids, int(l_seg[-1])).astype(np.uint64)
    l_w = rng.integers(1, 6, int(l_seg[-1])).astype(np.float32)      # 5 distinct weights: ties
    l_csr = O.csr_from_raw(l_ids, l_seg, l_nbr, l_w, 2)
    GL, OL = gpu_graph(EA, l_csr), O.OracleGraph(l_csr)
    ql = np.concatenate([l_ids, [0, 999]]).astype(np.uint64)
    for et, k in (([0, 1], 7), ([1], 3), ([1, 0], 70), ([0], 1)):
        full = OL.get_full_neighbor(ql, et)
        want = O.neighbor_to_dense(*O.neighbor_post_process(*full, order_by="weight",
                                                            desc=True, limit=k), k, -3)
        got = GL.get_top_k_neighbor(torch.as_tensor(ql.astype(np.int64)).cuda(), et, k,
                                    default_node=-3)
        for x, y in zip(got, want):
            assert np.array_equal(t2n(x), y), (et, k)


def test_sage_dataflow_blocks(EA, O, torch_cuda, big_pair):
    """SageDataFlow on device == the same composition on the oracle
    (sample_neighbor of the unique frontier, tf.unique = first-occurrence
    ID_UNIQUE, edge_index / res_n_id arithmetic of neighbor_dataflow.py:84-110)."""
    torch = torch_cuda
    G, OG, ids, rng = big_pair
    roots = rng.choice(ids, 64).astype(np.int64)
    fanouts, metapath, max_id = [4, 3], [[0, 1], [2]], 10 ** 13
    G.set_seed(77, call_id=500)
    flow = EA.dataflow.SageDataFlow(G, fanouts, metapath, add_self_loops=True, max_id=max_id)
    df = flow(torch.as_tensor(roots).cuda())

    def uniq(a):
        uq, gi = O.id_unique(a.astype(np.uint64))
        return uq.astype(np.int64), gi.astype(np.int64)

    # oracle composition (call ids 500, 501 in get_neighbors)
    n_id = roots.copy()
    nbrs, srcs = [], []
    for h, (et, c) in enumerate(zip(metapath, fanouts)):
        nb, _, _ = OG.sample_neighbor(77, 500 + h, n_id, et, c, max_id + 1)
        nbrs.append(nb.reshape(-1))
        srcs.append(np.repeat(np.arange(len(n_id)), c))
        n_id, _ = uniq(np.concatenate([nb.reshape(-1), n_id]))
    n_id = roots.copy()
    last_idx = np.arange(len(n_id))
    want = []
    for i in range(2):
        new_n_id, inv = uniq(np.concatenate([nbrs[i], n_id]))
        res = inv[-len(n_id):]
        src = np.concatenate([srcs[i], last_idx])
        last_idx = np.arange(len(new_n_id))
        want.append((new_n_id, res, np.stack([src, inv]), [len(n_id), len(new_n_id)]))
        n_id = new_n_id
    assert len(df) == 2
    for blk, (wn, wr, we, ws) in zip(df.blocks, want):
        assert np.array_equal(t2n(blk.n_id), wn)
        assert np.array_equal(t2n(blk.res_n_id), wr)
        assert np.array_equal(t2n(blk.edge_index), we)
        assert blk.size == ws
    assert [b.size for b in df] == [w[3] for w in want][::-1]


def test_sage_blocks_fused_flow(EA, O, torch_cuda, big_pair):
    """Round 6: a Sage flow whose hops list ONE edge type runs as three launches per hop (sampler +
    insert in one kernel, flag, emit + index; the hash tables cleared by the kernels before them;
    tuning key 60) - the blocks must equal the oracle composition and the op-by-op flow's (key 60
    = 0): hashed ids, unknown roots, duplicate roots, default fills (ids without a row go through
    the hash table), self loops on and off, a plain graph at a size where chunks and tables span
    many workgroups."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    G, OG, ids, rng = big_pair

    def uniq(a):
        uq, gi = O.id_unique(a.astype(np.uint64))
        return uq.astype(np.int64), gi.astype(np.int64)

    try:
        roots = np.concatenate([rng.choice(ids, 300), [0, 10 ** 13 + 5], rng.choice(ids, 20)]).astype(np.int64)
        roots[5] = roots[6]
        fanouts, metapath, max_id = [5, 4], [[0], [2]], 10 ** 13
        for fused in (1, 2, 0):                 # 2: fused, ids with a row through the hop's own table (key 62)
            _lib.check(L.euler_gpu_set_tuning(60, min(fused, 1)))
            _lib.check(L.euler_gpu_set_tuning(62, 1 if fused == 2 else 0))
            for loops in (True, False):
                G.set_seed(79, call_id=700)
                df = EA.dataflow.SageDataFlow(G, fanouts, metapath, add_self_loops=loops, max_id=max_id)(
                    torch.as_tensor(roots).cuda())
                n_id = roots.copy()
                last_idx = np.arange(len(n_id))
                want = []
                for h, (et, c) in enumerate(zip(metapath, fanouts)):
                    nb, _, _ = OG.sample_neighbor(79, 700 + h, n_id, et, c, max_id + 1)
                    new_n_id, inv = uniq(np.concatenate([nb.reshape(-1), n_id]))
                    src = np.repeat(np.arange(len(n_id)), c)
                    res = inv[-len(n_id):]
                    e = np.stack([np.concatenate([src, last_idx]), inv]) if loops else np.stack([src, inv[:len(src)]])
                    last_idx = np.arange(len(new_n_id))
                    want.append((new_n_id, res, e))
                    n_id = new_n_id
                for blk, (wn, wr, we) in zip(df.blocks, want):
                    assert np.array_equal(t2n(blk.n_id), wn), (fused, loops)
                    assert np.array_equal(t2n(blk.res_n_id), wr), (fused, loops)
                    assert np.array_equal(t2n(blk.edge_index), we), (fused, loops)
        # a plain weighted graph, 20 000 roots x [25, 10]: fused == op by op, every array
        p = EA.synth_params(4242, 300000, 3000000, n_types=1, weighted=True)
        Gs = EA.Graph.synthetic(p)
        r = torch.as_tensor(np.concatenate([np.random.default_rng(4).integers(1, 300001, 20000), [0, 300001, 7, 7]])).cuda()
        outs = []
        for fused in (1, 0, 2):
            _lib.check(L.euler_gpu_set_tuning(60, min(fused, 1)))
            _lib.check(L.euler_gpu_set_tuning(62, 1 if fused == 2 else 0))
            Gs.set_seed(5, call_id=40)
            df = EA.dataflow.SageDataFlow(Gs, [25, 10], [[0], [0]], add_self_loops=True, max_id=300000)(r)
            outs.append([(t2n(b.n_id), t2n(b.res_n_id), t2n(b.edge_index)) for b in df.blocks])
        for a, b in ((outs[0], outs[1]), (outs[0], outs[2])):
            for x, y in zip(a, b):
                assert all(np.array_equal(u, v) for u, v in zip(x, y))
        assert max(len(x[0]) for x in outs[0]) > 50000
    finally:
        L.euler_gpu_set_tuning(60, 1)
        L.euler_gpu_set_tuning(62, 2)


def test_sage_blocks_two_host_threads_one_stream(EA, torch_cuda):
    """Two host threads building blocks on the SAME stream (the null stream; ctypes releases the
    GIL inside the C call): the stream's row-indexed first-occurrence table is shared, so a call's
    hops must be enqueued as one run (g->launch_mu) - every block equals the one a single thread
    builds (B's Insert with a newer epoch used to slip between A's Insert and Flag)."""
    import threading
    torch = torch_cuda
    N = 200_000
    G = EA.Graph.synthetic(EA.synth_params(9, N, 12 * N, weighted=True))
    G.set_seed(3)
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    batches = [torch.randint(1, N + 1, (6000,), generator=gen, device="cuda", dtype=torch.int64) for _ in range(2)]
    fan, mp_ = [6, 4], [[0], [0]]

    def blocks(t, it):
        return G.sage_blocks(batches[t], mp_, fan, default_node=N + 1, call_id=1000 + 10 * t + 2 * (it % 3))
    want = [[blocks(t, it) for it in range(3)] for t in range(2)]
    torch.cuda.synchronize()
    errs = []

    def work(t):
        try:
            for it in range(60):
                got = blocks(t, it)
                for (b1, _c1), (b2, _c2) in ((got, want[t][it % 3]),):
                    for x, y in zip(b1, b2):
                        for u, v in zip(x, y):
                            if u is not None and not torch.equal(u, v):
                                errs.append((t, it))
                                return
        except Exception as e:          # noqa: BLE001
            errs.append((t, repr(e)))
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs


def test_sage_blocks_multi_equals_separate_calls(EA, O, torch_cuda, big_pair):
    """euler_gpu_sage_blocks_multi: M minibatches' SageDataFlows in ONE enqueue (every kernel of the
    flow with the minibatch as second grid dimension, the hops' samplers one launch with minibatch
    b's own call id) == M separate sage_blocks calls with the call ids consecutive calls take, bit
    for bit: identity and hashed id maps, weighted and uniform weights, unknown / duplicate roots,
    default fills that are no node (-1: the all-ones id's side slot), with and without self loops,
    three hops, minibatch counts around the launch geometry; hops with type draws go through the
    separate calls inside the same entry; SageDataFlow.produce_subgraphs == the loop."""
    torch = torch_cuda
    N = 200_000
    gen = torch.Generator(device="cuda"); gen.manual_seed(31)

    def check(G, roots, mp_, fan, dflt, loops):
        M = roots.shape[0]
        layers = len(fan)
        G.set_seed(17)
        got = G.sage_blocks_multi(roots, mp_, fan, default_node=dflt, add_self_loops=loops, call_id=400)
        assert len(got) == M
        for b in range(M):
            want = G.sage_blocks(roots[b], mp_, fan, default_node=dflt, add_self_loops=loops,
                                 call_id=400 + b * layers)
            assert list(got[b][1]) == list(want[1]), (b, got[b][1], want[1])
            for x, y in zip(got[b][0], want[0]):
                for u, v in zip(x, y):
                    assert torch.equal(u, v), b
        # ... and the launches of round 5 (sampler, insert as separate kernels: tuning key 60 = 0)
        from euler_amd import _lib
        try:
            _lib.check(_lib.lib().euler_gpu_set_tuning(60, 0))
            G.set_seed(17)
            old = G.sage_blocks_multi(roots, mp_, fan, default_node=dflt, add_self_loops=loops, call_id=400)
        finally:
            _lib.lib().euler_gpu_set_tuning(60, 1)
        for b in range(M):
            assert list(got[b][1]) == list(old[b][1])
            for x, y in zip(got[b][0], old[b][0]):
                for u, v in zip(x, y):
                    assert torch.equal(u, v), b
        return got

    for weighted in (True, False):
        G = EA.Graph.synthetic(EA.synth_params(5, N, 8 * N, weighted=weighted))
        for M, n, fan, dflt, loops in ((64, 300, [5, 4], N + 1, True), (3, 2000, [25, 10], -1, True),
                                       (130, 17, [3, 2, 2], N + 9, False), (1, 500, [4, 4], N + 1, True)):
            r = torch.randint(1, N + 1, (M, n), generator=gen, device="cuda", dtype=torch.int64)
            r[:, ::13] = N + 3                    # ids without a row
            r[:, 5::29] = 0
            r[:, 1::7] = r[:, :1]                  # duplicates inside a minibatch
            if M > 1:
                r[1] = r[0]                        # ... and two identical minibatches (own call ids: other draws)
            got = check(G, r, [[0]] * len(fan), fan, dflt, loops)
            if M > 1 and weighted:
                assert not torch.equal(got[0][0][0][0], got[1][0][0][0]) or n < 50
    GH, _OG, ids, rng = big_pair                   # hashed ids, 4 edge types
    roots = torch.as_tensor(rng.choice(ids, (20, 150)).astype(np.int64)).cuda()
    roots[:, ::11] = 4242
    check(GH, roots, [[2], [0]], [4, 3], 10 ** 13 + 1, True)          # one listed type per hop: one enqueue
    check(GH, roots, [[0, 1], [2, 3]], [4, 3], 10 ** 13 + 1, True)    # type draws: the separate calls
    # the flow class: the list form == the loop
    G = EA.Graph.synthetic(EA.synth_params(6, N, 8 * N, weighted=True))
    r = torch.randint(1, N + 1, (9, 256), generator=gen, device="cuda", dtype=torch.int64)
    f = EA.dataflow.SageDataFlow(G, [6, 4], [[0], [0]], add_self_loops=True, max_id=N)
    G.set_seed(3, 70)
    flows = f.produce_subgraphs(r)
    G.set_seed(3, 70)
    loop = [f.produce_subgraph(r[b]) for b in range(9)]
    for a, b_ in zip(flows, loop):
        for x, y in zip(a.blocks, b_.blocks):
            assert torch.equal(x.n_id, y.n_id) and torch.equal(x.res_n_id, y.res_n_id)
            assert torch.equal(x.edge_index, y.edge_index) and x.size == y.size
    # minibatches of different lengths take the loop
    assert len(f.produce_subgraphs([r[0], r[1][:100]])) == 2


def test_gcn_and_relation_dataflow_blocks(EA, O, torch_cuda, big_pair):
    """GCNDataFlow / RelationDataFlow (RGCN, config 5) on device == the same
    composition on the oracle: full neighbours of the unique frontier per hop
    (gcn_dataflow.py:33-47, relation_dataflow.py:30-72), tf.unique =
    first-occurrence ID_UNIQUE, edge types as e_id."""
    torch = torch_cuda
    G, OG, ids, rng = big_pair
    roots = np.concatenate([rng.choice(ids, 48), [0, 4242]]).astype(np.int64)
    metapath = [[0, 1], [2, 3]]

    def uniq(a):
        uq, gi = O.id_unique(a.astype(np.uint64))
        return uq.astype(np.int64), gi.astype(np.int64)

    n_id = roots.copy()
    nbrs, srcs, typs = [], [], []
    for et in metapath:
        idx, nb, _w, t = OG.get_full_neighbor(n_id.astype(np.uint64), et)
        lens = idx[:, 1] - idx[:, 0]
        nbrs.append(nb.astype(np.int64)); typs.append(t)
        srcs.append(np.repeat(np.arange(len(n_id)), lens))
        n_id, _ = uniq(np.concatenate([nb.astype(np.int64), n_id]))
    rt = torch.as_tensor(roots).cuda()
    # RelationDataFlow: no self loops, e_id = edge types
    df = EA.dataflow.RelationDataFlow(G, metapath)(rt)
    n_id = roots.copy()
    for i, blk in enumerate(df.blocks):
        new_n_id, inv = uniq(np.concatenate([nbrs[i], n_id]))
        assert np.array_equal(t2n(blk.n_id), new_n_id)
        assert np.array_equal(t2n(blk.res_n_id), inv[len(inv) - len(n_id):])
        assert np.array_equal(t2n(blk.edge_index), np.stack([srcs[i], inv[:len(inv) - len(n_id)]]))
        assert np.array_equal(t2n(blk.e_id), typs[i])
        assert blk.size == [len(n_id), len(new_n_id)]
        n_id = new_n_id
    # GCNDataFlow: the UniqueDataFlow arithmetic with self loops
    df = EA.dataflow.GCNDataFlow(G, metapath, add_self_loops=True)(rt)
    n_id = roots.copy()
    last_idx = np.arange(len(n_id))
    for i, blk in enumerate(df.blocks):
        new_n_id, inv = uniq(np.concatenate([nbrs[i], n_id]))
        src = np.concatenate([srcs[i], last_idx])
        last_idx = np.arange(len(new_n_id))
        assert np.array_equal(t2n(blk.n_id), new_n_id)
        assert np.array_equal(t2n(blk.res_n_id), inv[len(inv) - len(n_id):])
        assert np.array_equal(t2n(blk.edge_index), np.stack([src, inv]))
        n_id = new_n_id


def test_full_neighbour_flows_one_enqueue(EA, O, torch_cuda, big_pair):
    """euler_gpu_full_blocks (GCNDataFlow / RelationDataFlow without a host round trip per
    hop): the blocks equal the op-by-op composition of the base classes (itself checked
    against the oracle above) - with and without self loops, three hops, duplicate and
    unknown roots; a capacity that is too small is reported (no blocks), the flow then
    falls back and raises its estimate so that the next minibatch fits."""
    torch = torch_cuda
    G, _OG, ids, rng = big_pair
    roots = np.concatenate([rng.choice(ids, 300), rng.choice(ids, 20).repeat(3), [0, 4242]])
    rt = torch.as_tensor(roots.astype(np.int64)).cuda()

    def same(df_a, df_b, with_types):
        assert len(df_a.blocks) == len(df_b.blocks)
        for a, b in zip(df_a.blocks, df_b.blocks):
            assert torch.equal(a.n_id, b.n_id) and torch.equal(a.res_n_id, b.res_n_id)
            assert torch.equal(a.edge_index, b.edge_index) and a.size == b.size
            if with_types:
                assert torch.equal(a.e_id.to(torch.int64), b.e_id.to(torch.int64))

    for metapath in ([[0, 1], [2, 3]], [[3], [0], [1]], [[0, 1, 2, 3]]):
        for loops in (True, False):
            f1 = EA.dataflow.GCNDataFlow(G, metapath, add_self_loops=loops)
            f2 = EA.dataflow.GCNDataFlow(G, metapath, add_self_loops=loops)
            f2.fused = False
            same(f1(rt), f2(rt), False)
        r1 = EA.dataflow.RelationDataFlow(G, metapath)
        r2 = EA.dataflow.RelationDataFlow(G, metapath)
        r2.fused = False
        same(r1(rt), r2(rt), True)
    # capacity too small: reported, the flow falls back and learns
    blocks, cnt = G.full_blocks(rt, [[0, 1, 2, 3], [0, 1, 2, 3]], [10, 10], True, False)
    assert blocks is None and cnt[-1] == 1
    f = EA.dataflow.GCNDataFlow(G, [[0, 1, 2, 3], [0, 1, 2, 3]])
    f._growth = [0.01, 0.01]
    ref = EA.dataflow.GCNDataFlow(G, [[0, 1, 2, 3], [0, 1, 2, 3]])
    ref.fused = False
    same(f(rt), ref(rt), False)              # overflowed -> op by op
    assert min(f._growth) > 0.01
    same(f(rt), ref(rt), False)
    same(f(rt), ref(rt), False)              # by now the capacities fit
    blocks, cnt = G.full_blocks(rt, [[0, 1, 2, 3], [0, 1, 2, 3]], f._edge_caps(rt.numel()), True, False)
    assert blocks is not None


def test_dedup_split_pack_expand(EA, O, torch_cuda):
    """Fused front / back end of a multi-GPU hop: every position finds its id in
    the bucketed distinct list, buckets hold the ids their shard owns
    (id_split_op.cc:46-49), duplicates collapse (almost all: unresolved hash
    collisions may leave a few), and pack -> expand_packed returns each
    position its row."""
    torch = torch_cuda
    rng = np.random.default_rng(12)
    pool = np.concatenate([rng.integers(1, 2 ** 62, 5000), [0, 2 ** 63 + 9]]).astype(np.uint64)
    ids = rng.choice(pool, 200_000)
    mask = (rng.random(200_000 // 10) < 0.05).astype(np.uint8)
    eff = ids.copy()
    eff[np.repeat(mask, 10).astype(bool)] = 0
    it = torch.as_tensor(ids.astype(np.int64)).cuda()
    for parts, shards in ((8, 8), (1024, 3), (5, 1)):
        off, sid, pos = EA.ops.dedup_split(it, parts, shards, torch.as_tensor(mask).cuda(), 10)
        sid_n, pos_n = t2n(sid).astype(np.uint64), t2n(pos)
        assert off[0] == 0 and off[-1] == len(sid_n) <= len(ids)
        assert np.array_equal(sid_n[pos_n], eff)
        assert set(sid_n.tolist()) == set(eff.tolist())
        assert len(sid_n) < 1.05 * len(set(eff.tolist()))
        own = O.shard_of(sid_n, parts, shards)
        for s in range(shards):
            assert np.all(own[off[s]:off[s + 1]] == s)
    # wire format round trip
    m, count = len(sid_n), 6
    r_id = torch.as_tensor(rng.integers(-2 ** 62, 2 ** 62, (m, count))).cuda()
    r_w = torch.as_tensor(rng.random((m, count)).astype(np.float32)).cuda()
    r_t = torch.as_tensor(rng.integers(-1, 9, (m, count)).astype(np.int32)).cuda()
    r_m = torch.as_tensor((rng.random(m) < 0.3).astype(np.uint8)).cuda()
    packed = EA.ops.pack_rows(r_id, r_w, r_t, r_m, count)
    assert tuple(packed.shape) == (m, 4 * count + 2)
    o_id, o_w, o_t, o_m = EA.ops.expand_packed(pos, packed, count)
    assert np.array_equal(t2n(o_id), t2n(r_id)[pos_n])
    assert np.array_equal(t2n(o_w), t2n(r_w)[pos_n])
    assert np.array_equal(t2n(o_t), t2n(r_t)[pos_n])
    assert np.array_equal(t2n(o_m), t2n(r_m)[pos_n])
    # single-type calls: no type column on the wire, types rebuilt from the mask
    for cnt1 in (6, 5, 4, 2):          # even counts: the lean expansion; odd: the general kernel
        r_id1 = r_id[:, :cnt1].contiguous(); r_w1 = r_w[:, :cnt1].contiguous()
        packed1 = EA.ops.pack_rows(r_id1, r_w1, r_t[:, :cnt1].contiguous(), r_m, cnt1, single_type=3)
        assert tuple(packed1.shape) == (m, (3 * cnt1 + 3) & ~1)
        s_id, s_w, s_t, s_m = EA.ops.expand_packed(pos, packed1, cnt1, single_type=3)
        assert np.array_equal(t2n(s_id), t2n(r_id1)[pos_n])
        assert np.array_equal(t2n(s_w), t2n(r_w1)[pos_n])
        assert np.array_equal(t2n(s_m), t2n(r_m)[pos_n])
        assert np.array_equal(t2n(s_t), np.where(t2n(r_m)[pos_n][:, None] != 0, -1, 3)
                              * np.ones((1, cnt1), np.int32))
        # an odd number of positions, a handful of positions
        for cut in (1, 199_997):
            po = pos[:len(pos_n) - cut].contiguous()
            o_id2, o_w2, o_t2, o_m2 = EA.ops.expand_packed(po, packed1, cnt1, single_type=3)
            assert np.array_equal(t2n(o_id2), t2n(s_id)[:len(pos_n) - cut]) and np.array_equal(t2n(o_w2), t2n(s_w)[:len(pos_n) - cut])
            assert np.array_equal(t2n(o_t2), t2n(s_t)[:len(pos_n) - cut]) and np.array_equal(t2n(o_m2), t2n(s_m)[:len(pos_n) - cut])
    e_id, e_w, e_t, e_m = EA.ops.expand_rows(pos, r_id, r_w, r_t, r_m, count)
    assert np.array_equal(t2n(e_id), t2n(o_id)) and np.array_equal(t2n(e_m), t2n(o_m))


def test_dedup_split_dense_id_table(EA, O, torch_cuda):
    """Front end with the id-indexed table (graphs whose ids are all below a known
    limit): exactly one copy of every distinct id below the limit; ids at or
    above it (no such node) may share a representative - every position still
    finds an id of its own class; the table is reused dirty across calls."""
    torch = torch_cuda
    rng = np.random.default_rng(13)
    limit = 1_000_000
    table = torch.randint(-2 ** 31, 2 ** 31 - 1, (limit + 1,), dtype=torch.int32, device="cuda")
    for n, n_pool in ((200_000, 7000), (1, 1), (70_001, 70_001)):
        pool = np.concatenate([rng.integers(0, limit, n_pool),
                               [0, limit - 1, limit, limit + 5, 2 ** 63 + 9]]).astype(np.uint64)
        ids = rng.choice(pool, n)
        group = 10
        mask = (rng.random((n + group - 1) // group) < 0.05).astype(np.uint8)
        eff = ids.copy()
        eff[np.repeat(mask, group)[:n].astype(bool)] = 0
        it = torch.as_tensor(ids.astype(np.int64)).cuda()
        for parts, shards in ((8, 8), (1024, 3), (5, 1)):
            off, sid, pos = EA.ops.dedup_split(it, parts, shards, torch.as_tensor(mask).cuda(),
                                               group, dense_table=table)
            sid_n, pos_n = t2n(sid).astype(np.uint64), t2n(pos)
            assert off[0] == 0 and off[-1] == len(sid_n) <= n
            got = sid_n[pos_n]
            known = eff < limit
            assert np.array_equal(got[known], eff[known])
            assert np.all(got[~known] >= limit)
            below = sid_n[sid_n < limit]
            assert len(below) == len(set(below.tolist())) == len(set(eff[known].tolist()))
            assert (sid_n >= limit).sum() == (1 if (~known).any() else 0)
            own = O.shard_of(sid_n, parts, shards)
            for s in range(shards):
                assert np.all(own[off[s]:off[s + 1]] == s)


@pytest.mark.parametrize("ascending", [False, True], ids=["storage_order", "ascending_lists"])
@pytest.mark.parametrize("wave", [3, 2, 1, 0], ids=["n2v_stepwise", "n2v_parallel", "n2v_wave", "n2v_lane"])
def test_node2vec_long_lists_both_kernels(EA, O, torch_cuda, wave, ascending):
    """node2vec steps whose child AND parent lists span several 256-entry LDS
    chunks (hubs of 700-900 neighbours that point at each other), with two
    listed edge types: the wave-per-walker kernel and the lane-per-walker kernel
    must both reproduce the oracle's two-cursor BuildWeights walk."""
    torch = torch_cuda
    from euler_amd import _lib
    rng = np.random.default_rng(41)
    n, T = 400, 2
    ids = np.arange(1, n + 1).astype(np.uint64)
    deg = rng.integers(1, 12, size=(n, T))
    hubs = np.arange(0, 12)
    deg[hubs, :] = rng.integers(350, 450, size=(len(hubs), T))
    seg = np.zeros(n * T + 1, np.int64)
    seg[1:] = np.cumsum(deg.reshape(-1))
    E = int(seg[-1])
    nbr = rng.choice(ids, E).astype(np.uint64)
    # hubs mostly point at hubs, so walks keep meeting long parent lists
    for h in hubs:
        for t in range(T):
            b, e = seg[h * T + t], seg[h * T + t + 1]
            nbr[b:e] = np.where(rng.random(e - b) < 0.7, rng.choice(ids[hubs], e - b),
                                nbr[b:e])
    w = (rng.random(E) * 3 + 0.1).astype(np.float32)
    w[rng.random(E) < 0.05] = 0
    if ascending:
        # neighbour lists sorted by id inside every (node, type) segment: every child is
        # an event for the parallel kernel, which hands such steps to the lane-0 automaton
        for x in range(n * T):
            b, e = seg[x], seg[x + 1]
            o = np.argsort(nbr[b:e], kind="stable")
            nbr[b:e], w[b:e] = nbr[b:e][o], w[b:e][o]
    csr = O.csr_from_raw(ids, seg, nbr, w, T)
    G, OG = gpu_graph(EA, csr), O.OracleGraph(csr)
    starts = np.concatenate([rng.choice(ids, 300), ids[hubs], [0, 999]]).astype(np.int64)
    L = 7
    et = [[0, 1], [1], [0, 1], [1, 0], [0], [0, 1], [1, 0]]
    et_arr = [e + [e[-1]] * (2 - len(e)) for e in et]      # pad to k = 2 (repeats a type)
    _lib.lib().euler_gpu_set_tuning(7, wave)
    _lib.lib().euler_gpu_set_tuning(25, 256)      # stepwise: these hubs go to the workgroup kernel
    try:
        G.set_seed(6)
        for p, q in ((0.25, 4.0), (2.0, 0.5)):
            got = t2n(G.random_walk(torch.as_tensor(starts).cuda(), et_arr, p, q, -1,
                                    call_id=50))
            want = OG.random_walk(6, 50, starts, et_arr, L, p, q, -1)
            assert np.array_equal(got, want), (p, q)
    finally:
        _lib.lib().euler_gpu_set_tuning(7, 2)
        _lib.lib().euler_gpu_set_tuning(25, 8192)


@pytest.mark.parametrize("mode", ["stepwise", "stepwise_all_big", "one_launch"])
@pytest.mark.parametrize("weights", ["random", "dyadic", "zeros", "ascending"])
def test_node2vec_hub_rows_checkpointed_sums(EA, O, torch_cuda, weights, mode):
    """node2vec on hubs of 33 000 - 300 000 neighbours.  Default (key 7 = 3): the walk
    is launched per step and these rows go to the workgroup kernel (1 024 entries per
    round, parent cursor and running sum carried across 16 waves); "stepwise_all_big"
    sends every row of 2+ entries there, "one_launch" (key 7 = 2) is one wave per
    walker.  Both keep a (running sum, parent cursor) checkpoint per 2^sh rounds and
    replay only the rounds the draw lands in; inside a round the f32 running sums come
    from the integer scan over the mantissa when the round stays in one binade without
    a rounding tie (n2v_kernels.h: WaveSumsVec) and from the add chain
    otherwise.  Dyadic weights (multiples of 1/8) make ties and exact sums common,
    random weights make them rare, all-zero rows take RandomSelect's fall-through
    (random_walk_op.cc:83-138), ascending lists make every child move the parent
    cursor (handed to the sequential automaton)."""
    torch = torch_cuda
    from euler_amd import _lib
    rng = np.random.default_rng(77)
    n = 3000
    ids = np.arange(1, n + 1).astype(np.uint64)
    deg = rng.integers(1, 9, size=n)
    hubs = np.arange(0, 5)
    # 300 000 entries = 1 172 chunks of 256: more than the 512 checkpoint slots of the wave
    # kernel, so its checkpoints are 4 chunks apart and the second pass replays up to 4
    deg[hubs] = [41000, 300000, 33000, 52000, 36000]
    seg = np.zeros(n + 1, np.int64)
    seg[1:] = np.cumsum(deg)
    E = int(seg[-1])
    nbr = rng.choice(ids, E).astype(np.uint64)
    for h in hubs:
        b, e = seg[h], seg[h + 1]
        nbr[b:e] = np.where(rng.random(e - b) < 0.5, rng.choice(ids[hubs], e - b), nbr[b:e])
    # every small row points at a hub first
    nbr[seg[5:-1]] = rng.choice(ids[hubs], n - 5)
    if weights in ("random", "ascending"):
        w = (rng.random(E) * 7.5 + 0.5).astype(np.float32)
    elif weights == "dyadic":
        w = (rng.integers(1, 64, E) / 8.0).astype(np.float32)
    else:
        w = (rng.random(E) * 2).astype(np.float32)
        w[seg[1]:seg[2]] = 0            # one hub row of zero weights
        w[rng.random(E) < 0.3] = 0
    if weights == "ascending":
        for x in range(n):
            b, e = seg[x], seg[x + 1]
            o = np.argsort(nbr[b:e], kind="stable")
            nbr[b:e], w[b:e] = nbr[b:e][o], w[b:e][o]
    csr = O.csr_from_raw(ids, seg, nbr, w, 1)
    G, OG = gpu_graph(EA, csr), O.OracleGraph(csr)
    starts = np.concatenate([ids[hubs], rng.choice(ids, 200), [2, 2, 0]]).astype(np.int64)
    L = 5
    et = [[0]] * L
    G.set_seed(9)
    _lib.lib().euler_gpu_set_tuning(7, 2 if mode == "one_launch" else 3)
    _lib.lib().euler_gpu_set_tuning(25, 2 if mode == "stepwise_all_big" else 8192)
    try:
        for p_, q_ in ((0.25, 4.0), (2.0, 0.5), (3.0, 0.7), (1.0, 1.0)):
            got = t2n(G.random_walk(torch.as_tensor(starts).cuda(), et, p_, q_, -1, call_id=60))
            want = OG.random_walk(9, 60, starts, et, L, p_, q_, -1)
            assert np.array_equal(got, want), (weights, mode, p_, q_)
    finally:
        _lib.lib().euler_gpu_set_tuning(7, 2)
        _lib.lib().euler_gpu_set_tuning(25, 8192)


def test_concurrent_callers_share_a_stream(EA, O, torch_cuda, big_pair):
    """The reference runs ops from an 8-thread pool (query_proxy.cc:209).  Four
    host threads call the fanout (second hop through the duplicate-root path and
    its per-stream scratch) on the same stream at once: every thread must get
    what it gets alone."""
    import threading
    torch = torch_cuda
    G, OG, ids, rng = big_pair
    G.set_seed(3)
    qs = [torch.as_tensor(rng.choice(ids[:3000], 2048).astype(np.int64)).cuda()
          for _ in range(4)]
    alone = [G.sample_fanout(q, [[0], [1]], [8, 6], -1, call_id=10 * i)
             for i, q in enumerate(qs)]
    torch.cuda.synchronize()
    got = [None] * 4
    for _ in range(3):
        def work(i):
            for _rep in range(5):
                got[i] = G.sample_fanout(qs[i], [[0], [1]], [8, 6], -1, call_id=10 * i)
        ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        torch.cuda.synchronize()
        for i in range(4):
            for h in range(2):
                assert torch.equal(got[i][0][h + 1], alone[i][0][h + 1])
                assert torch.equal(got[i][1][h], alone[i][1][h])


@pytest.mark.parametrize("base,stride", [(1, 1), (1000, 3)])
def test_fanout_hop_chaining_on_identity_id_maps(EA, O, torch_cuda, base, stride,
                                                 dedup_numbering):
    """Fanout on graphs whose ids are base + stride * row (identity id map): hop
    h's kernels enter their ids into hop h+1's owner table (tuning key 9), so
    hop h+1's duplicate detection starts at its scan.  Rows without neighbours
    (masked -> node id 0 in the next hop), ids off the stride grid and ids
    beyond the last row all go through it; results must equal the oracle's and
    be the same with the chaining switched off.  Even counts take the
    pair-per-lane kernels, odd counts the single ones; the forced mode (key 5 =
    2) makes the small first hops use the duplicate path too, so the expand
    kernel is the one that marks."""
    torch = torch_cuda
    rng = np.random.default_rng(5150 + stride)
    n, T = 30000, 2
    ids = (base + stride * np.arange(n)).astype(np.uint64)
    deg = rng.integers(0, 30, size=(n, T))
    deg[rng.random((n, T)) < 0.3] = 0
    seg = np.zeros(n * T + 1, np.int64)
    seg[1:] = np.cumsum(deg.reshape(-1))
    E = int(seg[-1])
    nbr = rng.choice(ids, E).astype(np.uint64)
    dangling = rng.random(E) < 0.03
    nbr[dangling] = nbr[dangling] + (1 if stride > 1 else stride * n + 7)   # no such node
    w = (rng.random(E) * 7.5 + 0.5).astype(np.float32)
    nt = np.zeros(n, np.int32)
    nw = np.ones(n, np.float32)
    csr = O.csr_from_raw(ids, seg, nbr, w, T, nt, nw)
    G, OG = gpu_graph(EA, csr), O.OracleGraph(csr)
    q = np.concatenate([rng.choice(ids, 4094), [0, base + stride * n + 1]]).astype(np.int64)
    qt = torch.as_tensor(q).cuda()
    from euler_amd import _lib
    L = _lib.lib()
    try:
        for forced in (1, 2):
            L.euler_gpu_set_tuning(5, forced)
            for et, counts in (([[0], [1], [0]], [8, 6, 4]), ([[1], [0]], [25, 10]),
                               ([[0], [0], [1]], [5, 3, 3])):
                on, ow, ot = OG.sample_fanout(21, 60, q, et, counts, -1)
                for fuse in (1, 0):
                    L.euler_gpu_set_tuning(9, fuse)
                    G.set_seed(21)
                    gn, gw, gt = G.sample_fanout(qt, et, counts, -1, call_id=60)
                    for h in range(len(counts)):
                        assert np.array_equal(t2n(gn[h + 1]), on[h]), (forced, counts, fuse, h)
                        assert np.array_equal(t2n(gw[h]), ow[h]), (forced, counts, fuse, h)
                        assert np.array_equal(t2n(gt[h]), ot[h]), (forced, counts, fuse, h)
    finally:
        L.euler_gpu_set_tuning(5, 1)
        L.euler_gpu_set_tuning(9, 1)


def test_fanout_paths_agree_fuzz(EA, O, torch_cuda):
    """Differential fuzz: sample_fanout (duplicate-root path, hop chaining, both
    gated passes in one launch, expansion) against the plain per-hop kernel
    (sample_neighbor on the given roots, no duplicate detection) chained by hand,
    over random graphs (identity and hashed id maps, 1-3 edge types, empty rows,
    dangling and zero ids), batch sizes and fanouts.  Rows are a function of
    (seed, call id, node id) only, so both must agree bit for bit."""
    torch = torch_cuda
    rng = np.random.default_rng(20240927)
    for trial in range(24):
        n = int(rng.integers(200, 40000))
        T = int(rng.integers(1, 4))
        identity = trial % 3 != 0
        if identity:
            base, stride = int(rng.integers(0, 50)), int(rng.integers(1, 4))
            ids = (base + stride * np.arange(n)).astype(np.uint64)
        else:
            ids = np.unique(rng.integers(1, 10 ** 9, 2 * n)).astype(np.uint64)[:n]
            n = len(ids)
        deg = rng.integers(0, int(rng.integers(2, 60)), size=(n, T))
        deg[rng.random((n, T)) < 0.25] = 0
        seg = np.zeros(n * T + 1, np.int64)
        seg[1:] = np.cumsum(deg.reshape(-1))
        E = int(seg[-1])
        nbr = rng.choice(ids, E).astype(np.uint64)
        nbr[rng.random(E) < 0.02] = 10 ** 12 + 7            # no such node
        w = (rng.random(E) * 4 + 0.25).astype(np.float32)
        csr = O.csr_from_raw(ids, seg, nbr, w, T)
        G = gpu_graph(EA, csr)
        layers = int(rng.integers(2, 4))
        counts = [int(c) for c in rng.integers(1, 9, layers)]
        # the op takes a rectangular [layers, k] tensor: one listed type per hop
        # (pivot kernels, hop chaining) or all of them (type draws, reference loop)
        if rng.random() < 0.7:
            et = [[int(rng.integers(0, T))] for _ in range(layers)]
        else:
            et = [list(range(T)) for _ in range(layers)]
        B = int(rng.integers(1, 6000))
        q = np.concatenate([rng.choice(ids, B), [0]]).astype(np.int64)
        qt = torch.as_tensor(q).cuda()
        G.set_seed(1000 + trial)
        from euler_amd import _lib
        # every other trial: the duplicate path for every hop past the first,
        # whatever its size
        _lib.lib().euler_gpu_set_tuning(5, 2 if trial % 2 else 1)
        try:
            gn, gw, gt = G.sample_fanout(qt, et, counts, -1, call_id=5)
        finally:
            _lib.lib().euler_gpu_set_tuning(5, 1)
        cur, mask, group = qt, None, 1
        for h in range(layers):
            # hop h by hand: masked rows of the previous hop sample as node id 0
            roots_h = cur.clone()
            if mask is not None:
                roots_h[mask.to(torch.bool).repeat_interleave(group)] = 0
            ids_h, w_h, t_h, m_h = G.sample_neighbor(roots_h, et[h], counts[h], -1, call_id=5 + h,
                                                     return_mask=True, dedup=False)
            assert torch.equal(gn[h + 1], ids_h.reshape(-1)), (trial, h, counts, et)
            assert torch.equal(gw[h], w_h.reshape(-1)) and torch.equal(gt[h], t_h.reshape(-1))
            cur, mask, group = ids_h.reshape(-1), m_h, counts[h]


def test_uniform_weight_fast_path(EA, O, torch_cuda, k1_variant):
    """H1: a graph whose weights are all 1.0 (configs[1], ogbn-products-shaped) is
    sampled without a search - edge floor(u * deg) - and must still equal the
    reference's CDF inversion bit for bit, for one listed type of a two-type graph
    and for type draws (which take the reference loop)."""
    torch = torch_cuda
    rng = np.random.default_rng(31)
    ids, seg, nbr, w, nt, nw = make_random_graph(rng, 5000, 2, max_deg=60, id_space=10 ** 9,
                                                 zero_frac=0.0)
    w[:] = 1.0
    csr = O.csr_from_raw(ids, seg, nbr, w, 2, nt, nw)
    G = gpu_graph(EA, csr)
    OG = O.OracleGraph(csr)
    q = np.concatenate([rng.choice(ids, 4000), [0, 77]]).astype(np.int64)
    qt = torch.as_tensor(q).cuda()
    G.set_seed(3)
    for call, (et, count) in enumerate((([0], 25), ([1], 10), ([0, 1], 7), ([], 4))):
        on, ow, ot = OG.sample_neighbor(3, call, q, et, count, -1)
        gn, gw, gt = G.sample_neighbor(qt, et, count, -1, call_id=call)
        assert np.array_equal(t2n(gn), on), et
        assert np.array_equal(t2n(gw), ow) and np.array_equal(t2n(gt), ot)
    walk = G.random_walk(qt[:500], [[0]] * 8, 1.0, 1.0, -1, call_id=40)
    assert np.array_equal(t2n(walk), OG.random_walk(3, 40, q[:500], [[0]] * 8, 8, 1.0, 1.0, -1))


def test_small_fanout_in_one_launch(EA, O, torch_cuda, big_pair):
    """Tuning key 23: a 2-hop fanout of single listed types below the duplicate-root
    threshold runs as ONE launch (a workgroup draws a root's first-hop samples and,
    from LDS, their second-hop samples).  Same ids / weights / types as one launch
    per hop and as the oracle - including unknown roots, rows without the listed
    type, counts that are odd, larger than the block and equal to 1."""
    torch = torch_cuda
    from euler_amd import _lib
    G, OG, ids, rng = big_pair
    q = np.concatenate([rng.choice(ids, 700), [0, 4242, 2 ** 62]]).astype(np.int64)
    qt = torch.as_tensor(q).cuda()
    G.set_seed(19)
    try:
        for et, counts in (([[0], [1]], [25, 10]), ([[3], [3]], [7, 40]), ([[2], [0]], [1, 1]),
                           ([[1], [9]], [5, 3]), ([[0], [2]], [256, 2])):
            on, ow, ot = OG.sample_fanout(19, 77, q, et, counts, -5)
            res = []
            for fused in (1, 0):
                _lib.lib().euler_gpu_set_tuning(23, fused)
                res.append(G.sample_fanout(qt, et, counts, -5, call_id=77))
            for h in range(2):
                assert np.array_equal(t2n(res[0][0][h + 1]), on[h]), (et, counts, h)
                assert np.array_equal(t2n(res[0][1][h]), ow[h]) and np.array_equal(t2n(res[0][2][h]), ot[h])
                assert torch.equal(res[0][0][h + 1], res[1][0][h + 1])
                assert torch.equal(res[0][1][h], res[1][1][h]) and torch.equal(res[0][2][h], res[1][2][h])
    finally:
        _lib.lib().euler_gpu_set_tuning(23, 1)


def test_full_neighbor_fill_kernels_agree(EA, O, torch_cuda, big_pair):
    """Both fill passes of get_full_neighbor (tuning key 24: a lane owns 4 output entries /
    one wave per queried node) against the oracle: unknown ids, rows without the listed
    types, repeated ids, all type subsets."""
    torch = torch_cuda
    from euler_amd import _lib
    G, OG, ids, rng = big_pair
    q = np.concatenate([rng.choice(ids, 5000), rng.choice(ids[:20], 2000), [0, 31337]]).astype(np.uint64)
    qt = torch.as_tensor(q.astype(np.int64)).cuda()
    try:
        for et in ([0, 1, 2, 3], [2], [3, 0], [1, 1], []):
            wi, wd, ww, wt = OG.get_full_neighbor(q, et)
            for mode in (1, 0):
                _lib.lib().euler_gpu_set_tuning(24, mode)
                gi, gd, gw, gt = G.get_full_neighbor(qt, et)
                assert np.array_equal(t2n(gi), wi), (et, mode)
                assert np.array_equal(t2n(gd).astype(np.uint64), wd)
                assert np.array_equal(t2n(gw), ww) and np.array_equal(t2n(gt), wt)
    finally:
        _lib.lib().euler_gpu_set_tuning(24, 1)


_FL_DEFAULTS = {27: 1, 28: 0, 29: 0, 30: 0, 31: 1, 32: -1, 33: 32768, 34: 2, 35: 5, 45: 1, 53: 1, 55: 5, 75: 1}


@pytest.mark.parametrize("geom", [(4, 0, 256, 1, 8, 2, 0, 1), (1, 1, 64, 0, 5, 0, 0, 1), (2, 3, 128, 1, 8, 0, 0, 1),
                                  (8, 5, 256, 0, 8, 1, 3, 1), (16, 64, 64, 1, 5, 1, 0, 1), (3, 2, 256, 1, 8, 1, 1, 1),
                                  (1, 1, 64, 0, 8, 2, 0, 1), (8, 5, 128, 1, 8, 2, 3, 1), (16, 0, 256, 0, 8, 2, 1, 1),
                                  (5, 2, 256, 1, 8, 2, 0, 1), (4, 0, 64, 1, 5, 2, 0, 1), (2, 4, 128, 0, 6, 2, 1, 1),
                                  (4, 0, 64, 1, 5, 2, 0, 0), (8, 5, 128, 1, 8, 2, 3, 0), (3, 2, 256, 0, 6, 2, 1, 0),
                                  # 5 roots per wave: counts [25, 10] take the builds without the wide stores,
                                  # [3, 4] / [80, 6] those with them - the (wide, wps) pairs nothing above reaches
                                  (5, 2, 256, 1, 6, 2, 0, 1), (5, 2, 256, 1, 5, 2, 0, 1), (5, 2, 256, 1, 6, 2, 0, 0),
                                  (5, 2, 128, 1, 5, 2, 0, 0), (5, 2, 256, 0, 8, 2, 0, 0), (4, 0, 64, 0, 5, 2, 0, 1),
                                  # a ninth field 0: key 75 off - the plain weighted graph carries the side index, so
                                  # everything above draws hop 2 through it; these take the builds without it
                                  (5, 2, 256, 1, 5, 2, 0, 1, 0), (5, 2, 256, 1, 6, 2, 0, 1, 0), (5, 2, 128, 1, 8, 2, 0, 1, 0)],
                         ids=["default", "gr1cap1", "gr2cap3", "gr8cap5grid3", "gr16cap64", "gr3cap2grid1",
                              "lean_gr1cap1", "lean_gr8cap5grid3", "lean_gr16grid1", "lean_gr5cap2",
                              "lean_wb_shipped", "lean_wb_wps6_gr2", "lean_levels_shipped", "lean_levels_gr8",
                              "lean_levels_wps6", "lean_wb_wps6_gr5", "lean_wb_wps5_gr5", "lean_levels_wps6_gr5",
                              "lean_levels_wps5_gr5", "lean_levels_wps8_narrow", "lean_gr4_narrow",
                              "lean_wb_nohw_wps5", "lean_wb_nohw_wps6", "lean_wb_nohw_wps8"])
def test_fanout_local_dedup_kernel(EA, O, torch_cuda, big_pair, geom):
    """fanout_local.h: the 2-hop fanout of single listed types as ONE kernel - a wave owns
    `gr` roots, finds the distinct children among its own hop-1 samples and samples each
    once (`cap` of them per pass).  Every geometry (roots per wave, slots per pass, block
    size, 8- / 16-byte weight stores, register budget, constant-folded or general build,
    grid-stride loop) must give the oracle's ids / weights / types - including unknown
    roots, id 0, rows without the listed type, odd counts (scalar stores), count 1, ragged
    last tiles, duplicate roots, hashed and identity id maps, uniform weights and the
    id-0 sentinel rule - and what the hop-by-hop kernels write."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    gr, cap, block, wide, wps, plain, grid, wb = geom[:8]
    keys = {27: 2, 28: gr, 29: cap, 30: block, 31: wide, 32: grid, 33: 0, 34: plain, 35: wps, 45: wb,
            75: geom[8] if len(geom) > 8 else 1}

    def check(G, OG, q, et, counts, default, seed, call):
        qt = torch.as_tensor(q).cuda()
        G.set_seed(seed)
        on, ow, ot = OG.sample_fanout(seed, call, q, et, counts, default)
        L.euler_gpu_set_tuning(27, 2)
        gn, gw, gt = G.sample_fanout(qt, et, counts, default, call_id=call)
        for h in range(2):
            assert np.array_equal(t2n(gn[h + 1]), on[h]), (geom, len(q), et, counts, h)
            assert np.array_equal(t2n(gw[h]), ow[h]), (geom, len(q), et, counts, h)
            assert np.array_equal(t2n(gt[h]), ot[h]), (geom, len(q), et, counts, h)
        if len(et[0]) > 1:                      # typed hops: the row record walked in memory, not held in registers
            L.euler_gpu_set_tuning(48, 0)
            mn, mw, mt = G.sample_fanout(qt, et, counts, default, call_id=call)
            L.euler_gpu_set_tuning(48, 1)
            for h in range(2):
                assert torch.equal(gn[h + 1], mn[h + 1]) and torch.equal(gw[h], mw[h]) and torch.equal(gt[h], mt[h])
        L.euler_gpu_set_tuning(27, 0)           # hop by hop
        rn, rw, rt = G.sample_fanout(qt, et, counts, default, call_id=call)
        for h in range(2):
            assert torch.equal(gn[h + 1], rn[h + 1]) and torch.equal(gw[h], rw[h])
            assert torch.equal(gt[h], rt[h])

    try:
        for k_, v_ in keys.items():
            _lib.check(L.euler_gpu_set_tuning(k_, v_))
        # 4 edge types, arbitrary (hashed) ids
        G, OG, ids, rng = big_pair
        for B in (1, 7, 333, 2050):
            q = np.concatenate([rng.choice(ids, B), [0, 4242, 2 ** 62]]).astype(np.int64)
            if B == 1:
                q = q[:1]
            for et, counts in (([[0], [1]], [25, 10]), ([[3], [3]], [7, 40]), ([[2], [0]], [1, 1]),
                               ([[1], [9]], [5, 3]), ([[0], [2]], [70, 2]), ([[1], [1]], [10, 5]),
                               # hops that list several types: a type draw per sample (a sub-collection
                               # in the listed order, all groups, a list with a type the graph lacks,
                               # a type listed twice, an odd second count: hop by hop)
                               ([[0, 1], [2, 3]], [25, 10]), ([[0, 1, 2, 3], [3, 2, 1, 0]], [7, 4]),
                               ([[2, 0, 1], [1, 9, 0]], [5, 6]), ([[1, 1], [0, 3]], [10, 2]),
                               ([[3, 0], [0, 3]], [9, 8]), ([[0, 2], [1, 3]], [4, 3])):
                check(G, OG, q, et, counts, -5, 23, 91)
        # one edge type, identity ids: weighted (the constant-folded build) and uniform
        for weighted in (True, False):
            p = EA.synth_params(977, 20000, 260000, n_types=1, weighted=weighted)
            po = O.SynthParams()
            for f, _ in po._fields_:
                setattr(po, f, getattr(p, f))
            G1, OG1 = EA.Graph.synthetic(p), O.OracleGraph(O.synth_csr(po))
            r1 = np.random.default_rng(5)
            q = np.concatenate([r1.integers(1, 20001, 3001), [0, 20001, 1, 1, 2]]).astype(np.int64)
            for counts in ([25, 10], [3, 4], [10, 5], [1, 2], [80, 6]):
                check(G1, OG1, q, [[0], [0]], counts, 20001, 3, 6)
        # identity ids, 2 and 8 edge-type groups: every hop lists all of them / three of eight
        # (weights all 1.0 - what the reference's datasets have: the neighbour draw is an index computation)
        for T_, et, wgt in ((2, [[0, 1], [0, 1]], True), (2, [[1, 0], [1, 0]], True), (8, [[3, 1, 6], [0, 7, 2]], True),
                            (8, [list(range(8))] * 2, True), (2, [[0, 1], [0, 1]], False),
                            (3, [[2, 0], [1, 2]], False), (3, [[0, 1, 2], [2, 1, 0]], False),
                            (8, [[3, 1, 6], [0, 7, 2]], False),
                            # ... and one listed type per hop on such a graph (identity and hashed ids)
                            (2, [[0], [1]], False), (3, [[2], [2]], False), (-2, [[1], [0]], False),
                            (-2, [[0, 1], [1, 0]], False), (-1, [[0], [0]], False)):
            if (plain != 2 or gr not in (4, 8)) and (not wgt or T_ != 2):
                continue        # (these take the lean builds, which key 34 = 2 selects, in a few geometries:
                                #  elsewhere one case is enough)
            hashed = T_ < 0
            T_ = abs(T_)
            p = EA.synth_params(55 + T_, 20000, 400000, n_types=T_, weighted=wgt, hashed_ids=hashed)
            po = O.SynthParams()
            for f, _ in po._fields_:
                setattr(po, f, getattr(p, f))
            csr_t = O.synth_csr(po)
            Gt, OGt = EA.Graph.synthetic(p), O.OracleGraph(csr_t)
            q = np.concatenate([np.random.default_rng(8).integers(1, 20001, 2500), [0, 20001, 7, 7]]).astype(np.int64)
            if hashed:          # the graph knows node x by mix64(x)
                q = np.concatenate([np.random.default_rng(8).choice(csr_t.row_id, 2500),
                                    np.array([0, 4242, 7], np.uint64)]).astype(np.uint64).view(np.int64)
            for counts in ([25, 10], [3, 2]):
                check(Gt, OGt, q, et, counts, -7 if hashed else 20001, 12, 30)
        # ... and on hubs (rows of more than 64 edges: duplicates by id; several buckets per row)
        ph2 = EA.synth_params(37, 3000, 600000, n_types=2, weighted=True)
        po = O.SynthParams()
        for f, _ in po._fields_:
            setattr(po, f, getattr(ph2, f))
        Gh, OGh = EA.Graph.synthetic(ph2), O.OracleGraph(O.synth_csr(po))
        q = np.random.default_rng(9).integers(1, 3001, 600).astype(np.int64)
        check(Gh, OGh, q, [[0, 1], [1, 0]], [25, 10], 3001, 4, 50)
        # hubs: rows of thousands of edges (several pivot levels, > 64 edges: duplicates by id)
        ph = EA.synth_params(31, 3000, 900000, n_types=1, weighted=True)
        po = O.SynthParams()
        for f, _ in po._fields_:
            setattr(po, f, getattr(ph, f))
        G2, OG2 = EA.Graph.synthetic(ph), O.OracleGraph(O.synth_csr(po))
        q = np.random.default_rng(6).integers(1, 3001, 700).astype(np.int64)
        for counts in ([25, 10], [6, 4]):
            check(G2, OG2, q, [[0], [0]], counts, 3001, 9, 40)
        # Q1: a row whose FIRST sample is node id 0 is dropped (both hops)
        ids0 = np.array([0, 1, 2, 3], np.uint64)
        seg = np.array([0, 2, 4, 6, 7], np.int64)
        nbr = np.array([1, 2, 0, 2, 0, 3, 0], np.uint64)
        w = np.array([1, 1, 5, 1, 1, 1, 2], np.float32)
        csr = O.csr_from_raw(ids0, seg, nbr, w, 1)
        G0, OG0 = gpu_graph(EA, csr), O.OracleGraph(csr)
        q = np.array([0, 1, 2, 3, 9, 2, 2, 1], np.int64)
        for call in range(12):
            check(G0, OG0, q, [[0], [0]], [3, 2], -1, 1, call)
            check(G0, OG0, q, [[0], [0]], [4, 6], -1, 1, 100 + call)
    finally:
        for k_, v_ in _FL_DEFAULTS.items():
            L.euler_gpu_set_tuning(k_, v_)


@pytest.mark.parametrize("geom", [(0, 0, 0, 5, -1, 0), (4, 32, 128, 5, -1, 0), (4, 3, 64, 8, -1, 0), (4, 100, 256, 4, 0, 0),
                                  (2, 7, 128, 7, 5, 0), (4, 12, 128, 6, -1, 0), (4, 2, 64, 5, 3, 1), (1, 1, 64, 6, 1, 0),
                                  (4, 32, 128, 4, -1, 1), (4, 13, 256, 4, 7, 0), (4, 5, 64, 6, 2, 0)],
                         ids=["default_geometry", "cap32", "cap3_wps8", "cap100_wps4", "gr2_grid5", "cap12_wps6",
                              "three_chunks_cap2_grid3", "gr1_grid1", "three_chunks", "cap13_grid7", "cap5_wps6_grid2"])
def test_fanout_plain_kernel(EA, O, torch_cuda, geom):
    """fanout_plain.h (round 6): the one-kernel 2-hop fanout rebuilt for plain graphs served by
    the weight-bucket index.  Every build (register budget; hop 2 through the header + window
    lines - key 75 = 1 - or through the weight-bucket blocks) and geometry (roots per wave, slots per pass incl. several
    passes, block size, grid-stride loop) must write the oracle's ids / weights / types and
    what round 5's kernel (key 53 = 0) writes: unknown roots, id 0, duplicate roots, ragged
    last tiles, strided ids, dangling neighbour ids, hub rows (> 64 edges: duplicates by id;
    several buckets per row), rows without edges, several fanouts, several minibatches per
    launch and the (unique rows, index) form."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    gr, cap, block, wps, grid, hw = geom
    keys = {27: 2, 28: gr, 29: cap, 30: block, 32: grid, 33: 0, 55: wps, 75: hw, 53: 2}

    def check(G, OG, q, counts, default, seed, call, took=True):
        qt = torch.as_tensor(q).cuda()
        G.set_seed(seed)
        on, ow, ot = OG.sample_fanout(seed, call, q, [[0], [0]], counts, default)
        L.euler_gpu_set_tuning(53, 2)
        gn, gw, gt = G.sample_fanout(qt, [[0], [0]], counts, default, call_id=call)
        for h in range(2):
            assert np.array_equal(t2n(gn[h + 1]), on[h]), (geom, len(q), counts, h)
            assert np.array_equal(t2n(gw[h]), ow[h]), (geom, len(q), counts, h)
            assert np.array_equal(t2n(gt[h]), ot[h]), (geom, len(q), counts, h)
        L.euler_gpu_set_tuning(53, 0)           # round 5's kernel
        rn, rw, rt = G.sample_fanout(qt, [[0], [0]], counts, default, call_id=call)
        L.euler_gpu_set_tuning(53, 2)
        for h in range(2):
            assert torch.equal(gn[h + 1], rn[h + 1]) and torch.equal(gw[h], rw[h]) and torch.equal(gt[h], rt[h])
        if counts[1] % 2 == 0:
            id1, w1, t1, idx, rid, rw2, rt2 = G.sample_fanout_unique(qt, [[0], [0]], counts, default, call_id=call)
            assert np.array_equal(t2n(id1).reshape(-1), on[0]) and np.array_equal(t2n(w1).reshape(-1), ow[0])
            assert np.array_equal(t2n(rid[idx]).reshape(-1), on[1]), (geom, counts)
            assert np.array_equal(t2n(rw2[idx]).reshape(-1), ow[1]) and np.array_equal(t2n(rt2[idx]).reshape(-1), ot[1])

    try:
        for k_, v_ in keys.items():
            _lib.check(L.euler_gpu_set_tuning(k_, v_))
        # power-law plain graph: mostly rows of 1 - 2 edges, a few hubs
        p = EA.synth_params(977, 20000, 260000, n_types=1, weighted=True)
        po = O.SynthParams()
        for f, _ in po._fields_:
            setattr(po, f, getattr(p, f))
        G1, OG1 = EA.Graph.synthetic(p), O.OracleGraph(O.synth_csr(po))
        r1 = np.random.default_rng(5)
        for B in (1, 2, 3, 5, 333, 3001):
            q = np.concatenate([r1.integers(1, 20001, B), [0, 20001, 1, 1, 2]]).astype(np.int64)
            if B <= 3:
                q = q[:B]
            for counts in ([25, 10], [10, 10], [3, 4], [10, 6], [1, 2], [80, 6], [7, 64], [2, 2]):
                check(G1, OG1, q, counts, 20001, 3, 6)
        # hubs only: rows of hundreds / thousands of edges
        ph = EA.synth_params(31, 3000, 900000, n_types=1, weighted=True)
        po = O.SynthParams()
        for f, _ in po._fields_:
            setattr(po, f, getattr(ph, f))
        G2, OG2 = EA.Graph.synthetic(ph), O.OracleGraph(O.synth_csr(po))
        q = np.random.default_rng(6).integers(1, 3001, 701).astype(np.int64)
        for counts in ([25, 10], [6, 4]):
            check(G2, OG2, q, counts, 3001, 9, 40)
        # ids = base + stride * row, rows without edges, dangling neighbour ids, degrees around 64
        for base, stride in ((1, 1), (7, 3), (0, 2)):
            rng = np.random.default_rng(99 + stride)
            n = 6000
            ids = (base + stride * np.arange(n)).astype(np.uint64)
            deg = rng.choice([0, 1, 2, 3, 9, 10, 11, 40, 63, 64, 65, 66, 130], n)
            seg = np.zeros(n + 1, np.int64)
            seg[1:] = np.cumsum(deg)
            E = int(seg[-1])
            nbr = rng.choice(ids[1:] if base == 0 else ids, E).astype(np.uint64)      # (no neighbour id 0)
            dang = rng.random(E) < 0.03
            nbr[dang] = nbr[dang] + (1 if stride > 1 else stride * n + 7)
            w = (rng.random(E) * 7.5 + 0.5).astype(np.float32)
            csr = O.csr_from_raw(ids, seg, nbr, w, 1, np.zeros(n, np.int32), np.ones(n, np.float32))
            G3, OG3 = gpu_graph(EA, csr), O.OracleGraph(csr)
            q = np.concatenate([rng.choice(ids, 2049), [0, base + stride * n + 1, base + 1]]).astype(np.int64)
            for counts in ([25, 10], [4, 6]):
                check(G3, OG3, q, counts, -1, 21, 60)
        # several minibatches per launch: minibatch b draws with its own call id
        M, Bm = 5, 64
        r = np.random.default_rng(8).integers(1, 20001, (M, Bm)).astype(np.int64)
        G1.set_seed(77)
        res = G1.sample_fanout_multi(torch.as_tensor(r).cuda(), [[0], [0]], [25, 10], 20001, call_id=500)
        for b in range(M):
            on, ow, ot = OG1.sample_fanout(77, 500 + 2 * b, r[b], [[0], [0]], [25, 10], 20001)
            nb, wb, tb = res[b]
            for h in range(2):
                assert np.array_equal(t2n(nb[h + 1]).reshape(-1), on[h]), (geom, b, h)
                assert np.array_equal(t2n(wb[h]).reshape(-1), ow[h]) and np.array_equal(t2n(tb[h]).reshape(-1), ot[h])
    finally:
        for k_, v_ in _FL_DEFAULTS.items():
            L.euler_gpu_set_tuning(k_, v_)
        L.euler_gpu_set_tuning(75, 1)


def test_retired_fanout_keys_are_refused(EA, O, torch_cuda):
    """Tuning keys 54 and 57 selected two builds of the plain-graph fanout kernel that were removed:
    setting them is an error (no stub that accepts and ignores), and the call changes nothing -
    a [3, 2] fanout gives the same tensors before and after."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    p = EA.synth_params(977, 20000, 260000, n_types=1, weighted=True)
    G = EA.Graph.synthetic(p)
    q = torch.as_tensor(np.array([1, 2, 17, 4000, 19999, 20000, 17], np.int64)).cuda()
    G.set_seed(3)
    try:
        _lib.check(L.euler_gpu_set_tuning(33, 0))
        bn, bw, bt = G.sample_fanout(q, [[0], [0]], [3, 2], 20001, call_id=6)
        for k_ in (54, 57):
            for v_ in (0, 1):
                assert L.euler_gpu_set_tuning(k_, v_) != 0, (k_, v_)
        an, aw, at = G.sample_fanout(q, [[0], [0]], [3, 2], 20001, call_id=6)
        for h in range(2):
            assert torch.equal(bn[h + 1], an[h + 1]) and torch.equal(bw[h], aw[h]) and torch.equal(bt[h], at[h])
    finally:
        L.euler_gpu_set_tuning(33, 32768)


def test_sample_fanout_multi_equals_separate_calls(EA, O, torch_cuda, big_pair):
    """euler_gpu_sample_fanout_multi: M minibatches in one enqueue == M separate
    sample_fanout calls == the oracle, bit for bit (draws are keyed by (call id, node id)).
    Covers the workgroup-per-root kernel (few roots in all), the wave-per-4-roots kernels
    (lean and general build; totals >= 8 192), minibatch sizes that are not a multiple of the
    tile (the launcher shrinks the tile), shapes that fall back to one enqueue per minibatch
    (3 hops, several listed types), explicit device call ids, hashed and identity id maps."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()

    def run(G, OG, batches, et, counts, default, seed, call, ids=None, oracle_rows=2):
        G.set_seed(seed)
        bt = torch.as_tensor(batches).cuda()
        layers = len(counts)
        cid = None if ids is None else torch.as_tensor(np.asarray(ids, np.int32)).cuda()
        res = G.sample_fanout_multi(bt, et, counts, default, call_id=call, call_ids=cid)
        assert len(res) == len(batches)
        for b in range(len(batches)):
            c = call + b * layers if ids is None else int(ids[b])
            sn, sw, st = G.sample_fanout(bt[b], et, counts, default, call_id=c)
            for h in range(layers):
                assert torch.equal(res[b][0][h + 1], sn[h + 1]), (b, h, counts)
                assert torch.equal(res[b][1][h], sw[h]) and torch.equal(res[b][2][h], st[h])
            if b < oracle_rows or b == len(batches) - 1:
                on, ow, ot = OG.sample_fanout(seed, c, np.asarray(batches[b]), et, counts, default)
                for h in range(layers):
                    assert np.array_equal(t2n(res[b][0][h + 1]), on[h]), (b, h, counts)
                    assert np.array_equal(t2n(res[b][1][h]), ow[h])
                    assert np.array_equal(t2n(res[b][2][h]), ot[h])

    # hashed ids, 4 edge types: general build / workgroup-per-root kernel / fallbacks
    G, OG, ids, rng = big_pair
    for M, B in ((1, 5), (3, 64), (7, 130), (16, 1024), (5, 2050)):
        q = rng.choice(ids, M * B).astype(np.int64).reshape(M, B)
        q[0, 0] = 0
        q[-1, -1] = 2 ** 62
        run(G, OG, q, [[0], [1]], [25, 10], -5, 23, 1000)
        run(G, OG, q, [[3], [3]], [5, 4], -5, 23, 7)
    q = rng.choice(ids, 4 * 96).astype(np.int64).reshape(4, 96)
    run(G, OG, q, [[0], [1], [2]], [4, 3, 2], -5, 23, 50)           # 3 hops: one enqueue each
    run(G, OG, q, [[0, 1], [1, 2]], [6, 3], -5, 23, 60)             # type draws: one enqueue each
    run(G, OG, q, [[0], [1]], [25, 10], -5, 23, 0, ids=[900, 3, 3, 2 ** 31 - 2])
    # type draws with enough roots for the one-kernel form: tiles of several minibatches in one
    # launch, consecutive and explicit call ids
    q = rng.choice(ids, 16 * 1024).astype(np.int64).reshape(16, 1024)
    run(G, OG, q, [[0, 1], [2, 3]], [6, 4], -5, 23, 300)
    run(G, OG, q, [[0, 1, 2, 3], [3, 2, 1, 0]], [5, 2], -5, 23, 0, ids=list(range(40, 56)))
    # identity ids, one type: lean build (weighted) and its uniform-weight form
    for weighted in (True, False):
        p = EA.synth_params(977, 20000, 260000, n_types=1, weighted=weighted)
        po = O.SynthParams()
        for f, _ in po._fields_:
            setattr(po, f, getattr(p, f))
        G1, OG1 = EA.Graph.synthetic(p), O.OracleGraph(O.synth_csr(po))
        r1 = np.random.default_rng(5)
        for M, B in ((64, 1024), (9, 1001), (2, 8192), (33, 256)):
            q = r1.integers(0, 20002, M * B).astype(np.int64).reshape(M, B)
            run(G1, OG1, q, [[0], [0]], [25, 10], 20001, 3, 6, oracle_rows=1)
        q = r1.integers(1, 20001, 12 * 1024).astype(np.int64).reshape(12, 1024)
        run(G1, OG1, q, [[0], [0]], [25, 10], 20001, 3, 0, ids=list(range(100, 112)), oracle_rows=1)
        run(G1, OG1, q, [[0], [0]], [3, 4], 20001, 3, 77, oracle_rows=1)
    # empty
    assert G1.sample_fanout_multi(torch.zeros((0, 8), dtype=torch.int64).cuda(), [[0], [0]], [2, 2]) == []


def test_sample_neighbor_sets_one_launch(EA, O, torch_cuda, big_pair):
    """euler_gpu_sample_neighbor_sets / _sample_aggregate_sets: the SampleNeighbor ops a
    heterogeneous model issues over one batch of roots - one per edge-type set - as ONE launch.
    Set s == sample_neighbor(call_id + s) == the oracle for every type mode of
    Node::__SampleNeighbor (one listed type, a sub-collection in the listed order, all groups,
    an empty list, a type the graph does not have, more types listed than exist), unknown
    roots and id 0; with and without the weight-bucket index; and the aggregation of the same
    enqueue == scatter_(aggr, gather(feat, neighbours)) bit for bit."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    G, OG, ids, rng = big_pair                     # hashed ids, 4 edge types
    q = np.concatenate([rng.choice(ids, 3000), [0, 4242, 2 ** 62]]).astype(np.int64)
    qt = torch.as_tensor(q).cuda()
    sets = [[3], [1, 2], [0, 1, 2, 3], [], [2, 0, 1], [9], [0, 1, 2, 3, 0], [1]]
    try:
        # (45: weight-bucket index or pivot levels; 47: the roots' records staged in LDS or read per lane)
        for wb, lds in ((1, 1), (1, 0), (0, 1)):
            L.euler_gpu_set_tuning(45, wb)
            L.euler_gpu_set_tuning(47, lds)
            for count in (10, 1, 7, 300):
                G.set_seed(5)
                gn, gw, gt = G.sample_neighbor_sets(qt, sets, count, -3, call_id=70)
                assert tuple(gn.shape) == (len(sets), len(q), count)
                for s_, et in enumerate(sets):
                    a = G.sample_neighbor(qt, et, count, -3, call_id=70 + s_)
                    assert torch.equal(gn[s_], a[0]) and torch.equal(gw[s_], a[1]) and torch.equal(gt[s_], a[2]), (wb, et)
                    on, ow, ot = OG.sample_neighbor(5, 70 + s_, q, et, count, -3)
                    assert np.array_equal(t2n(gn[s_]).reshape(-1), on.reshape(-1)), (wb, et, count)
                    assert np.array_equal(t2n(gw[s_]).reshape(-1), ow.reshape(-1))
                    assert np.array_equal(t2n(gt[s_]).reshape(-1), ot.reshape(-1))
    finally:
        L.euler_gpu_set_tuning(45, 1)
        L.euler_gpu_set_tuning(47, 1)
    # identity ids, 8 types, with the aggregation (feature table indexed by node id)
    N, T, D, CNT = 20000, 8, 32, 10
    p = EA.synth_params(99, N, 400000, n_types=T, weighted=True)
    G1 = EA.Graph.synthetic(p)
    G1.set_seed(4)
    r = torch.as_tensor(np.random.default_rng(2).integers(1, N + 1, 5000).astype(np.int64)).cuda()
    feat = torch.randn(N + 2, D, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    tsets = [[3], [1, 4, 6], list(range(T))]
    dst = torch.arange(5000, device="cuda", dtype=torch.int32).repeat_interleave(CNT)
    for aggr in ("mean", "add", "max"):
        gn, gw, gt, agg = G1.sample_neighbor_sets(r, tsets, CNT, N + 1, call_id=9, feat=feat, aggr=aggr)
        for s_, et in enumerate(tsets):
            a = G1.sample_neighbor(r, et, CNT, N + 1, call_id=9 + s_)
            assert torch.equal(gn[s_], a[0]) and torch.equal(gw[s_], a[1]) and torch.equal(gt[s_], a[2])
            x = EA.ops.gather(feat, a[0].reshape(-1).to(torch.int32))
            ref = {"mean": EA.ops.scatter_mean, "add": EA.ops.scatter_add, "max": EA.ops.scatter_max}[aggr](x, dst, 5000)
            assert torch.equal(agg[s_], ref), (aggr, et)
    # a feature table that does not cover the ids is refused
    # (a default fill inside the table, so the C entry's own check of the graph's ids is what refuses)
    with pytest.raises(_lib.EulerGpuError):
        G1.sample_neighbor_sets(r, tsets, CNT, 5, feat=feat[:100].contiguous())
    # ... and a default fill that names no row of the table is refused before the call
    with pytest.raises(ValueError):
        G1.sample_neighbor_sets(r, tsets, CNT, N + 1, feat=feat[:100].contiguous())
    # nothing to do
    e = G1.sample_neighbor_sets(r[:0], tsets, CNT, N + 1)
    assert tuple(e[0].shape) == (3, 0, CNT)


def test_node2vec_step_on_fetched_lists_wave_and_lane(EA, O, torch_cuda):
    """euler_gpu_node2vec_step - the step of the SHARDED node2vec walk, on explicit lists
    (random_walk_op.cc:83-168 on the rows `v(nodes).outV(...)` returned) - run by the wave
    kernels of the single-GPU walk (tuning key 7 = 2, default) and by the lane-per-walker
    reference loop (key 7 = 0): both == the single-GPU walk == the oracle, on hub rows of
    thousands of neighbours (several chunks, checkpoints, parent cursor events), walkers that
    share rows, unknown nodes and empty lists."""
    torch = torch_cuda
    from euler_amd import _lib, ops
    L = _lib.lib()
    ph = EA.synth_params(31, 3000, 900000, n_types=1, weighted=True)
    po = O.SynthParams()
    for f, _ in po._fields_:
        setattr(po, f, getattr(ph, f))
    G, OG = EA.Graph.synthetic(ph), O.OracleGraph(O.synth_csr(po))
    q = np.concatenate([np.random.default_rng(4).integers(1, 3001, 1500), [0, 3001, 7, 7, 7]]).astype(np.int64)
    qt = torch.as_tensor(q).cuda()
    steps = 4
    try:
        for p_, q_ in ((0.25, 4.0), (3.0, 0.7)):
            G.set_seed(5)
            want = G.random_walk(qt, [[0]] * steps, p_, q_, 3001, call_id=77)
            assert np.array_equal(t2n(want), OG.random_walk(5, 77, q, [[0]] * steps, steps, p_, q_, 3001))
            # (mode 2 twice: rows of >= 65 536 / >= 200 entries by a workgroup of 16 waves each -
            # N2vBigStepListKernel, tuning key 69; this graph's rows average 300 entries, hubs thousands)
            # (key 71: walkers whose PARENT's row is long go to a workgroup as well)
            # (key 72: both queues in one launch - the default - or the waves' launch, then the workgroups')
            for mode, big_at, par_at, merged in ((2, 65536, 65536, 1), (2, 200, 65536, 1), (2, 200, 65536, 0), (2, 4000, 150, 1),
                                                 (2, 4000, 150, 0), (2, 65536, 0, 1), (0, 65536, 65536, 1)):
                L.euler_gpu_set_tuning(7, mode)
                L.euler_gpu_set_tuning(69, big_at)
                L.euler_gpu_set_tuning(71, par_at)
                L.euler_gpu_set_tuning(72, merged)
                cur = parent = qt
                p_row = p_idx = p_ids = None
                cols = [qt]
                for s_ in range(steps):
                    # one row per DISTINCT node + the row of every walker, as the sharded sampler fetches
                    uq, inv = torch.unique(cur, return_inverse=True)
                    idx, ids, w, _t = G.get_full_neighbor(uq, [0])
                    nxt = ops.node2vec_step(5, 77 + s_, inv, idx, ids, w, p_row, p_idx, p_ids, parent, p_, q_, 3001)
                    parent, cur = cur, nxt
                    p_row, p_idx, p_ids = inv, idx, ids
                    cols.append(cur)
                assert torch.equal(torch.stack(cols, 1), want), (p_, q_, mode, big_at, par_at, merged)
    finally:
        L.euler_gpu_set_tuning(7, 2)
        L.euler_gpu_set_tuning(69, 65536)
        L.euler_gpu_set_tuning(71, 65536)
        L.euler_gpu_set_tuning(72, 1)


def test_sample_neighbor_sets_packed_equals_the_separate_packed_calls(EA, O, torch_cuda):
    """euler_gpu_sample_neighbor_sets_packed - the owners' passes of a heterogeneous minibatch's typed
    hops as ONE launch writing wire rows: every word ops.expand_packed reads equals the rows of the
    separate sample_neighbor_packed calls (one type: no type column; several: type draws), through
    the kernel that stages the records in LDS, the plain one and the fallback to separate calls
    (tuning keys 47 / 37), and the expanded rows == the oracle's SampleNeighbor per set."""
    torch = torch_cuda
    from euler_amd import _lib, ops
    L = _lib.lib()
    ph = EA.synth_params(17, 4000, 90000, n_types=5, weighted=True)
    po = O.SynthParams()
    for f, _ in po._fields_:
        setattr(po, f, getattr(ph, f))
    G, OG = EA.Graph.synthetic(ph), O.OracleGraph(O.synth_csr(po))
    G.set_seed(23)
    ids = np.concatenate([np.random.default_rng(8).permutation(4000)[:1500] + 1, [0, 4001]]).astype(np.int64)
    it = torch.as_tensor(ids).cuda()
    sets = [[2], [0, 3, 4], [0, 1, 2, 3, 4], [1]]
    try:
        for count in (10, 7):
            want = [G.sample_neighbor_packed(it, et, count, 4001, call_id=50 + s) for s, et in enumerate(sets)]
            for lds, typed in ((1, 1), (2, 1), (0, 1), (1, 0)):
                L.euler_gpu_set_tuning(47, lds)
                L.euler_gpu_set_tuning(37, typed)
                got = G.sample_neighbor_sets_packed(it, sets, count, 4001, call_id=50)
                for s, et in enumerate(sets):
                    used = (3 if len(et) == 1 else 4) * count + 1          # ids | weights | [types] | mask
                    assert got[s].shape == want[s].shape
                    assert torch.equal(got[s][:, :used], want[s][:, :used]), (count, lds, typed, s)
            L.euler_gpu_set_tuning(47, 1); L.euler_gpu_set_tuning(37, 1)
            pos = torch.arange(len(ids), dtype=torch.int32, device="cuda")
            for s, et in enumerate(sets):
                g_ids, g_w, g_t, g_m = ops.expand_packed(pos, got[s], count, et[0] if len(et) == 1 else None)
                o_ids, o_w, o_t = OG.sample_neighbor(23, 50 + s, ids, et, count, 4001)
                assert np.array_equal(t2n(g_ids).reshape(-1), np.asarray(o_ids).reshape(-1)), (count, s)
                assert np.array_equal(t2n(g_w).reshape(-1), np.asarray(o_w).reshape(-1))
                assert np.array_equal(t2n(g_t).reshape(-1), np.asarray(o_t).reshape(-1))
    finally:
        L.euler_gpu_set_tuning(47, 1)
        L.euler_gpu_set_tuning(37, 1)


def test_node2vec_walk_hands_walkers_out_by_ticket(EA, O, torch_cuda):
    """More than 16 384 walkers: the one-launch node2vec walk hands its walkers out by ticket (tuning
    key 73) instead of giving every 16 384th walker to a wave.  Which wave walks a walker does not
    matter - the draws are keyed by the walker's index: == the static assignment == the oracle."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    ph = EA.synth_params(91, 5000, 120000, n_types=2, weighted=True)
    po = O.SynthParams()
    for f, _ in po._fields_:
        setattr(po, f, getattr(ph, f))
    G, OG = EA.Graph.synthetic(ph), O.OracleGraph(O.synth_csr(po))
    q = np.random.default_rng(5).integers(0, 5002, 40000).astype(np.int64)      # (0 and 5001: unknown nodes)
    qt = torch.as_tensor(q).cuda()
    et = [[0, 1], [1, 0], [0, 1], [1, 0]]
    try:
        G.set_seed(3)
        outs = []
        for tickets in (1, 0):
            L.euler_gpu_set_tuning(73, tickets)
            outs.append(G.random_walk(qt, et, 0.25, 4.0, 5001, call_id=11))
        assert torch.equal(outs[0], outs[1])
        assert np.array_equal(t2n(outs[0]), OG.random_walk(3, 11, q, et, len(et), 0.25, 4.0, 5001))
    finally:
        L.euler_gpu_set_tuning(73, 1)


def test_node2vec_step_self_loop_rows_in_two_buffers(EA, O, torch_cuda):
    """A walker that took a self loop stands on its parent: on FETCHED rows the child list and the
    parent's list are then the same ids in two buffers (this step's rows, last step's rows), every
    child is a common neighbour and the parent cursor moves on every entry.  The kernels
    recognise equal id sequences (N2vSameFetched / N2vSameFetchedBlock) instead of handing a
    long row to the sequential automaton; rows that differ in one entry (first / middle / last),
    or in length, must not be taken for equal.  Wave kernel, workgroup kernel (key 69 = 2 000, long
    parent rows: key 71), one launch or two (key 72) and the lane-per-walker loop == the oracle's
    restatement of the client loop (random_walk_op.cc:83-168)."""
    torch = torch_cuda
    from euler_amd import _lib, ops
    L = _lib.lib()
    rng = np.random.default_rng(77)
    lens = [1, 2, 63, 64, 65, 300, 2500, 5000]
    c_idx, c_ids, c_w, p_idx, p_ids, c_row, p_row, parent = [], [], [], [], [], [], [], []
    def add_row(idx, ids, row):
        idx.append([len(ids), len(ids) + len(row)])
        ids.extend(int(x) for x in row)
    for n in lens:
        row = rng.integers(1, 1 << 40, n)
        if n > 2:
            row[n // 3] = 424242                       # the node itself: the self loop's edge
        variants = [row.copy()]                         # the parent's row: the same ids ...
        for at in (0, n // 2, n - 1):                   # ... or one entry apart
            v = row.copy(); v[at] += 1; variants.append(v)
        variants.append(row[:-1].copy() if n > 1 else np.concatenate([row, row]))   # another length
        variants.append(np.sort(row))                   # an ascending parent row (events)
        for v in variants:
            add_row(c_idx, c_ids, row)
            c_w.extend(rng.uniform(0.5, 8.0, n).astype(np.float32).tolist())
            add_row(p_idx, p_ids, v)
            c_row.append(len(c_idx) - 1); p_row.append(len(p_idx) - 1); parent.append(424242)
    n_w = len(c_row)
    # several walkers per row pair (rows are shared between walkers on one node)
    c_row = np.asarray(c_row * 3, np.int32); p_row = np.asarray(p_row * 3, np.int32)
    parent = np.asarray(parent * 3, np.int64)
    c_idx = np.asarray(c_idx, np.int32); p_idx = np.asarray(p_idx, np.int32)
    c_ids = np.asarray(c_ids, np.uint64); p_ids = np.asarray(p_ids, np.uint64)
    c_w = np.asarray(c_w, np.float32)
    cu = lambda a: torch.as_tensor(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    try:
        for p_, q_ in ((0.25, 4.0), (3.0, 0.7)):
            want = O.node2vec_step_lists(9, 41, c_row, c_idx, c_ids, c_w, p_row, p_idx, p_ids, parent, p_, q_, -5)
            for mode, big_at, par_at, merged in ((2, 65536, 65536, 1), (2, 2000, 65536, 1), (2, 2000, 65536, 0),
                                                 (2, 2000, 0, 1), (2, 65536, 0, 0), (2, 65536, 60, 1),
                                                 (2, 4000, 300, 1), (2, 4000, 300, 0), (0, 65536, 65536, 1)):
                L.euler_gpu_set_tuning(7, mode)
                L.euler_gpu_set_tuning(69, big_at)
                L.euler_gpu_set_tuning(71, par_at)
                L.euler_gpu_set_tuning(72, merged)
                got = ops.node2vec_step(9, 41, cu(c_row), cu(c_idx), cu(c_ids), cu(c_w), cu(p_row), cu(p_idx),
                                        cu(p_ids), cu(parent), p_, q_, -5)
                assert np.array_equal(t2n(got), want), (p_, q_, mode, big_at, par_at, merged)
        assert n_w == len(lens) * 6
    finally:
        L.euler_gpu_set_tuning(7, 2)
        L.euler_gpu_set_tuning(69, 65536)
        L.euler_gpu_set_tuning(71, 65536)
        L.euler_gpu_set_tuning(72, 1)


@pytest.mark.parametrize("index_alone", [0, 1])
def test_heavy_tailed_weights_take_the_second_chance(EA, O, torch_cuda, index_alone):
    """Rows whose weights are far from even - Pareto(0.7): dust among giants - make the weight-bucket
    index's blocks miss a few draws in a hundred.  The keys decide, so the results do not change:
    K1 / typed / small-batch kernels fall through to the pivot levels inside BlockPivotSample, the
    lean kernels are kept off the index by the builder's overflow count (wb_lean_ok) and walk the
    levels.  SampleNeighbor, the fanout at every size class, type sets and walks == the oracle.
    index_alone = 1 (tuning key 51): the graph gets NO EdgeBlocks - the state of every graph the
    index serves since round 5 - so each of those missed draws takes the fallback such graphs
    have, the bisection of the flat running sums, in every kernel family."""
    torch = torch_cuda
    from euler_amd import _lib
    _lib.check(_lib.lib().euler_gpu_set_tuning(51, index_alone))
    try:
        _heavy_tailed_battery(EA, O, torch)
    finally:
        _lib.lib().euler_gpu_set_tuning(51, 0)


def _heavy_tailed_battery(EA, O, torch):
    rng = np.random.default_rng(21)
    n = 4000
    deg = np.minimum(rng.zipf(1.6, n), 6000).astype(np.int64)
    seg = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(seg[-1])
    ids = np.arange(1, n + 1, dtype=np.uint64)
    nbr = rng.integers(1, n + 1, E).astype(np.uint64)
    w = (rng.pareto(0.7, E) + 1e-3).astype(np.float32)
    csr = O.csr_from_raw(ids, seg, nbr, w, 1)
    G, OG = gpu_graph(EA, csr), O.OracleGraph(csr)
    hubs = ids[np.argsort(-deg)[:200]].astype(np.int64)
    q = np.concatenate([rng.integers(1, n + 1, 3000), hubs, hubs, [0, n + 7]]).astype(np.int64)
    qt = torch.as_tensor(q).cuda()
    G.set_seed(9)
    for count in (10, 25, 7):
        a = G.sample_neighbor(qt, [0], count, -1, call_id=5)
        on, ow, ot = OG.sample_neighbor(9, 5, q, [0], count, -1)
        assert np.array_equal(t2n(a[0]).reshape(-1), on.reshape(-1)), count
        assert np.array_equal(t2n(a[1]).reshape(-1), ow.reshape(-1))
    for B in (64, 3000, len(q)):                     # workgroup-per-root, hop by hop, one-kernel
        for counts in ([25, 10], [5, 4]):
            gn, gw, gt = G.sample_fanout(qt[:B], [[0], [0]], counts, -1, call_id=11)
            on, ow, ot = OG.sample_fanout(9, 11, q[:B], [[0], [0]], counts, -1)
            for h in range(2):
                assert np.array_equal(t2n(gn[h + 1]), on[h]), (B, counts, h)
                assert np.array_equal(t2n(gw[h]), ow[h])
    big = torch.as_tensor(np.tile(q, 12)[:40000]).cuda()             # >= 32 768 roots: the lean kernel
    gn, gw, gt = G.sample_fanout(big, [[0], [0]], [25, 10], -1, call_id=13)
    on, ow, ot = OG.sample_fanout(9, 13, t2n(big), [[0], [0]], [25, 10], -1)
    assert np.array_equal(t2n(gn[2]), on[1]) and np.array_equal(t2n(gw[1]), ow[1])
    sn, sw, st = G.sample_neighbor_sets(qt, [[0], [0, 0], []], 6, -1, call_id=30)
    for s_, et in enumerate([[0], [0, 0], []]):
        on, ow, ot = OG.sample_neighbor(9, 30 + s_, q, et, 6, -1)
        assert np.array_equal(t2n(sn[s_]).reshape(-1), on.reshape(-1)), et
    walk = G.random_walk(qt, [[0]] * 6, 1.0, 1.0, -1, call_id=40)
    assert np.array_equal(t2n(walk), OG.random_walk(9, 40, q, [[0]] * 6, 6, 1.0, 1.0, -1))
    # several edge-type groups: the typed kernels (a segment's limits out of the row's record, type
    # draws, type sets, typed hops of the fanout, a walk on one listed type) on such weights
    T = 3
    deg3 = np.minimum(rng.zipf(1.7, n * T), 3000).astype(np.int64)
    seg3 = np.concatenate([[0], np.cumsum(deg3)]).astype(np.int64)
    e3 = int(seg3[-1])
    csr3 = O.csr_from_raw(ids, seg3, rng.integers(1, n + 1, e3).astype(np.uint64),
                          (rng.pareto(0.7, e3) + 1e-3).astype(np.float32), T)
    G3, OG3 = gpu_graph(EA, csr3), O.OracleGraph(csr3)
    G3.set_seed(9)
    sets3 = [[1], [0, 1, 2], [2, 0], []]
    for et in sets3:
        a = G3.sample_neighbor(qt, et, 10, -1, call_id=7)
        on, ow, ot = OG3.sample_neighbor(9, 7, q, et, 10, -1)
        assert np.array_equal(t2n(a[0]).reshape(-1), on.reshape(-1)), et
        assert np.array_equal(t2n(a[1]).reshape(-1), ow.reshape(-1)), et
        assert np.array_equal(t2n(a[2]).reshape(-1), ot.reshape(-1)), et
    sn, sw, st = G3.sample_neighbor_sets(qt, sets3, 6, -1, call_id=50)
    for s_, et in enumerate(sets3):
        on, ow, ot = OG3.sample_neighbor(9, 50 + s_, q, et, 6, -1)
        assert np.array_equal(t2n(sn[s_]).reshape(-1), on.reshape(-1)), et
        assert np.array_equal(t2n(st[s_]).reshape(-1), ot.reshape(-1)), et
    for etf in ([[0, 1], [1, 2]], [[2], [0]]):
        gn, gw, gt = G3.sample_fanout(qt, etf, [4, 6], -1, call_id=17)
        on, ow, ot = OG3.sample_fanout(9, 17, q, etf, [4, 6], -1)
        for h in range(2):
            assert np.array_equal(t2n(gn[h + 1]), on[h]), (etf, h)
            assert np.array_equal(t2n(gw[h]), ow[h]) and np.array_equal(t2n(gt[h]), ot[h])
    walk = G3.random_walk(qt, [[1]] * 5, 1.0, 1.0, -1, call_id=60)
    assert np.array_equal(t2n(walk), OG3.random_walk(9, 60, q, [[1]] * 5, 5, 1.0, 1.0, -1))


def test_random_walk_over_merged_walkers(EA, O, torch_cuda, big_pair):
    """DeepWalk over groups of merged walkers (walk_kernels.hip: CwSampleKernel /
    CwNumberKernel / CwTailKernel / CwPathKernel - or CwChainKernel / CwTransposeKernel when the
    merging part of the walk is too long for the path kernel's LDS tile: the 130-step walk
    with tail 0 -, tuning key 38): walkers that meet on a node in a step
    share every later draw (the draw is keyed by node id and step), so the walk is run once
    per distinct node and expanded.  Same paths as the per-walker kernel and the oracle -
    after `tail` steps (key 43) the groups stop merging and finish the walk in one launch;
    duplicate and unknown start nodes, dangling neighbour ids (never merged: they are
    different ids), rows without the listed type, hashed and identity id maps, one listed
    type (pivot search) and several (reference loop), walk lengths around the staging size
    and beyond what the transpose holds in LDS at once (131 steps: three passes)."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    G, OG, ids, rng = big_pair
    try:
        for n, walk_len, et in ((5000, 9, [[0, 1, 2, 3]]), (777, 4, [[2]]), (3000, 17, [[1, 3]]), (300, 130, [[1]]),
                                (2500, 8, [[3]])):
            et_w = et * walk_len
            q = np.concatenate([rng.choice(ids, n), rng.choice(ids, 50).repeat(4),
                                [0, 4242, 2 ** 62]]).astype(np.int64)
            qt = torch.as_tensor(q).cuda()
            G.set_seed(41)
            want = OG.random_walk(41, 500, q, et_w, walk_len, 1.0, 1.0, -9)
            L.euler_gpu_set_tuning(38, 0)
            ref = G.random_walk(qt, et_w, 1.0, 1.0, -9, call_id=500)
            assert np.array_equal(t2n(ref), want), (n, walk_len, et)
            # merging all the way (0), then from step 1 / 3 / 12 on every group walks alone
            for tail in (0, 1, 3, 9, 12):
                L.euler_gpu_set_tuning(38, 1)
                L.euler_gpu_set_tuning(43, tail)
                got = G.random_walk(qt, et_w, 1.0, 1.0, -9, call_id=500)
                assert torch.equal(got, ref), (n, walk_len, et, tail)
        # identity ids, hubs: most walkers merge within a few steps
        p = EA.synth_params(17, 30000, 600000, n_types=1, weighted=True)
        po = O.SynthParams()
        for f, _ in po._fields_:
            setattr(po, f, getattr(p, f))
        G1, OG1 = EA.Graph.synthetic(p), O.OracleGraph(O.synth_csr(po))
        q = np.concatenate([np.random.default_rng(3).integers(1, 30001, 40000),
                            [0, 30001, 2 ** 40, 1, 1]]).astype(np.int64)
        G1.set_seed(8)
        L.euler_gpu_set_tuning(38, 1)
        want1 = OG1.random_walk(8, 3, q, [[0]] * 12, 12, 1.0, 1.0, 30001)
        # a plain graph: the draws come from the lean search (key 44) or the block pivots
        # (with key 45 = 1, the default, the lean draws go through the weight-bucket index)
        for lean, tail, wb in ((1, 0, 1), (1, 5, 1), (1, 11, 1), (0, 5, 1), (1, 0, 0), (1, 5, 0)):
            L.euler_gpu_set_tuning(44, lean)
            L.euler_gpu_set_tuning(43, tail)
            L.euler_gpu_set_tuning(45, wb)
            got = G1.random_walk(torch.as_tensor(q).cuda(), [[0]] * 12, 1.0, 1.0, 30001, call_id=3)
            assert np.array_equal(t2n(got), want1), (lean, tail, wb)
        L.euler_gpu_set_tuning(45, 1)
        # a listed type the graph does not have: every walker stops at once
        L.euler_gpu_set_tuning(44, 1)
        got = G1.random_walk(torch.as_tensor(q).cuda(), [[0], [0], [2], [0], [0]], 1.0, 1.0, 30001, call_id=9)
        assert np.array_equal(t2n(got), OG1.random_walk(8, 9, q, [[0], [0], [2], [0], [0]], 5, 1.0, 1.0, 30001))
        # hubs of thousands of edges (several pivot levels, the interpolation start)
        ph = EA.synth_params(31, 3000, 900000, n_types=1, weighted=True)
        po = O.SynthParams()
        for f, _ in po._fields_:
            setattr(po, f, getattr(ph, f))
        G2, OG2 = EA.Graph.synthetic(ph), O.OracleGraph(O.synth_csr(po))
        q2 = np.random.default_rng(4).integers(1, 3001, 9000).astype(np.int64)
        G2.set_seed(5)
        want2 = OG2.random_walk(5, 77, q2, [[0]] * 9, 9, 1.0, 1.0, 3001)
        for tail in (0, 4):
            L.euler_gpu_set_tuning(43, tail)
            got = G2.random_walk(torch.as_tensor(q2).cuda(), [[0]] * 9, 1.0, 1.0, 3001, call_id=77)
            assert np.array_equal(t2n(got), want2), tail
        frac = len(np.unique(t2n(got)[:, -1])) / len(q)
        assert frac < 0.5, frac          # the premise: walkers do merge on a power-law graph
    finally:
        L.euler_gpu_set_tuning(38, 262144)
        L.euler_gpu_set_tuning(43, 9)
        L.euler_gpu_set_tuning(44, 1)
        L.euler_gpu_set_tuning(45, 1)


def test_fanout_unique_rows_and_index(EA, O, torch_cuda, big_pair):
    """euler_gpu_sample_fanout_unique: the GQL result before DATA_GATHER - hop 2 as the
    distinct rows of every group of roots plus the row of each hop-1 sample.  rows[row_index]
    must be the dense hop-2 tensors of sample_fanout (== the oracle), weighted and uniform
    plain graphs, odd batch sizes, hub roots (several passes of slots); other graphs
    answer EINVAL (the caller uses the dense form)."""
    torch = torch_cuda
    from euler_amd import _lib
    for weighted in (True, False):
        p = EA.synth_params(977, 20000, 260000, n_types=1, weighted=weighted)
        po = O.SynthParams()
        for f, _ in po._fields_:
            setattr(po, f, getattr(p, f))
        G, OG = EA.Graph.synthetic(p), O.OracleGraph(O.synth_csr(po))
        q = np.concatenate([np.random.default_rng(5).integers(1, 20001, 5003), [0, 20001, 1, 1]])
        q = q.astype(np.int64)
        qt = torch.as_tensor(q).cuda()
        G.set_seed(3)
        for counts in ([25, 10], [3, 4], [7, 2]):
            on, ow, ot = OG.sample_fanout(3, 12, q, [[0], [0]], counts, 20001)
            id1, w1, t1, idx, rid, rw, rt = G.sample_fanout_unique(qt, [[0], [0]], counts, 20001,
                                                                   call_id=12)
            assert np.array_equal(t2n(id1).reshape(-1), on[0]) and np.array_equal(t2n(w1).reshape(-1), ow[0])
            assert np.array_equal(t2n(t1).reshape(-1), ot[0])
            assert np.array_equal(t2n(rid[idx]).reshape(-1), on[1]), (weighted, counts)
            assert np.array_equal(t2n(rw[idx]).reshape(-1), ow[1])
            assert np.array_equal(t2n(rt[idx]).reshape(-1), ot[1])
            # the point of the form: far fewer rows than positions
            assert len(np.unique(t2n(idx))) < 0.8 * idx.numel()
    G4, _OG4, ids4, rng = big_pair          # four edge-type groups: not served
    with pytest.raises(_lib.EulerGpuError):
        G4.sample_fanout_unique(torch.as_tensor(rng.choice(ids4, 100).astype(np.int64)).cuda(),
                                [[0], [1]], [4, 2], -1, call_id=1)


def test_sparse_adj_mask_and_triple(EA, O, torch_cuda, big_pair):
    """The two halves of SparseGetAdj on a sharded graph: euler_gpu_sparse_adj_mask (the hit
    mask of the sources a graph holds) + euler_gpu_sparse_adj_from_mask_tf (the TF triple
    from a mask) == euler_gpu_sparse_get_adj_tf == the oracle; masks of two disjoint shards
    OR to the mask of the whole graph."""
    torch = torch_cuda
    G, OG, ids, rng = big_pair
    for batch, n, m in ((1, 1, 1), (3, 4, 9), (2, 17, 70), (1, 40, 200), (4, 5, 130)):
        nodes = rng.choice(ids, (batch, n)).astype(np.uint64)
        nodes[0, 0] = 2 ** 62 + 5
        cand = rng.choice(ids, (batch, m)).astype(np.uint64)
        for b in range(batch):
            nb = OG.get_full_neighbor(nodes[b], [0, 1, 2, 3])[1]
            if len(nb):
                take = rng.choice(nb, m // 2 + 1)
                cand[b, :len(take)] = take[:m]
        nt = torch.as_tensor(nodes.view(np.int64)).cuda()
        ct = torch.as_tensor(cand.view(np.int64)).cuda()
        for et in ([0], [2, 1], [0, 1, 2, 3]):
            mask = G.sparse_adj_mask(nt, ct, batch, n, m, et)
            ind, val, shape = EA.Graph.adj_from_mask(mask, batch, n, m)
            wi, wv, ws = G.sparse_get_adj(nt, ct, et, n, m)
            assert torch.equal(ind, wi) and torch.equal(val, wv) and list(shape) == list(ws)
            want = OG.sparse_get_adj_tf(nodes, cand, et, n, m)
            assert np.array_equal(t2n(ind), want[0]) and np.array_equal(t2n(val), want[1])
