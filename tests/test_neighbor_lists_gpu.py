"""The neighbour-listing family on the GPU against the CPU oracle, bit for bit, on the cases of
neighbor_list_cases.py: get_full_neighbor with both fill kernels (and the balanced fill's
super-window path), neighbor_post_process at the 64 / 65 split and at limit 0 / limit >= len,
order_by id over keys at and above 2^63, get_top_k_neighbor in all three branches with ties
and zero weights, and the int32 limits of the count passes (refused, never wrapped).
test_neighbor_lists_host.py proves from the oracle alone that the cases reach those paths."""
import ctypes as C

import numpy as np
import pytest

import neighbor_list_cases as NC

pytestmark = pytest.mark.gpu


def gpu_graph(EA, csr):
    return EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w,
                             csr.type_prefix, csr.n_types, csr.node_type, csr.node_weight)


def t2n(t):
    return t.detach().cpu().numpy()


def same(got, want, what):
    """(idx, ids, w, t) or dense triples: bit-exact, ids as the same 64 bits, weights as uint32."""
    assert len(got) == len(want)
    for g, w_ in zip(got, want):
        g = t2n(g) if hasattr(g, "detach") else np.asarray(g)
        w_ = np.asarray(w_)
        if g.dtype == np.int64 and w_.dtype == np.uint64:
            g = g.view(np.uint64)
        if w_.dtype == np.float32:
            g, w_ = g.view(np.uint32), w_.view(np.uint32)
        assert g.dtype == w_.dtype and g.shape == w_.shape and np.array_equal(g, w_), what


@pytest.fixture(scope="module")
def case(EA, O, torch_cuda):
    c = NC.CaseGraph()
    csr = c.csr(O)
    return c, gpu_graph(EA, csr), O.OracleGraph(csr)


@pytest.fixture(scope="module")
def super_pair(EA, O, torch_cuda):
    b = NC.SuperGraph()
    csr = b.csr(O)
    return b, gpu_graph(EA, csr), O.OracleGraph(csr)


def dev(torch, q):
    return torch.as_tensor(NC.as_i64(q)).cuda()


# ---------------------------------------------------------------- A. both fill kernels
@pytest.mark.parametrize("et", list(NC.TYPE_LISTS) + [[], [9]], ids=str)
def test_full_neighbor_both_fills(EA, O, torch_cuda, case, et):
    from euler_amd import _lib
    c, G, OG = case
    queries = {"all": c.queries(), "one_empty": c.ids[c.rows_with(0, 0)][:1],
               "one_2049": c.ids[c.rows_with(2049, 0)][:1], "one_unknown": c.unknown[1:]}
    try:
        for name, q in queries.items():
            want = OG.get_full_neighbor(q, et)
            got = {}
            for mode in (1, 0):
                _lib.check(_lib.lib().euler_gpu_set_tuning(24, mode))
                got[mode] = G.get_full_neighbor(dev(torch_cuda, q), et)
                same(got[mode], want, (et, name, "balanced" if mode else "wave per node"))
            for x, y in zip(got[1], got[0]):
                assert torch_cuda.equal(x, y), (et, name)
    finally:
        _lib.lib().euler_gpu_set_tuning(24, 1)


# ---------------------------------------------------------------- B. the super-window path
def test_full_neighbor_super_windows(EA, O, torch_cuda, super_pair):
    """A call of over 32 << 20 entries: the balanced fill takes 8 windows per pair of row
    searches.  balanced == wave per node == oracle, compared on the device."""
    from euler_amd import _lib
    torch = torch_cuda
    b, G, OG = super_pair
    q = b.queries()
    want = OG.get_full_neighbor(q, [0, 1])
    assert int(want[0][-1, 1]) >= NC.SUPER_THRESHOLD
    want_dev = [torch.as_tensor(want[0]).cuda(), torch.as_tensor(want[1].view(np.int64)).cuda(),
                torch.as_tensor(want[2].view(np.int32)).cuda(), torch.as_tensor(want[3]).cuda()]
    qd = dev(torch, q)
    try:
        for mode in (1, 0):
            _lib.check(_lib.lib().euler_gpu_set_tuning(24, mode))
            gi, gd, gw, gt = G.get_full_neighbor(qd, [0, 1])
            assert gd.numel() == want[1].size
            assert torch.equal(gi, want_dev[0]), mode
            assert torch.equal(gd, want_dev[1]), mode
            assert torch.equal(gw.view(torch.int32), want_dev[2]), mode      # weights by their bits
            assert torch.equal(gt, want_dev[3]), mode
            del gi, gd, gw, gt
    finally:
        _lib.lib().euler_gpu_set_tuning(24, 1)


# ---------------------------------------------------------------- C. post-process
def _to_dense_gpu(torch, got, k, default_node):
    """euler_gpu_neighbor_to_dense: the C entry of the dense fill (it has no Python wrapper)."""
    from euler_amd import _lib
    from euler_amd.graph import _stream, _ptr
    idx, ids, w, t = got
    n = idx.shape[0]
    oi = torch.empty((n, k), dtype=torch.int64, device=idx.device)
    ow = torch.empty((n, k), dtype=torch.float32, device=idx.device)
    ot = torch.empty((n, k), dtype=torch.int32, device=idx.device)
    _lib.check(_lib.lib().euler_gpu_neighbor_to_dense(
        _stream(), n, _ptr(idx), _ptr(ids.contiguous()), _ptr(w.contiguous()), _ptr(t.contiguous()), k,
        default_node, _ptr(oi), _ptr(ow), _ptr(ot)))
    return oi, ow, ot


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("order_by", [None, "id", "weight"], ids=str)
def test_post_process(EA, O, torch_cuda, case, order_by, desc):
    c, G, OG = case
    for et, names in (([0, 1], ("short", "long", "mixed")), ([1, 0], ("mixed",))):
        batches = c.batches(et)
        for name in names:
            q = batches[name]
            qd = dev(torch_cuda, q)
            full = OG.get_full_neighbor(q, et)
            for limit in NC.LIMITS:
                what = (et, name, order_by, desc, limit)
                want = O.neighbor_post_process(*full, order_by=order_by, desc=desc, limit=limit)
                got = G.get_full_neighbor(qd, et, order_by=order_by, desc=desc, limit=limit)
                same(got, want, what)
                if limit in (2, 65):
                    k = limit + 1                      # one column of defaults in every row
                    same(_to_dense_gpu(torch_cuda, got, k, 261), O.neighbor_to_dense(*want, k, 261), what)


# ---------------------------------------------------------------- D. top-k
@pytest.mark.parametrize("et", NC.TYPE_LISTS, ids=str)
def test_top_k_neighbor(EA, O, torch_cuda, case, et):
    c, G, OG = case
    q = c.queries()
    qd = dev(torch_cuda, q)
    full = OG.get_full_neighbor(q, et)
    for k in NC.TOP_KS:
        top = O.neighbor_post_process(*full, order_by="weight", desc=True, limit=k)
        for default_node in (-1, 261):
            want = O.neighbor_to_dense(*top, k, default_node)
            got = G.get_top_k_neighbor(qd, et, k, default_node=default_node)
            same(got, want, (et, k, default_node))


def test_top_k_neighbor_no_listed_type(EA, O, torch_cuda, case):
    """[] and an unknown type list nothing: every row is defaults."""
    c, G, OG = case
    q = c.queries()
    for et in ([], [9]):
        full = OG.get_full_neighbor(q, et)
        want = O.neighbor_to_dense(*O.neighbor_post_process(*full, order_by="weight", desc=True, limit=8),
                                   8, 261)
        same(G.get_top_k_neighbor(dev(torch_cuda, q), et, 8, default_node=261), want, et)


# ---------------------------------------------------------------- E. int32 limits
def test_full_neighbor_refuses_totals_past_int32(EA, O, torch_cuda, super_pair):
    """A total of 2^31 entries or more does not fit the int32 idx pairs: the count pass says so
    (as neighbor_post_process does) instead of handing back a wrapped total.  Count passes
    only: the wrapper is not called before the C entry has been seen to refuse."""
    from euler_amd import _lib
    from euler_amd.graph import _stream, _ptr
    torch = torch_cuda
    b, G, OG = super_pair
    et = (C.c_int32 * 1)(0)
    for reps in (2049, 4097):                 # int32 would wrap negative / to a small positive total
        q = dev(torch, np.repeat(b.hub[:1], reps))
        idx = torch.empty((reps, 2), dtype=torch.int32, device="cuda")
        total = C.c_int64(-7)
        rc = _lib.lib().euler_gpu_get_full_neighbor(G._h, _stream(), _ptr(q), reps, et, 1, _ptr(idx),
                                                    C.byref(total), None, None, None)
        assert rc == _lib.EINVAL, (reps, rc, total.value)
        assert "2^31" in _lib.lib().euler_gpu_last_error().decode()
        assert total.value == -7
    for reps in (2049, 4097):
        with pytest.raises(_lib.EulerGpuError, match="2\\^31"):
            G.get_full_neighbor(dev(torch, np.repeat(b.hub[:1], reps)), [0])
    # just under the limit is still counted right (count pass only: 2047 * (2^20 + 3) + ...)
    reps = 2047
    q = dev(torch, np.repeat(b.hub[:1], reps))
    idx = torch.empty((reps, 2), dtype=torch.int32, device="cuda")
    total = C.c_int64(0)
    _lib.check(_lib.lib().euler_gpu_get_full_neighbor(G._h, _stream(), _ptr(q), reps, et, 1, _ptr(idx),
                                                      C.byref(total), None, None, None))
    assert total.value == reps * NC.HUB_ENTRIES < 2 ** 31
    assert t2n(idx[-1]).tolist() == [(reps - 1) * NC.HUB_ENTRIES, reps * NC.HUB_ENTRIES]


def test_idx_gather_refuses_totals_past_int32(EA, O, torch_cuda):
    from euler_amd import _lib
    torch, ops = torch_cuda, EA.ops
    idx = torch.tensor([[0, 2 ** 20]], dtype=torch.int32, device="cuda")
    for reps in (2049, 4097):
        gi = torch.zeros(reps, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.EulerGpuError, match="2\\^31"):
            ops.idx_gather(idx, gi)
    # (only now: with the count pass refusing, data_gather stops before its kernel)
    data = torch.zeros(2 ** 20, dtype=torch.uint8, device="cuda")
    for reps in (2049, 4097):
        gi = torch.zeros(reps, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.EulerGpuError, match="2\\^31"):
            ops.data_gather(data, idx, gi)
    # 2^31 - 1 exactly is still answered: 2048 times a row of 2^20 - 1 and one of 2047
    idx = np.array([[0, 2 ** 20 - 1], [2 ** 20 - 1, 2 ** 20 - 1 + 2047]], np.int32)
    gi = np.concatenate([np.zeros(2048, np.int32), np.ones(1, np.int32)])
    out, total = ops.idx_gather(torch.as_tensor(idx).cuda(), torch.as_tensor(gi).cuda())
    assert total == 2 ** 31 - 1
    assert np.array_equal(t2n(out), O.idx_gather(idx, gi))


def test_inflate_idx_range_check_before_narrowing(EA, O, torch_cuda):
    torch, ops = torch_cuda, EA.ops
    for bad in ([0, 1, 2 ** 32 + 1], [0, 1, -2 ** 32], [2 ** 32, 2 ** 32 + 1]):
        with pytest.raises(ValueError, match="unique_cnt"):
            O.inflate_idx(np.asarray(bad, np.int64))
        with pytest.raises(ValueError, match="unique_cnt"):
            ops.inflate_idx(torch.tensor(bad, dtype=torch.int64, device="cuda"))
    good = np.array([2, 0, 1, 0, 2, 2, 1, 0], np.int64)
    want = O.inflate_idx(good)
    for dt in (torch.int64, torch.int32):
        got = ops.inflate_idx(torch.as_tensor(good).to(dt).cuda())
        assert got.dtype == torch.int32 and np.array_equal(t2n(got), want)
    assert ops.inflate_idx(torch.zeros(0, dtype=torch.int64, device="cuda")).numel() == 0
    with pytest.raises(ValueError, match="unique_cnt"):       # in int32 range, outside [0, U)
        ops.inflate_idx(torch.tensor([0, 1, 3], dtype=torch.int64, device="cuda"))
