"""GPU checks of graph labels: the label index, SampleGraphLabel and
GetGraphByLabel against the numpy restatement (tests/graph_label_ref.py), the whole-graph block
against SparseGetAdj, forced hash collisions, the byte budget and the error paths."""
import os

import numpy as np
import pytest
import torch

import graph_label_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")


def block_oracle(G, n_id, et, loops=True):
    ind, val, _ = G.sparse_get_adj(n_id, n_id, et)
    return R.block_from_adj(ind.cpu().numpy(), val.cpu().numpy(), len(n_id), loops)


def check_graph(G, ids, labels, batch_labels):
    table, nodes = R.label_table(ids, labels)
    assert G.graph_labels() == table
    assert G.num_graph_labels == len(table)
    ind, val, shape = G.get_graph_by_label(batch_labels)
    want = R.graph_by_label(table, nodes, batch_labels)
    assert np.array_equal(ind.cpu().numpy(), want[0])
    assert np.array_equal(val.cpu().numpy(), want[1])
    assert shape == want[2]
    return table, nodes


def test_fixture_labels_and_ops():
    import euler_amd
    G = euler_amd.Graph.load(FIXTURE)
    b0 = G.device_bytes
    ids = list(range(1, 7))
    check_graph(G, ids, [str(i) for i in ids], ['1', '2', '3', 'nope', '2'])
    assert G.device_bytes > b0
    for seed, call_id in ((0, 0), (7, 3), (2**40 + 1, 11)):
        G.set_seed(seed)
        for count in (0, 1, 7, 100_000):
            got = G.sample_graph_label(count, call_id=call_id).cpu().numpy()
            assert np.array_equal(got, R.sample_graph_label(seed, call_id, count, 6))
            if count == 100_000:
                assert set(got.tolist()) == set(range(6))
    n_id = torch.tensor([1, 2, 3, 4, 5, 6, 2, 99, 1], device="cuda")
    for et in ([0], [1], [0, 1], [], [7]):
        got = G.whole_graph_block(n_id, et).cpu().numpy()
        assert np.array_equal(got, block_oracle(G, n_id, et)), et
    got = G.whole_graph_block(n_id, [0, 1], add_self_loops=False).cpu().numpy()
    assert np.array_equal(got, block_oracle(G, n_id, [0, 1], False))


def test_fixture_through_euler_ops():
    from euler_amd import euler_ops
    from euler_amd.euler_ops import sample_ops
    assert euler_ops.initialize_embedded_graph(FIXTURE)
    try:
        G = euler_ops.base.get_default_graph()
        assert G.graph_labels() == [str(i) for i in range(1, 7)]
        euler_ops.set_seed(5)
        s = sample_ops.sample_graph_label(50)
        assert len(s) == 50 and set(s) <= {str(i) for i in range(1, 7)}
        ind, val, shape = sample_ops.get_graph_by_label(['6', 'x'])
        assert ind.cpu().tolist() == [[0, 0], [1, 0]] and val.cpu().tolist() == [6, 0]
        assert shape == [2, 1]
    finally:
        euler_ops.set_default_graph(None)


@pytest.fixture(scope="module")
def big():
    import euler_amd
    kw, ids, labels, _ = R.multigraph_csr(100_000, 17)
    G = euler_amd.Graph.from_csr(**kw)
    b0 = G.device_bytes
    G.set_graph_labels(ids, labels)
    return G, ids, labels, b0


def test_synthetic_at_scale(big):
    G, ids, labels, b0 = big
    table, nodes = R.label_table(ids, labels)
    assert len(table) >= 99_000
    rng = np.random.default_rng(3)
    batch = [table[i] for i in rng.integers(0, len(table), 512)]
    batch[5] = batch[9]                                    # a graph twice
    batch[7] = "no such graph"
    check_graph(G, ids, labels, batch)
    # byte budget: <= 16 B per labelled node + 64 B per label + the label bytes
    n_lab, nbytes = G.label_index_info()
    assert n_lab == sum(len(x) for x in nodes)
    label_bytes = sum(len(x) for x in table)
    assert nbytes <= 16 * n_lab + 64 * len(table) + label_bytes
    assert G.device_bytes - b0 == nbytes
    # the block against SparseGetAdj on the batch's nodes (hub rows included)
    _, n_id = G.get_graph_by_label_core(batch)
    for et in ([0], [0, 1]):
        got = G.whole_graph_block(n_id, et).cpu().numpy()
        assert np.array_equal(got, block_oracle(G, n_id, et))


def test_hubs_in_block():
    import euler_amd
    kw, ids, labels, (src, nbr, deg) = R.multigraph_csr(300, 5, n_hubs=4, hub_degree=20_000, cross=0.5)
    G = euler_amd.Graph.from_csr(**kw)
    G.set_graph_labels(ids, labels)
    hubs = np.nonzero(deg[:, 0] == 20_000)[0]
    n_id = torch.as_tensor(np.concatenate([ids[hubs], ids[: 4000], ids[hubs]]).astype(np.int64)).cuda()
    for et in ([0], [1, 0]):
        got = G.whole_graph_block(n_id, et).cpu().numpy()
        assert np.array_equal(got, block_oracle(G, n_id, et))


def test_collisions_give_the_same_index():
    import euler_amd
    from euler_amd._lib import lib
    kw, ids, labels, _ = R.multigraph_csr(100_000, 29)
    G = euler_amd.Graph.from_csr(**kw)
    G.set_graph_labels(ids, labels)
    want = G.graph_labels()
    _, want_nodes = G.get_graph_by_label_core(list(range(0, len(want), 97)))
    assert lib().euler_gpu_set_tuning(74, 4) == 0
    try:
        H = euler_amd.Graph.from_csr(**kw)
        H.set_graph_labels(ids, labels)
        assert H.graph_labels() == want
        _, got_nodes = H.get_graph_by_label_core(list(range(0, len(want), 97)))
        assert torch.equal(got_nodes, want_nodes)
    finally:
        lib().euler_gpu_set_tuning(74, 64)


def test_errors_and_release():
    import euler_amd
    from euler_amd._lib import EulerGpuError, EEMPTY, EINVAL
    kw, ids, labels, _ = R.multigraph_csr(50, 3)
    G = euler_amd.Graph.from_csr(**kw)
    b0 = G.device_bytes
    with pytest.raises(EulerGpuError) as e:
        G.sample_graph_label(3)
    assert e.value.code == EEMPTY
    assert G.num_graph_labels == 0
    G.set_graph_labels(ids, labels)
    before = G.graph_labels()
    with pytest.raises(EulerGpuError) as e:
        G.set_graph_labels(np.append(ids, 10**9), labels + ["x"])
    assert e.value.code == EINVAL
    assert G.graph_labels() == before                       # the old index stays
    assert G.device_bytes > b0
    G.set_graph_labels([], [])
    assert G.num_graph_labels == 0 and G.device_bytes == b0
    S = euler_amd.Graph.synthetic(euler_amd.synth_params(1, 1000, 5000), partitions=2,
                                  shard_index=0, shards=2)
    with pytest.raises(EulerGpuError) as e:
        S.set_graph_labels([2, 4], ["a", "b"])
    assert e.value.code == EINVAL
    G.close()


def test_sharded_load_refuses_labels():
    import euler_amd
    from euler_amd._lib import EulerGpuError, EINVAL
    S = euler_amd.Graph.load(FIXTURE, shard_index=0, shards=2)
    b0 = S.device_bytes
    for call in (S.graph_labels, lambda: S.sample_graph_label(4), lambda: S.get_graph_by_label(['1'])):
        with pytest.raises(EulerGpuError) as e:
            call()
        assert e.value.code == EINVAL
    assert S.device_bytes == b0


def test_graph_batch_with_unknown_labels_follows_the_triple():
    import euler_amd
    G = euler_amd.Graph.load(FIXTURE)
    lab, n_id, gidx, ei = G.graph_batch(['2', 'nope', '5'], [0, 1])
    assert lab.cpu().tolist() == [1, -1, 4]
    assert n_id.cpu().tolist() == [2, 0, 5] and gidx.cpu().tolist() == [0, 1, 2]
    assert torch.equal(ei, G.whole_graph_block(n_id, [0, 1]))


# ---- the plugin ops and the single-op euler::Query (C++ / TF hosts)
K_INT32, K_UINT64, K_STRING = 2, 7, 11         # euler::DataType (core/framework/types.h:26-39)


def run_op_query(L, op, alias, output_num, inputs, attrs, result, capacity):
    """euler::Query(op, alias, output_num, input names, attr names) with tensors built as the TF
    kernels build them; (name, dtype, values) each, kString values as a list of str."""
    import ctypes as C
    tensors = inputs + attrs
    n = len(tensors)
    names = (C.c_char_p * n)(*[nm.encode() for nm, _, _ in tensors])
    dts = (C.c_int32 * n)(*[dt for _, dt, _ in tensors])
    keep, ptrs, cnts = [], [], []
    for _, dt, v in tensors:
        if dt == K_STRING:
            arr = (C.c_char_p * max(len(v), 1))(*[x.encode() for x in v])
            keep.append(arr)
            ptrs.append(C.cast(arr, C.c_void_p).value)
            cnts.append(len(v))
        else:
            a = np.ascontiguousarray(np.asarray(v, np.int32 if dt == K_INT32 else np.uint64).reshape(-1))
            keep.append(a)
            ptrs.append(a.ctypes.data)
            cnts.append(a.size)
    out = np.zeros(max(capacity, 1), np.uint8)
    rc = L.euler_query_run_op(op.encode(), alias.encode(), output_num, len(inputs), len(attrs), names,
                              dts, (C.c_int64 * n)(*cnts), (C.c_void_p * n)(*ptrs), result.encode(),
                              out.ctypes.data_as(C.c_void_p), out.nbytes)
    return rc, (out[:rc].tobytes() if rc >= 0 else None)


def test_label_ops_through_registry_and_single_op_query():
    import euler_amd
    from euler_amd import _lib
    L = _lib.lib()
    assert L.euler_op_registered(b"API_SAMPLE_GRAPH_LABEL") == 1
    assert L.euler_op_registered(b"API_GET_GRAPH_BY_LABEL") == 1
    G = euler_amd.Graph.load(FIXTURE)
    table = G.graph_labels()
    L.euler_query_set_graph(G._h)
    try:
        # tf_euler/kernels/sample_graph_label_op.cc:47
        for seed, count in ((3, 1), (4, 257), (5, 0)):
            L.euler_query_set_seed(seed)
            rc, got = run_op_query(L, "API_SAMPLE_GRAPH_LABEL", "sample_graph", 1,
                                   [("count", K_INT32, [count])], [], "sample_graph:0", 4096)
            assert rc >= 0
            G.set_seed(seed)
            want = [table[i] for i in G.sample_graph_label(count, call_id=0).cpu().tolist()]
            assert (got.decode().split(",") if count else []) == want
        # tf_euler/kernels/get_graph_by_label_op.cc:43 with a kString input
        labels = ['3', 'nope', '1', '3']
        rc, idx = run_op_query(L, "API_GET_GRAPH_BY_LABEL", "graphs", 2,
                               [("labels", K_STRING, labels)], [], "graphs:0", 4096)
        rc1, ids = run_op_query(L, "API_GET_GRAPH_BY_LABEL", "graphs", 2,
                                [("labels", K_STRING, labels)], [], "graphs:1", 4096)
        want_idx, want_ids = G.get_graph_by_label_core(labels)
        assert np.frombuffer(idx, np.int32).tolist() == want_idx.cpu().reshape(-1).tolist()
        assert np.frombuffer(ids, np.uint64).tolist() == want_ids.cpu().tolist()
        # tf_euler/kernels/sparse_get_adj_op.cc:58: inputs then norm attrs, in that order
        nodes = np.array([1, 2, 3, 4, 5, 6], np.uint64)
        nb = np.array([2, 3, 4, 1, 5, 6], np.uint64)
        n, m, batch = 3, 3, 2
        rb = np.stack([nodes, np.repeat(np.arange(batch), n).astype(np.uint64)], 1)
        for et in ([0], [0, 1]):
            got = [run_op_query(L, "API_SPARSE_GET_ADJ", "get_adj", 2,
                                [("root_batch", K_UINT64, rb), ("l_nb", K_UINT64, nb)],
                                [("edge_types", K_INT32, et), ("m", K_INT32, [m])], "get_adj:%d" % i,
                                4096) for i in (0, 1)]
            want_idx, want_ids = G.sparse_get_adj_core(nodes.astype(np.int64), nb.astype(np.int64),
                                                       n, m, et)
            assert np.frombuffer(got[0][1], np.int32).tolist() == want_idx.cpu().reshape(-1).tolist()
            assert np.frombuffer(got[1][1], np.uint64).tolist() == want_ids.cpu().tolist()
        # a graph without labels: the ops log and leave no output
        kw, _, _, _ = R.multigraph_csr(20, 1)
        H = euler_amd.Graph.from_csr(**kw)
        L.euler_query_set_graph(H._h)
        rc, _ = run_op_query(L, "API_SAMPLE_GRAPH_LABEL", "sample_graph", 1,
                             [("count", K_INT32, [4])], [], "sample_graph:0", 4096)
        assert rc == -1
        rc, _ = run_op_query(L, "API_GET_GRAPH_BY_LABEL", "graphs", 2,
                             [("labels", K_STRING, ['1'])], [], "graphs:0", 4096)
        assert rc == -1
    finally:
        L.euler_query_set_graph(None)


def test_dataflow_and_graph_batch_match_composition():
    import euler_amd
    from euler_amd.dataflow import WholeGraphDataFlow
    kw, ids, labels, _ = R.multigraph_csr(188, 11, min_nodes=12, max_nodes=24)
    G = euler_amd.Graph.from_csr(**kw)
    G.set_graph_labels(ids, labels)
    G.set_seed(9)
    lab, n_id, gidx, ei = G.graph_batch(128, [0, 1], call_id=4)
    want_lab = G.sample_graph_label(128, call_id=4)
    assert torch.equal(lab, want_lab)
    ind, val, _ = G.get_graph_by_label(want_lab)
    assert torch.equal(n_id, val) and torch.equal(gidx, ind[:, 0])
    flow = WholeGraphDataFlow(G, [[0, 1], [0, 1]])(n_id)
    assert len(flow) == 2
    for blk in flow.blocks:
        assert torch.equal(blk.edge_index, ei)
    assert torch.equal(ei, G.whole_graph_block(n_id, [0, 1]))


def test_example_runs():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python",
                                                     "graph_classification_minibatch.py")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ok" in r.stdout
