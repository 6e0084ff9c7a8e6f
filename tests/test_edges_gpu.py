"""GPU checks of the edge store: edge lookups and edge / binary features on the fixture
(Graph.load(edges=True) and euler_ops), SampleEdge against the oracle's SampleNode restatement
(the reference draws both from one generator), and a synthetic graph at scale."""
import os
import shutil

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import euler_amd
    g = euler_amd.Graph.load(FIXTURE, edges=True)
    yield g
    g.close()


def test_fixture_edge_features(G):
    assert G.num_edge_records == 12
    edges = [[1, 2, 0], [2, 3, 1], [7, 8, 0], [1, 2, 1]]
    ords = G.edge_ordinals(edges).cpu().numpy()
    assert ords[0] >= 0 and ords[1] >= 0 and ords[2] == -1 and ords[3] == -1
    d3, d4 = G.get_edge_dense_feature(edges, [0, 1], [2, 3])
    assert np.allclose(d3.cpu().numpy(), [[12.1, 12.2], [23.1, 23.2], [0, 0], [0, 0]])
    assert np.allclose(d4.cpu().numpy()[0], [12.3, 12.4, 12.5])
    assert not d4.cpu().numpy()[2:].any()
    (i1, v1, s1), (i2, v2, s2) = G.get_edge_sparse_feature(edges, [0, 1], [-7, -7])
    rows = i1.cpu().numpy()[:, 0]
    assert v1.cpu().numpy()[rows == 0].tolist() == [121, 122]
    assert v2.cpu().numpy()[i2.cpu().numpy()[:, 0] == 0].tolist() == [123, 124]
    assert v1.cpu().numpy()[rows == 2].tolist() == [-7]
    (off, data), = G.get_edge_binary_feature(edges, [0])
    o, b = off.cpu().numpy(), data.cpu().numpy().tobytes()
    assert [b[o[i]:o[i + 1]] for i in range(4)] == [b"12a", b"23a", b"", b""]
    (off, data), = G.get_binary_feature([1, 2, 99], [1])
    o, b = off.cpu().numpy(), data.cpu().numpy().tobytes()
    assert [b[o[i]:o[i + 1]] for i in range(3)] == [b"1b", b"2b", b""]


def test_fixture_through_euler_ops():
    from euler_amd import euler_ops
    from euler_amd.euler_ops import feature_ops, sample_ops
    assert euler_ops.initialize_embedded_graph(FIXTURE)
    try:
        edges = np.array([[1, 2, 0], [2, 3, 1], [9, 9, 0]], np.int64)
        f3, = feature_ops.get_edge_dense_feature(edges, ["f3"], [2])
        assert np.allclose(f3.cpu().numpy(), [[12.1, 12.2], [23.1, 23.2], [0, 0]])
        (_, v, _), = feature_ops.get_edge_sparse_feature(edges[:1], ["f1"])
        assert v.cpu().numpy().tolist() == [121, 122]
        f5, = feature_ops.get_edge_binary_feature(edges, ["f5"])
        assert f5 == [b"12a", b"23a", b""]
        f5n, f6n = feature_ops.get_binary_feature([1, 2], ["f5", "f6"])
        assert f5n == [b"1a", b"2a"] and f6n == [b"1b", b"2b"]
        with pytest.raises(Exception):
            feature_ops.get_edge_dense_feature(edges, ["nope"], [2])
        euler_ops.set_seed(3)
        s = sample_ops.sample_edge(10, '1').cpu().numpy()
        assert s.shape == (10, 3) and set(s[:, 1].tolist()) <= {1, 3, 5}
        assert set(s[:, 2].tolist()) == {1}
    finally:
        euler_ops.set_default_graph(None)


def test_node_only_directory_loads_node_only(tmp_path):
    import euler_amd
    d = tmp_path / "nodes_only"
    shutil.copytree(FIXTURE, d)
    shutil.rmtree(d / "Edge")
    a = euler_amd.Graph.load(FIXTURE)
    b = euler_amd.Graph.load(str(d))
    assert a.num_edge_records == -1 and b.num_edge_records == -1
    assert a.device_bytes == b.device_bytes
    # the node binary features are not on the device until the first call that reads them
    bytes0 = b.device_bytes
    (off, data), = b.get_binary_feature([1], [0])
    assert bytes(data.cpu().numpy()) == b"1a"
    bytes1 = b.device_bytes
    assert bytes1 > bytes0
    b.get_binary_feature([2], [1])
    assert b.device_bytes == bytes1
    e = euler_amd.Graph.load(FIXTURE, edges=True)
    assert e.device_bytes > a.device_bytes
    with pytest.raises(Exception):
        b.sample_edge(4, 0)
    from euler_amd import euler_ops
    assert euler_ops.initialize_embedded_graph(str(d))
    try:
        assert euler_ops.get_default_graph().num_edge_records == -1
    finally:
        euler_ops.set_default_graph(None)


def oracle_sample_edge(records, order, seed, call_id, types, count):
    """The oracle's SampleNode over ids = ordinals, mapped through the record table."""
    from oracle import oracle as O
    src, dst, ty, w = records
    order = np.asarray(order, np.int64)
    ids = order.astype(np.uint64)
    tt = ty[order].astype(np.int32)
    ww = w[order].astype(np.float32)
    L = O.lib()
    s = L.eo_node_sampler_create(len(ids), O._p(ids, O._u64p), O._p(tt, O._i32p),
                                 O._p(ww, O._f32p), int(ty.max()) + 1)
    try:
        nt = np.atleast_1d(np.asarray(types, np.int32))
        out = np.zeros(max(count, 1), np.uint64)
        got = L.eo_sample_node(s, seed, call_id, O._p(nt, O._i32p), len(nt), count,
                               O._p(out, O._u64p))
    finally:
        L.eo_node_sampler_destroy(s)
    o = out[:max(got, 0)].astype(np.int64)
    return np.stack([src[o].astype(np.int64), dst[o].astype(np.int64), ty[o].astype(np.int64)], 1)


def check_parity(G, seed, types_list, counts, order=None):
    recs = G.export_edges()
    if order is None:
        order = np.arange(len(recs[0]))
    G.set_seed(seed)
    for c, types in enumerate(types_list):
        for count in counts:
            got = G.sample_edge(count, types, call_id=c).cpu().numpy()
            want = oracle_sample_edge(recs, order, seed, c, types, count)
            assert got.shape == (count, 3)
            assert np.array_equal(got, want), (types, count)


def test_sample_edge_parity_fixture(G):
    check_parity(G, 11, [0, 1, -1, [0, 1]], [0, 1, 7, 1001])
    order = np.random.default_rng(1).permutation(G.num_edge_records)
    G.set_edge_sampler(order)
    try:
        check_parity(G, 12, [0, -1, [1, 0]], [1, 333], order=order)
    finally:
        G.set_edge_sampler()


def test_sample_edge_zero_weight_type_is_empty():
    import euler_amd
    from euler_amd import _lib
    g = euler_amd.Graph.load(FIXTURE)
    g.set_edges([1, 2, 3], [2, 3, 4], [0, 1, 1], [1.0, 0.0, 0.0])
    out = torch.full((4, 3), 77, dtype=torch.int64, device="cuda")
    rc = _lib.lib().euler_gpu_sample_edge(g._h, None, 0, 0, (_lib.C.c_int32 * 1)(1), 1, 4,
                                          _lib.C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    assert rc == _lib.EEMPTY and (out == 77).all()
    assert g.sample_edge(3, 0).cpu().numpy().tolist() == [[1, 2, 0]] * 3
    with pytest.raises(_lib.EulerGpuError):            # repeated triple
        g.set_edges([1, 1], [2, 2], [0, 0], [1.0, 1.0])
    assert g.num_edge_records == 3                     # the failed build left the store alone


def synth(n_nodes, n_edges, n_types, seed):
    import euler_amd
    from oracle import oracle as O
    p = euler_amd.synth_params(seed, n_nodes, n_edges, n_types=n_types, weighted=True)
    po = O.SynthParams()
    for f, _ in po._fields_:
        setattr(po, f, getattr(p, f))
    return p, O.synth_csr(po, threads=16)


def host_records(c):
    """First-occurrence dedup of the CSR's (src, dst, type) entries in row / entry order."""
    n, T = c.n_rows, c.n_types
    deg = np.diff(c.row_ptr)
    src = np.repeat(c.row_id, deg)
    te = c.type_end.reshape(n, T).astype(np.int64)
    pos = np.arange(len(c.nbr)) - np.repeat(c.row_ptr[:-1], deg)
    ty = np.zeros(len(c.nbr), np.int32)
    for t in range(T - 1):
        ty += (pos >= np.repeat(te[:, t], deg)).astype(np.int32)
    prev = np.concatenate([[0.0], c.prefix_w[:-1]]).astype(np.float32)
    prev[c.row_ptr[:-1][deg > 0]] = 0.0
    w = (c.prefix_w - prev).astype(np.float32)
    key = np.stack([src, c.nbr, ty.astype(np.uint64)], 1)
    _, first = np.unique(key, axis=0, return_index=True)
    first.sort()
    return src[first], c.nbr[first], ty[first], w[first]


def test_sample_edge_parity_synthetic():
    import euler_amd
    p, c = synth(300_000, 5_000_000, 3, 77)
    G = euler_amd.Graph.synthetic(p)
    G.edges_from_rows()
    recs = G.export_edges()
    want = host_records(c)
    for a, b in zip(recs, want):
        assert np.array_equal(a, b)
    check_parity(G, 5, [1, -1, [0, 2, 1]], [0, 1, 99_999])


def test_edges_at_scale():
    import euler_amd
    p, c = synth(4_000_000, 50_000_000, 2, 2024)
    assert len(c.nbr) >= 50_000_000
    G = euler_amd.Graph.synthetic(p)
    G.edges_from_rows()
    src, dst, ty, w = G.export_edges()
    want = host_records(c)
    for a, b in zip((src, dst, ty, w), want):
        assert np.array_equal(a, b)
    n = len(src)
    G.close()
    # the same records with features, from host arrays
    G = euler_amd.Graph.synthetic(p)
    bytes0 = G.device_bytes
    rng = np.random.default_rng(5)
    dense = rng.standard_normal((n, 4)).astype(np.float32)
    sparse = rng.integers(0, 1 << 40, (n, 2)).astype(np.uint64)
    binary = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    G.set_edges(src, dst, ty, w, dense=[dense], sparse=[sparse], binary=[binary])
    feat_bytes = dense.nbytes + sparse.nbytes + binary.nbytes
    assert G.device_bytes - bytes0 <= 112 * n + feat_bytes + 4096
    q = rng.integers(0, n, 1_000_000)
    edges = np.stack([src[q].astype(np.int64), dst[q].astype(np.int64), ty[q].astype(np.int64)], 1)
    miss = rng.random(len(q)) < 0.1
    edges[miss, 1] = -5 - np.arange(miss.sum())          # no such dst
    ords = G.edge_ordinals(edges).cpu().numpy()
    assert np.array_equal(ords, np.where(miss, -1, q))
    d, = G.get_edge_dense_feature(edges, [0], [4])
    assert np.array_equal(d.cpu().numpy(), np.where(miss[:, None], 0, dense[q]))
    (ind, val, shape), = G.get_edge_sparse_feature(edges, [0], [-1])
    vals = val.cpu().numpy()
    rows = ind.cpu().numpy()[:, 0]
    want_vals = np.where(miss[:, None], -1, sparse[q].astype(np.int64))
    assert np.array_equal(vals[np.isin(rows, np.where(~miss)[0])], want_vals[~miss].reshape(-1))
    assert np.array_equal(vals[np.isin(rows, np.where(miss)[0])], np.full(miss.sum(), -1))
    (off, data), = G.get_edge_binary_feature(edges, [0])
    o = off.cpu().numpy()
    assert np.array_equal(np.diff(o), np.where(miss, 0, 3))
    assert np.array_equal(data.cpu().numpy(), binary[q[~miss]].reshape(-1))
    G.close()


K_INT32 = 2                          # euler::DataType (core/framework/types.h:26-39)


def run_query(L, gremlin, inputs, result, capacity):
    """euler::Query with int32 inputs (name, value or array); int64 result of `capacity`."""
    import ctypes as C
    n = len(inputs)
    names = (C.c_char_p * n)(*[nm.encode() for nm, _ in inputs])
    dts = (C.c_int32 * n)(*[K_INT32] * n)
    arrs = [np.atleast_1d(np.asarray(v, np.int32)) for _, v in inputs]
    cnt = (C.c_int64 * n)(*[-1 if np.isscalar(v) else len(a) for (_, v), a in zip(inputs, arrs)])
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    out = np.zeros(max(capacity, 1), np.int64)
    rc = L.euler_query_run(gremlin.encode(), n, names, dts, cnt, ptrs, result.encode(),
                           out.ctypes.data_as(C.c_void_p), out.nbytes)
    return rc, (out[:rc // 8] if rc >= 0 else None)


def test_sample_edge_op_and_query(G):
    """tf_euler/kernels/sample_edge_op.cc:56 builds sampleE(edge_type, count).as(eid): the shim
    runs API_SAMPLE_EDGE of the plugin-API registry, which equals the C ABI call."""
    from euler_amd import _lib
    L = _lib.lib()
    assert L.euler_op_registered(b"API_SAMPLE_EDGE") == 1
    L.euler_query_set_graph(G._h)
    for seed, types in ((31, 1), (32, [0, 1]), (33, -1)):
        L.euler_query_set_seed(seed)
        rc, got = run_query(L, "sampleE(edge_type, count).as(eid)",
                            [("edge_type", types), ("count", 257)], "eid:0", 257 * 3)
        assert rc == 257 * 3 * 8
        G.set_seed(seed)
        want = G.sample_edge(257, types, call_id=0).cpu().numpy().reshape(-1)
        assert np.array_equal(got, want)
    # failures (a type out of range, a type of zero weight) leave no output
    L.euler_query_set_seed(1)
    rc, _ = run_query(L, "sampleE(edge_type, count).as(eid)",
                      [("edge_type", 5), ("count", 8)], "eid:0", 24)
    assert rc == -1
    rc, _ = run_query(L, "sampleE(edge_type).as(eid)", [("edge_type", 0)], "eid:0", 24)
    assert rc == -1


def test_init_query_proxy_refuses_malformed_edges(tmp_path):
    from euler_amd import euler_ops
    d = tmp_path / "bad_edges"
    shutil.copytree(FIXTURE, d)
    f = d / "Edge" / "data_0.dat"
    f.write_bytes(f.read_bytes()[:-5])
    try:
        assert not euler_ops.initialize_graph({"mode": "local", "data_path": str(d),
                                               "data_type": "all"})
        assert not euler_ops.initialize_graph({"mode": "local", "data_path": str(d),
                                               "data_type": "edge"})
        # without data_type (or data_type node) the Edge records are not read: node-only
        assert euler_ops.initialize_graph({"mode": "local", "data_path": str(d)})
        assert euler_ops.get_default_graph().num_edge_records == -1
        assert euler_ops.initialize_graph({"mode": "local", "data_path": str(d),
                                           "data_type": "node"})
        assert euler_ops.get_default_graph().num_edge_records == -1
    finally:
        euler_ops.set_default_graph(None)
