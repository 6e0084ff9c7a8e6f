"""The kernels that move node and edge features to the device, against tests/feature_ref.py on
ragged tables: euler_gpu_get_dense_feature, _get_sparse_feature, _get_sparse_feature_core,
_get_binary_feature, euler_gpu_edge_ordinals and _get_edge_{dense,sparse,binary}_feature.  All of
it is data movement: every comparison is exact.

The graphs are small (hundreds of nodes, 20 000 edge records); the large numbers are QUERY counts,
chosen above the sizes at which a launch of 4096 blocks x 256 threads starts its grid-stride loop:
1 048 576 for a lane per query, 16 384 for a wave per query, 131 072 for an 8-lane group per
query, 1 048 576 elements for the dense lane-per-element kernels (x 4 floats on the 16-byte path).
"""
import ctypes as C

import numpy as np
import pytest

import dat_write
import feature_cases as FC
import feature_ref as FR

pytestmark = pytest.mark.gpu

N_NODES = 700
N_EDGES = 20_000
DIMS = (1, 3, 4, 5, 8, 64, 65, 301)
DEFAULTS = (0, -1, 2 ** 62)


def t2n(t):
    return t.detach().cpu().numpy()


def bits(a):
    """float32 compared by bit pattern"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def chain_graph(EA, O, ids, **kw):
    """Every node with one out-edge to the next; the features are what the tests are about."""
    n = len(ids)
    c = O.csr_from_raw(ids, np.arange(n + 1, dtype=np.int64), np.roll(ids, -1),
                       np.ones(n, np.float32), 1)
    return EA.Graph.from_csr(c.row_id, c.row_ptr, c.type_end, c.nbr, c.prefix_w, c.type_prefix,
                             c.n_types, **kw)


# ---------------------------------------------------------------------------------- node tables
@pytest.fixture(scope="module")
def nodes(EA, O, torch_cuda):
    torch = torch_cuda
    lens = FC.ragged_lengths(N_NODES, 21)
    ids = FC.node_ids(N_NODES, 22)
    f = FR.ragged_table(FC.float_lists(lens), np.float32)
    u = FR.ragged_table(FC.u64_lists(lens), np.uint64)
    assert not f.is_uniform() and not u.is_uniform()
    G = chain_graph(EA, O, ids, features=f.as_tuple(), sparse_features=u.as_tuple())
    q = FC.node_queries(ids, 23)
    rows = FR.rows_of(ids, q)
    assert (rows >= 0).sum() > N_NODES and (rows < 0).sum() >= 8
    assert len(np.unique(q)) < len(q)                       # repeated ids
    case = dict(G=G, ids=ids, f=f, u=u, q=q, rows=rows, qt=torch.as_tensor(q).cuda(), lens=lens)
    yield case
    G.close()


def query_sets(case, torch):
    """(name, device queries, rows): the mix, one query, none"""
    q, rows = case["q"], case["rows"]
    known = int(np.where(rows >= 0)[0][0])
    return [("mix", case["qt"], rows),
            ("one", torch.as_tensor(q[known:known + 1]).cuda(), rows[known:known + 1]),
            ("none", torch.zeros(0, dtype=torch.int64, device="cuda"), rows[:0])]


def test_node_dense_ragged(nodes, torch_cuda):
    G, f = nodes["G"], nodes["f"]
    # every slot meets dims on both sides of its length
    longest = np.diff(np.concatenate([np.zeros((N_NODES, 1), np.int64),
                                      f.idx.reshape(N_NODES, -1)], 1), axis=1).max(0)
    assert (longest > min(DIMS)).all() and (longest < max(DIMS)).all()
    for name, qt, rows in query_sets(nodes, torch_cuda):
        for fid in FC.FIDS:
            got = G.get_dense_feature(qt, [fid] * len(DIMS), list(DIMS))
            for dim, g in zip(DIMS, got):
                want = FR.dense(f, rows, fid, dim)
                assert g.shape == want.shape
                assert np.array_equal(bits(t2n(g)), bits(want)), (name, fid, dim)


def test_node_dense_ragged_grid_stride(nodes, torch_cuda):
    """n * dim > 1 048 576 elements with dim = 5: the lane-per-element kernel strides."""
    G, f = nodes["G"], nodes["f"]
    q = FC.grow(nodes["q"], 1_048_576 // 5 + 1000, 31)
    assert len(q) * 5 > 1_048_576
    rows = FR.rows_of(nodes["ids"], q)
    got, = G.get_dense_feature(torch_cuda.as_tensor(q).cuda(), [1], [5])
    assert np.array_equal(bits(t2n(got)), bits(FR.dense(f, rows, 1, 5)))


# ---- uniform tables: the 16-byte (Vec4) kernel against the scalar one
def uniform_case(EA, O, widths, n, seed):
    ids = FC.node_ids(n, seed)
    arrays, at = [], 0
    for s, w in enumerate(widths):
        # value = 1 + row * stride + column (exact in float32, never 0: a zero fill is visible)
        arrays.append((1 + np.arange(n)[:, None] * sum(widths) + at + np.arange(w)[None, :])
                      .astype(np.float32))
        at += w
    t = FR.uniform_table(arrays, np.float32)
    assert t.is_uniform()
    return ids, t, chain_graph(EA, O, ids, features=t.as_tuple())


@pytest.fixture(scope="module")
def table_a(EA, O):
    """slots [4, 8, 12]: every slot begins on a multiple of 4 floats, the stride is one too -
    eligible for the 16-byte kernel when dim % 4 == 0 and the output is 16-byte aligned"""
    ids, t, G = uniform_case(EA, O, [4, 8, 12], 1000, 41)
    yield dict(ids=ids, t=t, G=G, q=FC.node_queries(ids, 42))
    G.close()


DIMS_A = (4, 8, 12, 16, 3, 5)


def dense_by_abi(G, torch, q, fid, dim, offset_floats):
    """euler_gpu_get_dense_feature into a buffer `offset_floats` past a 16-byte boundary; the
    floats around the output must stay untouched."""
    from euler_amd import _lib
    from euler_amd.graph import _stream
    n = len(q)
    qt = torch.as_tensor(q).cuda()
    guard = -12345.0
    buf = torch.full((n * dim + 8,), guard, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    with torch.cuda.device(G.device):
        _lib.check(_lib.lib().euler_gpu_get_dense_feature(
            G._h, _stream(), C.c_void_p(qt.data_ptr()), n, fid, dim,
            C.c_void_p(buf.data_ptr() + 4 * offset_floats)))
        torch.cuda.synchronize()
    out = t2n(buf)
    assert (out[:offset_floats] == guard).all() and (out[offset_floats + n * dim:] == guard).all()
    return out[offset_floats:offset_floats + n * dim].reshape(n, dim)


def check_table_a(case, torch, how):
    G, t, q = case["G"], case["t"], case["q"]
    rows = FR.rows_of(case["ids"], q)
    assert (rows < 0).any()
    qt = torch.as_tensor(q).cuda()
    for fid in FC.FIDS:
        for dim in DIMS_A:
            want = FR.dense(t, rows, fid, dim)
            if how == "api":
                got = t2n(G.get_dense_feature(qt, [fid], [dim])[0])
            else:
                got = dense_by_abi(G, torch, q, fid, dim, 1 if how == "unaligned" else 0)
            assert np.array_equal(bits(got), bits(want)), (how, fid, dim)


def test_node_dense_uniform_aligned(table_a, torch_cuda):
    """dims 4, 8, 12, 16: the 16-byte kernel, with dim > slot length zero-filled (slot 0 has 4
    values, slot 1 has 8, slot 2 has 12); dims 3 and 5: the scalar kernel."""
    check_table_a(table_a, torch_cuda, "api")
    check_table_a(table_a, torch_cuda, "aligned")


def test_node_dense_uniform_vec4_off(table_a, torch_cuda):
    """tuning key 8 = 0 (per thread): the scalar kernel answers every dim"""
    from euler_amd import _lib
    L = _lib.lib()
    assert L.euler_gpu_set_tuning(8, 0) == 0
    try:
        check_table_a(table_a, torch_cuda, "api")
    finally:
        assert L.euler_gpu_set_tuning(8, 1) == 0


def test_node_dense_uniform_unaligned_output(table_a, torch_cuda):
    """an output one float past a 16-byte boundary: the scalar kernel must take it"""
    check_table_a(table_a, torch_cuda, "unaligned")


def test_node_dense_uniform_grid_stride(table_a, torch_cuda):
    """n * dim / 4 > 1 048 576 16-byte lanes; dim 16 over the 12-value slot zero-fills"""
    G, t = table_a["G"], table_a["t"]
    q = FC.grow(table_a["q"], 270_000, 43)
    assert len(q) * 16 // 4 > 1_048_576
    rows = FR.rows_of(table_a["ids"], q)
    got, = G.get_dense_feature(torch_cuda.as_tensor(q).cuda(), [2], [16])
    assert np.array_equal(bits(t2n(got)), bits(FR.dense(t, rows, 2, 16)))


def test_node_dense_uniform_unaligned_slots(EA, O, torch_cuda):
    """slots [3, 5]: uniform, stride 8, but slot 1 begins at float 3 - not for the 16-byte kernel"""
    ids, t, G = uniform_case(EA, O, [3, 5], 500, 44)
    q = FC.node_queries(ids, 45)
    rows = FR.rows_of(ids, q)
    qt = torch_cuda.as_tensor(q).cuda()
    for fid in FC.FIDS:
        for dim in (4, 8):
            got, = G.get_dense_feature(qt, [fid], [dim])
            assert np.array_equal(bits(t2n(got)), bits(FR.dense(t, rows, fid, dim))), (fid, dim)
    G.close()


# ---- node sparse
def check_sparse(got, want, n, what):
    ind, val, shape = got
    w_ind, w_val, w_shape = want
    ind, val = t2n(ind), t2n(val)
    assert ind.shape == w_ind.shape and ind.dtype == np.int64 and val.dtype == np.int64, what
    assert np.array_equal(ind, w_ind), what
    assert np.array_equal(val, w_val), what
    assert list(shape) == list(w_shape), what
    assert np.array_equal(FR.row_offsets(ind, n), FR.row_offsets(w_ind, n)), what


def test_node_sparse(nodes, torch_cuda):
    G, u = nodes["G"], nodes["u"]
    assert G.num_u64_features() == FC.SLOTS
    for name, qt, rows in query_sets(nodes, torch_cuda):
        for dv in DEFAULTS:
            got = G.get_sparse_feature(qt, list(FC.FIDS), [dv] * len(FC.FIDS))
            for fid, g in zip(FC.FIDS, got):
                check_sparse(g, FR.sparse(u, rows, fid, dv), len(rows), (name, fid, dv))


def test_node_sparse_core(nodes, torch_cuda):
    G, u = nodes["G"], nodes["u"]
    for name, qt, rows in query_sets(nodes, torch_cuda):
        for fid in FC.FIDS:
            idx, val = G.get_sparse_feature_core(qt, fid)
            w_idx, w_val = FR.sparse_core(u, rows, fid)
            idx = t2n(idx)
            assert idx.dtype == np.int32 and idx.shape == (len(rows), 2)
            assert np.array_equal(idx, w_idx), (name, fid)
            assert np.array_equal(t2n(val), w_val), (name, fid)


def test_node_sparse_grid_stride(nodes, torch_cuda):
    """16 385+ queries: more waves than the fill launches"""
    G, u = nodes["G"], nodes["u"]
    q = FC.grow(nodes["q"], 16_384 + 613, 51)
    rows = FR.rows_of(nodes["ids"], q)
    qt = torch_cuda.as_tensor(q).cuda()
    g, = G.get_sparse_feature(qt, [2], [-1])
    check_sparse(g, FR.sparse(u, rows, 2, -1), len(q), "fid 2")
    idx, val = G.get_sparse_feature_core(qt, 0)
    w_idx, w_val = FR.sparse_core(u, rows, 0)
    assert np.array_equal(t2n(idx), w_idx) and np.array_equal(t2n(val), w_val)


def test_node_sparse_count_grid_stride(nodes, torch_cuda):
    """1 048 577+ queries through the count call of the C entry (indices_dev = NULL): nnz,
    max_len and the offsets"""
    from euler_amd import _lib
    from euler_amd.graph import _stream
    torch = torch_cuda
    G, u = nodes["G"], nodes["u"]
    q = FC.grow(nodes["q"], 1_048_576 + 4321, 52)
    rows = FR.rows_of(nodes["ids"], q)
    qt = torch.as_tensor(q).cuda()
    n = len(q)
    for fid in (1, 3):
        per_row = np.array([len(u.slot(r, fid)) for r in range(u.n)] + [0], np.int64)
        counts = np.maximum(per_row[rows], 1)               # (rows == -1 reads the appended 0)
        off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        nnz, max_len = C.c_int64(-1), C.c_int64(-1)
        _lib.check(_lib.lib().euler_gpu_get_sparse_feature(
            G._h, _stream(), C.c_void_p(qt.data_ptr()), n, fid, 0, C.c_void_p(off.data_ptr()),
            C.byref(nnz), C.byref(max_len), None, None))
        want = np.zeros(n + 1, np.int64)
        want[1:] = np.cumsum(counts)
        assert nnz.value == want[-1] and max_len.value == counts.max(), fid
        assert np.array_equal(t2n(off), want), fid


# ---- node binary: through a written directory
@pytest.fixture(scope="module")
def dat_nodes(EA, tmp_path_factory):
    d = tmp_path_factory.mktemp("feature_dat")
    lens = FC.ragged_lengths(N_NODES, 61)
    ids = FC.node_ids(N_NODES, 62)
    fl, ul, bl = FC.float_lists(lens), FC.u64_lists(lens), FC.byte_lists(lens)
    dat_write.write_feature_dat_dir(d, ids, fl, ul, bl, partitions=2)
    b = FR.ragged_table(bl, np.uint8)
    assert 0 in b.val and 255 in b.val and not b.is_uniform()
    return dict(path=str(d), ids=ids, b=b, u=FR.ragged_table(ul, np.uint64),
                f=FR.ragged_table(fl, np.float32), q=FC.node_queries(ids, 63))


def check_binary(got, want, what):
    off, data = got
    w_off, w_data = want
    assert np.array_equal(t2n(off), w_off), what
    assert np.array_equal(t2n(data), w_data), what


def test_node_binary(EA, dat_nodes, torch_cuda):
    torch = torch_cuda
    G = EA.Graph.load(dat_nodes["path"])
    b, ids, q = dat_nodes["b"], dat_nodes["ids"], dat_nodes["q"]
    rows = FR.rows_of(ids, q)
    qt = torch.as_tensor(q).cuda()
    # the table goes to the device with the first call that reads it, once
    bytes0 = G.device_bytes
    check_binary(G.get_binary_feature(qt[:1], [0])[0], FR.binary(b, rows[:1], 0), "first")
    bytes1 = G.device_bytes
    assert bytes1 > bytes0
    for fid, g in zip(FC.FIDS, G.get_binary_feature(qt, list(FC.FIDS))):
        check_binary(g, FR.binary(b, rows, fid), fid)
    assert G.device_bytes == bytes1
    check_binary(G.get_binary_feature(qt[:0], [1])[0], FR.binary(b, rows[:0], 1), "none")
    # 16 385+ queries: more waves than the fill launches
    big = FC.grow(q, 16_384 + 777, 64)
    check_binary(G.get_binary_feature(torch.as_tensor(big).cuda(), [2])[0],
                 FR.binary(b, FR.rows_of(ids, big), 2), "grid stride")
    # the float and uint64 slots of the same records came through the loader too
    got, = G.get_dense_feature(qt, [1], [301])
    assert np.array_equal(bits(t2n(got)), bits(FR.dense(dat_nodes["f"], rows, 1, 301)))
    g, = G.get_sparse_feature(qt, [2], [7])
    check_sparse(g, FR.sparse(dat_nodes["u"], rows, 2, 7), len(q), "dat sparse")
    G.close()


def test_node_binary_without_a_table(nodes, torch_cuda):
    """A graph with no binary table (n_slots 0): every row empty, nothing uploaded."""
    G = nodes["G"]
    bytes0 = G.device_bytes
    for fid, (off, data) in zip(FC.FIDS, G.get_binary_feature(nodes["qt"], list(FC.FIDS))):
        assert np.array_equal(t2n(off), np.zeros(len(nodes["q"]) + 1, np.int64)), fid
        assert data.numel() == 0, fid
    assert G.device_bytes == bytes0


def test_names_through_euler_ops(dat_nodes, torch_cuda):
    """feature names of the written directory's euler.meta; slots of 65+ values"""
    from euler_amd import euler_ops
    from euler_amd.euler_ops import feature_ops
    b, u, ids = dat_nodes["b"], dat_nodes["u"], dat_nodes["ids"]
    q = dat_nodes["q"]
    rows = FR.rows_of(ids, q)
    assert max(len(b.slot(r, 1)) for r in rows) >= 65 and max(len(u.slot(r, 2)) for r in rows) >= 65
    assert euler_ops.initialize_embedded_graph(dat_nodes["path"])
    try:
        G = euler_ops.get_default_graph()
        assert G.feature_info("binary_fb1") == (dat_write.BINARY, 1, 0)
        kind, slot, _ = G.feature_info("sparse_fs2")
        assert (kind, slot) == (dat_write.SPARSE, 2)
        fb1, fb0 = feature_ops.get_binary_feature(q, ["fb1", "fb0"])
        for name, fid, got in (("fb1", 1, fb1), ("fb0", 0, fb0)):
            assert got == [b.slot(r, fid).tobytes() for r in rows], name
        g, = feature_ops.get_sparse_feature(q, [str(slot)], [-3])
        check_sparse(g, FR.sparse(u, rows, slot, -3), len(q), "fs2")
        with pytest.raises(Exception):
            feature_ops.get_binary_feature(q, ["fs2"])           # a sparse feature's name
    finally:
        euler_ops.set_default_graph(None)


# ---------------------------------------------------------------------------------- edge store
def edge_triples(n, seed):
    """n distinct (src, dst, type): ids over the whole uint64 range (half at or above 2^63),
    types 0..2; records 0 / 1 are one (src, dst) under two types, record 2 has src 0."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    dst = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    ty = rng.integers(0, 3, n).astype(np.int32)
    src[1], dst[1], ty[0], ty[1] = src[0], dst[0], 0, 1
    src[2] = 0
    assert len({(int(a), int(b), int(c)) for a, b, c in zip(src, dst, ty)}) == n
    assert (src >= np.uint64(1 << 63)).any() and (dst >= np.uint64(1 << 63)).any()
    return src, dst, ty


def edge_queries(src, dst, ty, lens, seed):
    """[n, 3] int64: records of every slot length, random records, repeats and the misses."""
    rng = np.random.default_rng(seed)
    n = len(src)
    special = np.concatenate([
        np.where(lens.max(1) >= 15)[0], np.where(lens.sum(1) == 0)[0][:10],
        np.where((lens[:, 0] > 0) & (lens[:, 1] == 0) & (lens[:, 2] > 0))[0][:10]])
    pick = np.concatenate([[0, 1, 2], special, rng.integers(0, n, 400), [5, 5, 5]])
    s, d, t = (src[pick].astype(np.int64), dst[pick].astype(np.int64), ty[pick].astype(np.int64))
    known = np.stack([s, d, t], 1)
    k = known[:40]
    miss = [np.stack([k[:, 1], k[:, 0], k[:, 2]], 1),                  # (dst, src) swapped
            np.stack([k[:, 0], k[:, 1], np.full(40, -1)], 1),          # type -1
            np.stack([k[:, 0], k[:, 1], np.full(40, 1000)], 1),        # type 1000
            np.stack([k[:, 0] + 1, k[:, 1], k[:, 2]], 1),              # ids one off
            np.stack([k[:, 0], k[:, 1] - 1, k[:, 2]], 1),
            np.stack([np.zeros(40, np.int64), k[:, 1], k[:, 2]], 1),   # src 0 with another dst
            np.array([[s[0], d[0], 2], [0, 0, 0], [-1, -1, 0], [-2 ** 63, 2 ** 63 - 1, 1]])]
    q = np.concatenate([known[:300]] + miss + [known[300:]]).astype(np.int64)
    return q


@pytest.fixture(scope="module")
def edges(EA, O, torch_cuda):
    torch = torch_cuda
    lens = FC.ragged_lengths(N_EDGES, 71)
    src, dst, ty = edge_triples(N_EDGES, 72)
    w = np.ones(N_EDGES, np.float32)
    fl, ul, bl = FC.float_lists(lens), FC.u64_lists(lens), FC.byte_lists(lens)
    f, u, b = (FR.ragged_table(fl, np.float32), FR.ragged_table(ul, np.uint64),
               FR.ragged_table(bl, np.uint8))
    assert not f.is_uniform() and not u.is_uniform() and not b.is_uniform()
    G = chain_graph(EA, O, FC.node_ids(64, 73))
    G.set_edges(src, dst, ty, w,
                dense=[[rec[s] for rec in fl] for s in range(FC.SLOTS)],
                sparse=[[rec[s] for rec in ul] for s in range(FC.SLOTS)],
                binary=[[rec[s] for rec in bl] for s in range(FC.SLOTS)])
    assert G.num_edge_records == N_EDGES
    q = edge_queries(src, dst, ty, lens, 74)
    ords = FR.ordinals(src, dst, ty, q)
    assert (ords >= 0).sum() >= 400 and (ords < 0).sum() >= 240
    assert ords[0] == 0 and ords[1] == 1 and ords[2] == 2
    asked = lens[ords[ords >= 0]]
    for s in range(FC.SLOTS):
        assert set(FC.LENGTHS) <= set(asked[:, s].tolist())
    big = FC.grow(q, 131_072 + 999, 75)
    case = dict(G=G, src=src, dst=dst, ty=ty, f=f, u=u, b=b, q=q, ords=ords,
                qt=torch.as_tensor(q).cuda(), big=big, big_ords=FR.ordinals(src, dst, ty, big),
                big_t=torch.as_tensor(big).cuda())
    yield case
    G.close()


def edge_query_sets(case, torch):
    return [("mix", case["qt"], case["ords"]),
            ("one", case["qt"][3:4], case["ords"][3:4]),
            ("none", torch.zeros((0, 3), dtype=torch.int64, device="cuda"), case["ords"][:0])]


def test_edge_ordinals(edges, torch_cuda):
    G = edges["G"]
    for name, qt, ords in edge_query_sets(edges, torch_cuda):
        assert np.array_equal(t2n(G.edge_ordinals(qt)), ords), name
    assert np.array_equal(t2n(G.edge_ordinals(edges["big_t"])), edges["big_ords"])


def test_edge_table_full_lines(edges):
    """20 000 records in 10 000 lines of 4 slots: some lines are the home of more than 4
    records, whose overflow lives in the following lines.  Every record must be found."""
    G = edges["G"]
    src, dst, ty = edges["src"], edges["dst"], edges["ty"]
    n_lines = (N_EDGES + 1) // 2
    home = np.array([edge_line(n_lines, int(s), int(d), int(t)) for s, d, t in zip(src, dst, ty)])
    assert (np.bincount(home, minlength=n_lines) > 4).sum() >= 50     # (about 5% of the lines)
    e_src, e_dst, e_ty, _ = G.export_edges()
    assert np.array_equal(e_src, src) and np.array_equal(e_dst, dst) and np.array_equal(e_ty, ty)
    triples = np.stack([e_src.astype(np.int64), e_dst.astype(np.int64), e_ty.astype(np.int64)], 1)
    assert np.array_equal(t2n(G.edge_ordinals(triples)), np.arange(N_EDGES))


def test_edge_dense(edges, torch_cuda):
    G, f = edges["G"], edges["f"]
    dims = (1, 3, 8, 9, 17, 65, 301)
    for name, qt, ords in edge_query_sets(edges, torch_cuda):
        for fid in FC.FIDS:
            got = G.get_edge_dense_feature(qt, [fid] * len(dims), list(dims))
            for dim, g in zip(dims, got):
                assert np.array_equal(bits(t2n(g)), bits(FR.dense(f, ords, fid, dim))), (name, fid, dim)
    got, = G.get_edge_dense_feature(edges["big_t"], [1], [9])
    assert np.array_equal(bits(t2n(got)), bits(FR.dense(f, edges["big_ords"], 1, 9)))


def test_edge_sparse(edges, torch_cuda):
    G, u = edges["G"], edges["u"]
    for name, qt, ords in edge_query_sets(edges, torch_cuda):
        for dv in DEFAULTS:
            got = G.get_edge_sparse_feature(qt, list(FC.FIDS), [dv] * len(FC.FIDS))
            for fid, g in zip(FC.FIDS, got):
                check_sparse(g, FR.sparse(u, ords, fid, dv), len(ords), (name, fid, dv))
    g, = G.get_edge_sparse_feature(edges["big_t"], [0], [-1])
    check_sparse(g, FR.sparse(u, edges["big_ords"], 0, -1), len(edges["big"]), "grid stride")


def test_edge_binary(edges, torch_cuda):
    G, b = edges["G"], edges["b"]
    for name, qt, ords in edge_query_sets(edges, torch_cuda):
        for fid, g in zip(FC.FIDS, G.get_edge_binary_feature(qt, list(FC.FIDS))):
            check_binary(g, FR.binary(b, ords, fid), (name, fid))
    check_binary(G.get_edge_binary_feature(edges["big_t"], [2])[0],
                 FR.binary(b, edges["big_ords"], 2), "grid stride")


def test_edge_uniform_arrays_and_lists_agree(EA, O, edges, torch_cuda):
    """Slots of one length everywhere, passed as [n, d] arrays and as lists of equal-length
    sequences: both are stored as uniform tables and answer identically."""
    n = 5000
    src, dst, ty = edges["src"][:n], edges["dst"][:n], edges["ty"][:n]
    rng = np.random.default_rng(81)
    d0, d1 = (rng.standard_normal((n, 5)).astype(np.float32),
              rng.standard_normal((n, 9)).astype(np.float32))
    s0 = rng.integers(0, 2 ** 64, (n, 10), dtype=np.uint64)
    b0 = rng.integers(0, 256, (n, 11)).astype(np.uint8)
    tf, tu, tb = (FR.uniform_table([d0, d1], np.float32), FR.uniform_table([s0], np.uint64),
                  FR.uniform_table([b0], np.uint8))
    as_lists = FR.ragged_table([[list(a), list(b)] for a, b in zip(d0, d1)], np.float32)
    assert tf.is_uniform() and as_lists.is_uniform() and np.array_equal(as_lists.val, tf.val)
    w = np.ones(n, np.float32)
    ids = FC.node_ids(64, 82)
    Ga, Gb = chain_graph(EA, O, ids), chain_graph(EA, O, ids)
    Ga.set_edges(src, dst, ty, w, dense=[d0, d1], sparse=[s0], binary=[b0])
    Gb.set_edges(src, dst, ty, w, dense=[[list(r) for r in d0], [list(r) for r in d1]],
                 sparse=[[list(r) for r in s0]], binary=[[r.tobytes() for r in b0]])
    q = edges["q"]
    ords = FR.ordinals(src, dst, ty, q)
    assert (ords >= 0).any() and (ords < 0).any()
    qt = edges["qt"]
    for G in (Ga, Gb):
        assert np.array_equal(t2n(G.edge_ordinals(qt)), ords)
        for fid in FC.FIDS:
            for dim, g in zip((4, 9, 12), G.get_edge_dense_feature(qt, [fid] * 3, [4, 9, 12])):
                assert np.array_equal(bits(t2n(g)), bits(FR.dense(tf, ords, fid, dim))), (fid, dim)
            g, = G.get_edge_sparse_feature(qt, [fid], [-1])
            check_sparse(g, FR.sparse(tu, ords, fid, -1), len(q), fid)
            check_binary(G.get_edge_binary_feature(qt, [fid])[0], FR.binary(tb, ords, fid), fid)
    Ga.close()
    Gb.close()


# ---- probing: the wrap from the last line to line 0
_M64 = (1 << 64) - 1


def mix64(z):
    """Mix64 of euler_amd/csrc/common.h"""
    z ^= z >> 30
    z = z * 0xbf58476d1ce4e5b9 & _M64
    z ^= z >> 27
    z = z * 0x94d049bb133111eb & _M64
    return z ^ (z >> 31)


def edge_line(n_lines, src, dst, type):
    """EdgeLine of euler_amd/csrc/edge_kernels.hip (the home line of a triple), restated to
    CHOOSE inputs only - expected values come from the dict reference.  It must follow the
    library's hash if that ever changes: the preconditions asserted with it fail otherwise."""
    h = mix64(src ^ mix64(dst ^ ((type & 0xffffffff) << 40)))
    return (h * n_lines) >> 64                              # __umul64hi


def test_edge_table_probe_wraps(EA, O, torch_cuda):
    """10 records in 5 lines, 6 of them with the LAST line as their home: two of those live in
    line 0 (or later), reached only by wrapping; the records at home in line 0 move on in turn."""
    n, n_lines = 10, 5
    rng = np.random.default_rng(91)
    last, rest = [], []
    while len(last) < 6 or len(rest) < 4:
        s, d, t = int(rng.integers(1, 2 ** 63)), int(rng.integers(1, 2 ** 63)), int(rng.integers(0, 3))
        home = edge_line(n_lines, s, d, t)
        if home == n_lines - 1 and len(last) < 6:
            last.append((s, d, t))
        elif home != n_lines - 1 and len(rest) < 4:
            rest.append((s, d, t))
    # near misses whose probe starts in the full last line too
    near = []
    while len(near) < 6:
        s, d, t = last[len(near)]
        s += int(rng.integers(1, 1000))
        if edge_line(n_lines, s, d, t) == n_lines - 1 and (s, d, t) not in last:
            near.append((s, d, t))
    recs = np.array(rest[:2] + last + rest[2:], np.int64)
    homes = [edge_line(n_lines, *map(int, r)) for r in recs]
    assert sum(h == n_lines - 1 for h in homes) >= 5        # more than the line's 4 slots
    src, dst, ty = recs[:, 0].astype(np.uint64), recs[:, 1].astype(np.uint64), recs[:, 2].astype(np.int32)
    G = chain_graph(EA, O, FC.node_ids(64, 92))
    G.set_edges(src, dst, ty, np.ones(n, np.float32), sparse=[np.arange(n, dtype=np.uint64)[:, None] + 100])
    q = np.concatenate([recs, np.array(near, np.int64), recs[:, [1, 0, 2]]])
    want = FR.ordinals(src, dst, ty, q)
    assert want[:n].tolist() == list(range(n)) and (want[n:] == -1).all()
    assert np.array_equal(t2n(G.edge_ordinals(q)), want)
    (ind, val, shape), = G.get_edge_sparse_feature(q, [0], [-1])
    assert np.array_equal(t2n(val), np.where(want >= 0, want + 100, -1))
    G.close()
