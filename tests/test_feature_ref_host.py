"""The plain feature reference (tests/feature_ref.py) and the feature-writing .dat helper
(tests/dat_write.py) checked without a GPU: the reference against the reference project's own
recorded outputs and against the oracle on the ragged tables the GPU tests use; the helper's files
read back through the project's reader (and the reference's loader where it is built)."""
import ctypes as C
import os

import numpy as np
import pytest

import dat_write
import feature_cases as FC
import feature_ref as FR
from test_host import read_dat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

N = 400


@pytest.fixture(scope="module")
def ragged():
    """ids, float table, uint64 table, byte table, and the per-record lists they came from."""
    lens = FC.ragged_lengths(N, 11)
    ids = FC.node_ids(N, 12)
    fl, ul, bl = FC.float_lists(lens), FC.u64_lists(lens), FC.byte_lists(lens)
    return dict(ids=ids, lens=lens, fl=fl, ul=ul, bl=bl,
                f=FR.ragged_table(fl, np.float32), u=FR.ragged_table(ul, np.uint64),
                b=FR.ragged_table(bl, np.uint8))


def test_tables_and_builders(ragged):
    lens = ragged["lens"]
    for t, dt in ((ragged["f"], np.float32), (ragged["u"], np.uint64), (ragged["b"], np.uint8)):
        assert t.slots == FC.SLOTS and t.n == N and t.val.dtype == dt
        assert not t.is_uniform()
        assert np.array_equal(t.idx.reshape(N, -1), np.cumsum(lens, 1))
        assert np.array_equal(np.diff(t.ptr), lens.sum(1))
    assert (ragged["u"].val >= np.uint64(1 << 63)).any() and (ragged["u"].val < np.uint64(1 << 63)).any()
    assert 0 in ragged["b"].val and 255 in ragged["b"].val
    for vals in (ragged["f"].val.view(np.uint32), ragged["u"].val):
        assert len(np.unique(vals)) == len(vals)                 # a misplaced value is visible
    assert np.isfinite(ragged["f"].val).all()
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    b = np.arange(8, dtype=np.float32).reshape(4, 2) + 100
    t = FR.uniform_table([a, b], np.float32)
    assert t.is_uniform() and t.idx.tolist() == [3, 5] * 4 and t.ptr.tolist() == [0, 5, 10, 15, 20]
    assert t.slot(2, 1).tolist() == [104, 105] and t.slot(3, 0).tolist() == [9, 10, 11]
    same = FR.ragged_table([[list(x), list(y)] for x, y in zip(a, b)], np.float32)
    assert same.is_uniform() and np.array_equal(same.val, t.val) and np.array_equal(same.idx, t.idx)
    for row, fid in ((-1, 0), (0, -1), (0, 2), (0, 7)):
        assert len(t.slot(row, fid)) == 0


def test_lookups():
    ids = np.array([5, 9, 2 ** 63 + 1, 7], np.uint64)
    q = np.array([9, 0, -2 ** 63 + 1, 6, 7, 7, -1], np.int64)
    assert FR.rows_of(ids, q).tolist() == [1, -1, 2, -1, 3, 3, -1]
    assert FR.rows_of(ids, np.zeros(0, np.int64)).shape == (0,)
    src = np.array([1, 1, 2, 2 ** 63], np.uint64)
    dst = np.array([2, 2, 1, 4], np.uint64)
    ty = np.array([0, 1, 0, 3], np.int32)
    q = [[1, 2, 0], [1, 2, 1], [2, 1, 0], [2, 1, 1], [1, 2, -1], [1, 2, 1000], [-2 ** 63, 4, 3],
         [0, 2, 0]]
    assert FR.ordinals(src, dst, ty, q).tolist() == [0, 1, 2, -1, -1, -1, 3, -1]
    assert FR.ordinals(src, dst, ty, np.zeros((0, 3), np.int64)).shape == (0,)


def test_ops_by_hand():
    """One small table, every answer written out."""
    t = FR.ragged_table([[[1, 2, 3], [], [4]], [[], [], []], [[5], [6, 7], []]], np.uint64)
    rows = [0, -1, 2, 1]
    ind, val, shape = FR.sparse(t, rows, 0, -9)
    assert ind.tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [2, 0], [3, 0]]
    assert val.tolist() == [1, 2, 3, -9, 5, -9] and shape == [4, 3]
    assert FR.row_offsets(ind, 4).tolist() == [0, 3, 4, 5, 6]
    ind, val, shape = FR.sparse(t, rows, 1, 2 ** 62)              # empty middle slot of record 0
    assert val.tolist() == [2 ** 62, 2 ** 62, 6, 7, 2 ** 62] and shape == [4, 2]
    ind, val, shape = FR.sparse(t, rows, 2, 0)
    assert val.tolist() == [4, 0, 0, 0] and shape == [4, 1]
    assert FR.sparse(t, rows, 3, 7)[1].tolist() == [7] * 4
    assert FR.sparse(t, [], 0, 7)[2] == [0, 0] and FR.sparse(t, [], 0, 7)[0].shape == (0, 2)
    idx, val = FR.sparse_core(t, rows, 0)
    assert idx.dtype == np.int32 and idx.tolist() == [[0, 3], [3, 3], [3, 4], [4, 4]]
    assert val.tolist() == [1, 2, 3, 5]
    idx, val = FR.sparse_core(t, rows, -1)
    assert idx.tolist() == [[0, 0]] * 4 and len(val) == 0
    f = FR.ragged_table([[[1, 2, 3], [], [4]], [[], [], []], [[5], [6, 7], []]], np.float32)
    assert FR.dense(f, rows, 0, 2).tolist() == [[1, 2], [0, 0], [5, 0], [0, 0]]
    assert FR.dense(f, rows, 1, 3).tolist() == [[0, 0, 0], [0, 0, 0], [6, 7, 0], [0, 0, 0]]
    assert FR.dense(f, rows, 3, 2).tolist() == [[0, 0]] * 4 and FR.dense(f, [], 0, 2).shape == (0, 2)
    b = FR.ragged_table([[b"ab", b""], [b"", b"\x00\xff!"]], np.uint8)
    off, data = FR.binary(b, [1, 0, -1, 1], 1)
    assert off.tolist() == [0, 3, 3, 3, 6] and data.tobytes() == b"\x00\xff!\x00\xff!"
    off, data = FR.binary(b, [1, 0], 0)
    assert off.tolist() == [0, 0, 2] and data.tobytes() == b"ab"
    assert FR.binary(b, [], 0)[0].tolist() == [0]


@pytest.mark.parametrize("pre", ["fx", "rg"])
def test_dense_against_recorded_reference_outputs(pre, random_csr):
    """tests/golden/features.npz: the reference's GetDenseFeature on the fixture and the random
    graph."""
    g = np.load(os.path.join(GOLDEN, "features.npz"))
    ids = g["fx_ids"] if pre == "fx" else random_csr.row_id
    t = FR.Table(int(g[pre + "_n_float"]), g[pre + "_feat_ptr"], g[pre + "_feat_idx"],
                 g[pre + "_feat_val"])
    rows = FR.rows_of(ids, g[pre + "_query"])
    assert (rows < 0).any() and (rows >= 0).any()
    for k, (fid, dim) in enumerate(zip(g[pre + "_fids"].tolist(), g[pre + "_dims"].tolist())):
        assert np.array_equal(FR.dense(t, rows, fid, dim), g["%s_dense_%d" % (pre, k)]), (fid, dim)


@pytest.mark.parametrize("pre", ["fx", "rg"])
def test_sparse_against_recorded_reference_outputs(pre, random_csr):
    """tests/golden/sparse_features.npz: the reference's GetSparseFeature."""
    g = np.load(os.path.join(GOLDEN, "sparse_features.npz"))
    ids = g["fx_ids"] if pre == "fx" else random_csr.row_id
    t = FR.Table(int(g[pre + "_n_u64"]), g[pre + "_feat_ptr"], g[pre + "_feat_idx"],
                 g[pre + "_feat_val"])
    rows = FR.rows_of(ids, g[pre + "_query"])
    for k, (fid, dv) in enumerate(zip(g[pre + "_fids"].tolist(), g[pre + "_defaults"].tolist())):
        ind, val, shape = FR.sparse(t, rows, fid, dv)
        assert np.array_equal(ind, g["%s_sp_%d_ind" % (pre, k)]), fid
        assert np.array_equal(val, g["%s_sp_%d_val" % (pre, k)]), fid
        assert shape == g["%s_sp_%d_shape" % (pre, k)].tolist(), fid


def _chain_csr(O, ids):
    n = len(ids)
    return O.csr_from_raw(ids, np.arange(n + 1, dtype=np.int64), np.roll(ids, -1),
                          np.ones(n, np.float32), 1)


def test_against_oracle_on_the_ragged_tables(O, ragged):
    ids = ragged["ids"]
    OG = O.OracleGraph(_chain_csr(O, ids))
    q = FC.node_queries(ids, 3)
    rows = FR.rows_of(ids, q)
    assert (rows < 0).sum() >= 8
    f, u = ragged["f"], ragged["u"]
    DF = O.DenseFeatures(*f.as_tuple())
    SF = O.SparseFeatures(*u.as_tuple())
    for fid in FC.FIDS:
        # (the oracle refuses a slot longer than dim: the dims at or above the longest slot)
        for dim in (300, 301, 512):
            want, = OG.get_dense_feature(DF, q, [fid], [dim])
            assert np.array_equal(FR.dense(f, rows, fid, dim), want), (fid, dim)
        # truncation = the leading columns of the wide answer
        wide, = OG.get_dense_feature(DF, q, [fid], [301])
        for dim in (1, 5, 64, 65):
            assert np.array_equal(FR.dense(f, rows, fid, dim), wide[:, :dim]), (fid, dim)
        for dv in (0, -1, 2 ** 62):
            (ind, val, shape), = OG.get_sparse_feature(SF, q.astype(np.uint64), [fid], [dv])
            r_ind, r_val, r_shape = FR.sparse(u, rows, fid, dv)
            assert np.array_equal(r_ind, ind) and np.array_equal(r_val, val), (fid, dv)
            assert r_shape == shape.tolist(), (fid, dv)
        # the core form = the sparse form without its default entries
        idx, val = FR.sparse_core(u, rows, fid)
        lens = np.array([len(u.slot(r, fid)) for r in rows])
        assert np.array_equal(np.diff(idx, axis=1)[:, 0], lens)
        assert np.array_equal(idx[1:, 0], idx[:-1, 1]) and idx[0, 0] == 0
        r_ind, r_val, _ = FR.sparse(u, rows, fid, 0)
        keep = np.repeat(lens > 0, np.maximum(lens, 1))
        assert np.array_equal(val, r_val[keep])


def _dat_node_binary(path):
    from euler_amd import _lib
    L = _lib.lib()
    csr, parts, owner = _lib.HostCSR(), C.c_int32(0), C.c_void_p()
    assert L.euler_gpu_dat_open(str(path).encode(), 0, 1, C.byref(csr), C.byref(parts),
                                C.byref(owner)) == 0
    try:
        n = csr.n_rows
        cnt = C.c_int32(0)
        ptr, idx, val = _lib.i64p(), _lib.i32p(), _lib.u8p()
        assert L.euler_gpu_dat_node_binary(owner, C.byref(cnt), C.byref(ptr), C.byref(idx),
                                           C.byref(val)) == 0
        if cnt.value == 0:
            return None
        p = np.ctypeslib.as_array(ptr, (n + 1,)).copy()
        return FR.Table(cnt.value, p, np.ctypeslib.as_array(idx, (n * cnt.value,)).copy(),
                        np.ctypeslib.as_array(val, (max(int(p[-1]), 1),))[:int(p[-1])].copy())
    finally:
        L.euler_gpu_dat_close(owner)


def test_feature_dat_helper_reads_back(O, ragged, tmp_path):
    from euler_amd.graph import dat_feature_info
    ids = ragged["ids"]
    names = dat_write.write_feature_dat_dir(tmp_path, ids, ragged["fl"], ragged["ul"], ragged["bl"],
                                            partitions=3)
    d = read_dat(tmp_path)
    assert d["partitions"] == 3 and d["n_types"] == 1
    assert sorted(d["row_id"].tolist()) == ids.tolist()
    assert d["n_float"] == FC.SLOTS and d["n_u64"] == FC.SLOTS
    got_f = FR.Table(d["n_float"], d["feat_ptr"], d["feat_idx"], d["feat_val"])
    got_u = FR.Table(d["n_u64"], d["ufeat_ptr"], d["ufeat_idx"], d["ufeat_val"])
    got_b = _dat_node_binary(tmp_path)
    assert got_b is not None and got_b.slots == FC.SLOTS
    back = FR.rows_of(ids, d["row_id"])                # the written record of each row read
    for row, r in enumerate(back.tolist()):
        assert d["nbr"][d["row_ptr"][row]:d["row_ptr"][row + 1]].tolist() == [ids[(r + 1) % N]]
        for s in range(FC.SLOTS):
            assert np.array_equal(got_f.slot(row, s).view(np.uint32),
                                  ragged["f"].slot(r, s).view(np.uint32))
            assert np.array_equal(got_u.slot(row, s), ragged["u"].slot(r, s))
            assert np.array_equal(got_b.slot(row, s), ragged["b"].slot(r, s))
    # euler.meta's name tables
    assert [x[0] for x in names] == ["sparse_fs0", "sparse_fs1", "sparse_fs2", "dense_fd0",
                                     "dense_fd1", "dense_fd2", "binary_fb0", "binary_fb1",
                                     "binary_fb2"]
    assert dat_feature_info(tmp_path, "dense_fd1") == (dat_write.DENSE, 1, 300)
    assert dat_feature_info(tmp_path, "sparse_fs2") == (dat_write.SPARSE, 2, 300)
    assert dat_feature_info(tmp_path, "binary_fb0") == (dat_write.BINARY, 0, 0)
    if O.have_ref():
        R = O.RefGraph.load(str(tmp_path), 1)
        rf = R.export_float_features(ids)
        ru = R.export_u64_features(ids)
        for got, want in ((FR.Table(rf.n_float, rf.feat_ptr, rf.feat_idx, rf.feat_val), ragged["f"]),
                          (FR.Table(ru.n_u64, ru.feat_ptr, ru.feat_idx, ru.feat_val), ragged["u"])):
            assert got.slots == want.slots
            assert np.array_equal(got.ptr, want.ptr) and np.array_equal(got.idx, want.idx)
            assert got.val.tobytes() == want.val.tobytes()


def test_feature_dat_helper_without_a_kind(tmp_path):
    """A directory written without binary features has no binary table."""
    ids = FC.node_ids(8, 1)
    dat_write.write_feature_dat_dir(tmp_path, ids, floats=[[[1.0, 2.0]]] * 8, partitions=1)
    d = read_dat(tmp_path)
    assert d["n_float"] == 1 and d["n_u64"] == 0
    assert d["feat_val"].tolist() == [1.0, 2.0] * 8
    assert _dat_node_binary(tmp_path) is None
