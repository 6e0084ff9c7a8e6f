"""CPU checks of the graph-label path: the .dat reader's binary_graph_label values on the fixture,
the numpy restatement (tests/graph_label_ref.py) against hand-written expectations, its Philox
against the oracle's, and the library's new entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import graph_label_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")


@pytest.fixture(scope="module")
def L():
    from euler_amd import _lib
    return _lib.lib()


def fixture_labels(L):
    from euler_amd import _lib
    from euler_amd.graph import dat_feature_info
    ftype, slot, _ = dat_feature_info(FIXTURE, "binary_graph_label")
    assert ftype == 2
    csr = _lib.HostCSR()
    parts, owner = C.c_int32(0), C.c_void_p()
    assert L.euler_gpu_dat_open(FIXTURE.encode(), 0, 1, C.byref(csr), C.byref(parts),
                                C.byref(owner)) == 0
    try:
        n = csr.n_rows
        rid = np.ctypeslib.as_array(csr.row_id, (n,)).tolist()
        cnt = C.c_int32(0)
        ptr, idx, val = _lib.i64p(), _lib.i32p(), _lib.u8p()
        assert L.euler_gpu_dat_node_binary(owner, C.byref(cnt), C.byref(ptr), C.byref(idx),
                                           C.byref(val)) == 0
        p = np.ctypeslib.as_array(ptr, (n + 1,)).copy()
        ix = np.ctypeslib.as_array(idx, (n * cnt.value,)).reshape(n, cnt.value).copy()
        v = np.ctypeslib.as_array(val, (max(int(p[-1]), 1),)).tobytes()
        out = {}
        for r in range(n):
            pre = 0 if slot == 0 else ix[r, slot - 1]
            out[rid[r]] = v[p[r] + pre:p[r] + ix[r, slot]].decode()
        return out
    finally:
        L.euler_gpu_dat_close(owner)


def test_fixture_graph_labels_from_dat(L):
    labels = fixture_labels(L)
    assert {i: labels[i] for i in range(1, 7)} == {i: str(i) for i in range(1, 7)}


def test_restatement_on_fixture(L):
    labels = fixture_labels(L)
    ids = sorted(labels)
    table, nodes = R.label_table(ids, [labels[i] for i in ids])
    assert table == ["1", "2", "3", "4", "5", "6"]
    assert nodes == [[1], [2], [3], [4], [5], [6]]
    ind, val, shape = R.graph_by_label(table, nodes, ["1", "2", "3", "nope", "2"])
    assert ind.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [4, 0]]
    assert val.tolist() == [1, 2, 3, 0, 2]
    assert shape == [5, 1]
    ind, val, shape = R.graph_by_label(table, nodes, [])
    assert ind.shape == (0, 2) and shape == [0, 0]


def test_restatement_orders():
    # table by smallest id, nodes ascending, "" no label
    table, nodes = R.label_table([9, 3, 7, 5, 4, 8], ["b", "a", "b", "", "c", "a"])
    assert table == ["a", "c", "b"]
    assert nodes == [[3, 8], [4], [7, 9]]
    ind, val, shape = R.graph_by_label(table, nodes, ["b", "x", "a"])
    assert ind.tolist() == [[0, 0], [0, 1], [1, 0], [2, 0], [2, 1]]
    assert val.tolist() == [7, 9, 0, 3, 8]
    assert shape == [3, 2]


def test_restated_philox_matches_oracle():
    from oracle import oracle as O
    for seed, call_id, dom, stream in ((0, 0, 1, 0), (12345678901, 7, 6, 99), (2**40 + 3, 3, 5, 2**33)):
        u = R.rng_draws(seed, call_id, dom, stream, 6)
        for j in range(6):
            w = O.philox([call_id, stream & 0xFFFFFFFF, stream >> 32, j >> 1],
                         [seed & 0xFFFFFFFF, ((seed >> 32) ^ R.SALT[dom]) & 0xFFFFFFFF])
            a, b = w[2 * (j & 1)], w[2 * (j & 1) + 1]
            assert u[j] == ((a >> 5) * 67108864.0 + (b >> 6)) * (1.0 / 9007199254740992.0)
    s = R.sample_graph_label(5, 1, 1000, 7)
    assert s.min() >= 0 and s.max() <= 6


def test_block_restatement():
    n_id = [5, 1, 5, 2]
    adj = {5: {1, 2}, 1: {5}, 2: {9}}
    e = R.block_ref(n_id, adj)
    assert e.tolist() == [[0, 0, 1, 1, 2, 2, 0, 1, 2, 3], [1, 3, 0, 2, 1, 3, 0, 1, 2, 3]]


def test_library_exports_label_entry_points(L):
    for name in ("euler_gpu_graph_set_graph_labels", "euler_gpu_graph_num_graph_labels",
                 "euler_gpu_graph_export_graph_labels", "euler_gpu_graph_label_ids",
                 "euler_gpu_sample_graph_label", "euler_gpu_get_graph_by_label",
                 "euler_gpu_whole_graph_block"):
        assert hasattr(L, name)
    from euler_amd import dataflow
    with pytest.raises(ValueError):
        dataflow.WholeGraphDataFlow(None, [[0], [1]])
