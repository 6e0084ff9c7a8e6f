"""CPU checks of the Edge reader (euler_gpu_dat_open_edges), the binary node features of the
.dat reader and the euler.meta feature-name lookup, on tests/golden/fixture_dat."""
import ctypes as C
import os
import shutil
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")


@pytest.fixture(scope="module")
def L():
    from euler_amd import _lib
    return _lib.lib()


def parse_edge_files(path):
    """Independent parse of Edge/*.dat (Edge::DeSerialize field order), sorted file order."""
    recs = []
    edir = os.path.join(path, "Edge")
    for fn in sorted(os.listdir(edir)):
        b = open(os.path.join(edir, fn), "rb").read()
        i = 0
        while i < len(b):
            n, = struct.unpack_from("<I", b, i)
            r = b[i + 4:i + 4 + n]
            i += 4 + n
            src, dst, t, w = struct.unpack_from("<QQif", r, 0)
            j = 24

            def vec(fmt, j):
                k, = struct.unpack_from("<I", r, j)
                return list(struct.unpack_from("<%d%s" % (k, fmt), r, j + 4)), j + 4 + k * struct.calcsize(fmt)

            ui, j = vec("i", j)
            uv, j = vec("Q", j)
            fi, j = vec("i", j)
            fv, j = vec("f", j)
            bi, j = vec("i", j)
            k, = struct.unpack_from("<I", r, j)
            bv = r[j + 4:j + 4 + k]
            recs.append(dict(src=src, dst=dst, type=t, weight=w, ui=ui, uv=uv, fi=fi, fv=fv,
                             bi=bi, bv=bv))
    return recs


def open_edges(path):
    from euler_amd import _lib
    L = _lib.lib()
    e = _lib.HostEdges()
    owner = C.c_void_p()
    rc = L.euler_gpu_dat_open_edges(str(path).encode(), 0, 1, C.byref(e), C.byref(owner))
    if rc != 0:
        return rc, None
    n = e.n
    out = dict(src=np.ctypeslib.as_array(e.src, (n,)).copy(),
               dst=np.ctypeslib.as_array(e.dst, (n,)).copy(),
               type=np.ctypeslib.as_array(e.type, (n,)).copy(),
               weight=np.ctypeslib.as_array(e.weight, (n,)).copy(), n_types=e.n_edge_types)
    for key, cnt, ptr, idx, val in (("f", e.n_float_features, e.feat_ptr, e.feat_idx, e.feat_val),
                                    ("u", e.n_u64_features, e.ufeat_ptr, e.ufeat_idx, e.ufeat_val),
                                    ("b", e.n_binary_features, e.bfeat_ptr, e.bfeat_idx, e.bfeat_val)):
        p = np.ctypeslib.as_array(ptr, (n + 1,)).copy()
        out[key] = (cnt, p, np.ctypeslib.as_array(idx, (max(n * cnt, 1),))[:n * cnt].copy(),
                    np.ctypeslib.as_array(val, (max(int(p[-1]), 1),))[:int(p[-1])].copy())
    L.euler_gpu_dat_close(owner)
    return 0, out


def slot(table, r, f):
    cnt, ptr, idx, val = table
    if f >= cnt:
        return val[:0]
    ends = idx[r * cnt:(r + 1) * cnt]
    pre = 0 if f == 0 else ends[f - 1]
    return val[ptr[r] + pre:ptr[r] + ends[f]]


def test_edges_match_an_independent_parse(L):
    rc, got = open_edges(FIXTURE)
    assert rc == 0, L.euler_gpu_last_error()
    want = parse_edge_files(FIXTURE)
    assert len(want) == 12 and len(got["src"]) == 12
    assert got["n_types"] == 2
    for r, w in enumerate(want):
        assert (got["src"][r], got["dst"][r], got["type"][r]) == (w["src"], w["dst"], w["type"])
        assert got["weight"][r] == np.float32(w["weight"])
        for key, idx, vals in (("f", "fi", "fv"), ("u", "ui", "uv")):
            for f, end in enumerate(w[idx]):
                pre = 0 if f == 0 else w[idx][f - 1]
                assert list(slot(got[key], r, f)) == pytest.approx(vals and w[vals][pre:end])
        for f, end in enumerate(w["bi"]):
            pre = 0 if f == 0 else w["bi"][f - 1]
            assert slot(got["b"], r, f).tobytes() == w["bv"][pre:end]


def test_edge_features_of_the_reference_tests(L):
    # tf_euler/python/euler_ops/feature_ops_test.py:64-115
    rc, got = open_edges(FIXTURE)
    assert rc == 0
    trip = list(zip(got["src"].tolist(), got["dst"].tolist(), got["type"].tolist()))
    r = trip.index((1, 2, 0))
    assert list(slot(got["u"], r, 0)) == [121, 122]
    assert list(slot(got["u"], r, 1)) == [123, 124]
    assert np.allclose(slot(got["f"], r, 0), [12.1, 12.2])
    assert np.allclose(slot(got["f"], r, 1), [12.3, 12.4, 12.5])
    assert slot(got["b"], r, 0).tobytes() == b"12a"
    r = trip.index((2, 3, 1))
    assert np.allclose(slot(got["f"], r, 0), [23.1, 23.2])
    assert slot(got["b"], r, 0).tobytes() == b"23a"


def test_node_binary_features(L):
    from euler_amd import _lib
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
        table = (cnt.value, p, np.ctypeslib.as_array(idx, (n * cnt.value,)).copy(),
                 np.ctypeslib.as_array(val, (int(p[-1]),)).copy())
        assert cnt.value >= 2
        for node, f5, f6 in ((1, b"1a", b"1b"), (2, b"2a", b"2b")):
            r = rid.index(node)
            assert slot(table, r, 0).tobytes() == f5
            assert slot(table, r, 1).tobytes() == f6
    finally:
        L.euler_gpu_dat_close(owner)


def test_feature_names_from_meta(L):
    from euler_amd.graph import dat_feature_info
    assert dat_feature_info(FIXTURE, "dense_f4") == (1, 1, 3)
    assert dat_feature_info(FIXTURE, "binary_f6") == (2, 1, 0)
    assert dat_feature_info(FIXTURE, "sparse_f2", edge=True) == (0, 1, 654)
    assert dat_feature_info(FIXTURE, "dense_f3", edge=True) == (1, 0, 2)
    from euler_amd._lib import EulerGpuError
    with pytest.raises(EulerGpuError):
        dat_feature_info(FIXTURE, "dense_nope", edge=True)
    with pytest.raises(EulerGpuError):
        dat_feature_info(FIXTURE, "sparse_f11", edge=True)    # a node feature only


def test_truncated_edge_record_is_eio(L, tmp_path):
    from euler_amd import _lib
    d = tmp_path / "ds"
    shutil.copytree(FIXTURE, d)
    f = d / "Edge" / "data_1.dat"
    b = f.read_bytes()
    f.write_bytes(b[:-7])
    rc, _ = open_edges(d)
    assert rc == _lib.EIO
    # a record whose length prefix fits but whose fields do not
    n, = struct.unpack_from("<I", b, 0)
    f.write_bytes(struct.pack("<I", 12) + b[4:16])
    rc, _ = open_edges(d)
    assert rc == _lib.EIO


def test_repeated_triple_keeps_the_first_record(L, tmp_path):
    d = tmp_path / "ds"
    shutil.copytree(FIXTURE, d)
    f0 = (d / "Edge" / "data_0.dat").read_bytes()
    f1 = d / "Edge" / "data_1.dat"
    n, = struct.unpack_from("<I", f0, 0)
    first = bytearray(f0[:4 + n])
    struct.pack_into("<f", first, 4 + 20, 99.0)     # same (2, 3, 1), another weight
    f1.write_bytes(f1.read_bytes() + bytes(first))
    rc, got = open_edges(d)
    assert rc == 0 and len(got["src"]) == 12
    assert (got["src"][0], got["dst"][0], got["type"][0], got["weight"][0]) == (2, 3, 1, 3.0)

