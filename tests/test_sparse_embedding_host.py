"""The arithmetic of the sparse-feature embedding lookup (euler_amd/csrc/sparse_embed.h), compiled
with the host compiler and driven as the kernel drives it (entries handed over a group at a time,
the row cut into 16-byte chunks or single columns), against the numpy restatement
tests/sparse_embed_ref.py: bit equality, no tolerance.  CPU only.  Also: the new C-ABI entry is
exported, bound and declared, and the euler_ops export is there."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import sparse_embed_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
u64p = C.POINTER(C.c_uint64)
F32, BF16, F16 = 0, 1, 2
V, TOP = 97, 1 << 63
COUNTS = (0, 1, 2, 3, 7, 300)


@pytest.fixture(scope="module")
def SE():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libsparse_embed_check.so")
    src = os.path.join(HERE, "csrc", "sparse_embed_check.cc")
    inc = os.path.join(ROOT, "euler_amd", "csrc")
    deps = [src] + [os.path.join(inc, h) for h in ("sparse_embed.h", "mp_weighted.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # -ffp-contract=off: every sum of the header is its own rounding on the host too
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + inc, src, "-o", so])
    L = C.CDLL(so)
    L.se_row.argtypes = [u64p, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_int32, C.c_int64,
                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
    L.se_row.restype = C.c_int32
    L.se_group_lanes.argtypes = [C.c_int64]
    return L


def host_row(L, values, default, table, dtype, combiner, group, vec, out_dtype):
    """table: float32 array (dtype F32) or uint16 bit patterns -> (row of the out dtype's bits, cnt)"""
    v = np.ascontiguousarray(values, np.uint64)
    n_rows, dim = table.shape
    out = np.full(dim, 0xAAAA if out_dtype != F32 else np.nan, np.uint16 if out_dtype != F32 else np.float32)
    cnt = L.se_row(v.ctypes.data_as(u64p), len(v), int(default is not None),
                   (default or 0) % (1 << 64), table.ctypes.data, dtype, n_rows, dim,
                   ref.CODE[combiner], group, int(vec), out.ctypes.data, out_dtype)
    assert cnt >= 0
    return out, cnt


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def table32(dim, seed):
    """values of mixed sign and magnitude: sums that round at every step"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((V, dim)) * np.exp2(rng.integers(-6, 7, (V, 1)))).astype(np.float32)


def lists_for(rng):
    """(name, values): cnt in COUNTS by in-range entries alone, then the same with out-of-range
    entries (V, V + 1, 2^32 + 5, 2^63, 2^64 - 1) mixed in, lists of nothing but such entries."""
    far = np.array([V, V + 1, (1 << 32) + 5, TOP, TOP + 3, (1 << 64) - 1], np.uint64)
    out = []
    for c in COUNTS:
        inside = rng.integers(0, V, c).astype(np.uint64)
        out.append(("in%d" % c, inside))
        mixed = np.concatenate([inside, rng.choice(far, max(2, c // 3))])
        out.append(("mixed%d" % c, mixed[rng.permutation(len(mixed))]))
    out.append(("far1", far[:1]))
    out.append(("far", far))
    out.append(("far300", rng.choice(far, 300)))
    return out


@pytest.mark.parametrize("combiner", ref.COMBINERS)
@pytest.mark.parametrize("dim,vec", [(1, 0), (5, 0), (8, 0), (8, 1), (20, 1)])
def test_fp32_rows_equal_the_numpy_loop(SE, combiner, dim, vec):
    rng = np.random.default_rng(100 + dim)
    t = table32(dim, dim)
    for name, v in lists_for(rng):
        for default in (None, 7, V + 1, TOP + 9):
            want, want_cnt = ref.embed_row(v, default, t, combiner)
            for group in (1, 4, 64):
                got, cnt = host_row(SE, v, default, t, F32, combiner, group, vec, F32)
                assert cnt == want_cnt, (name, default, group)
                assert same(got, want), (name, default, group)
            # the expectations of the cases themselves
            if name.startswith("in"):
                n_in = int(name[2:])
                assert want_cnt == (n_in if n_in else (1 if default == 7 else 0))
            if name.startswith("far"):
                assert want_cnt == 0 and not want.any()


def test_counts_and_range_rule_by_hand(SE):
    """two rows by hand: the first row is taken as it is, the range rule is unsigned, the default
    is used only for an empty list and obeys the rule"""
    t = np.array([[-0.0, 1.0], [0.5, 3.0], [0.25, 5.0]], np.float32)

    def run(v, default, combiner):
        return host_row(SE, np.array(v, np.uint64), default, t, F32, combiner, 2, 0, F32)
    got, cnt = run([0], None, "sum")
    assert cnt == 1 and np.signbit(got[0]) and got[1] == 1          # -0.0 kept: not 0 + row
    got, cnt = run([1, 3, TOP + 1, 2, (1 << 32) + 1], None, "mean")
    assert cnt == 2 and got.tolist() == [0.375, 4.0]
    got, cnt = run([1, 2, 1], None, "sqrtn")
    want = (np.array([1.25, 11.0], np.float32) / np.sqrt(np.float32(3))).astype(np.float32)
    assert cnt == 3 and same(got, want)
    assert run([], None, "mean")[1] == 0 and not run([], None, "mean")[0].any()
    got, cnt = run([], 2, "sum")
    assert cnt == 1 and got.tolist() == [0.25, 5.0]
    got, cnt = run([], 3, "sum")
    assert cnt == 0 and got.tolist() == [0.0, 0.0]
    got, cnt = run([5], 1, "sum")                    # not empty: the default does not apply
    assert cnt == 0 and got.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("combiner", ref.COMBINERS)
def test_16bit_tables_widen_exactly_and_round_once(SE, dtype, combiner):
    import torch
    tt = torch.bfloat16 if dtype == BF16 else torch.float16
    rng = np.random.default_rng(7 + dtype)
    for dim, vec in ((3, 0), (8, 0), (8, 1), (16, 1)):
        stored = torch.from_numpy(table32(dim, 50 + dim)).to(tt)
        bits = stored.view(torch.int16).numpy().view(np.uint16)
        wide = stored.float().numpy()
        for name, v in lists_for(rng):
            for default in (None, 7, V + 1):
                want, want_cnt = ref.embed_row(v, default, wide, combiner)
                got32, cnt = host_row(SE, v, default, bits, dtype, combiner, 8, vec, F32)
                assert cnt == want_cnt and same(got32, want), (dim, vec, name, default)
                got16, cnt = host_row(SE, v, default, bits, dtype, combiner, 8, vec, dtype)
                want16 = torch.from_numpy(want).to(tt).view(torch.int16).numpy().view(np.uint16)
                assert cnt == want_cnt and np.array_equal(got16, want16), (dim, vec, name, default)


def test_restatement_all_nodes_at_once_equals_the_row_loop():
    """ref.embed (what the GPU tests compare with) against ref.embed_row, node by node"""
    rng = np.random.default_rng(3)
    t = table32(6, 9)
    lists = [v for _, v in lists_for(rng)] + [np.zeros(0, np.uint64)]
    for combiner in ref.COMBINERS:
        for default in (None, 7, V + 1):
            out, counts = ref.embed(lists, default, t, combiner)
            for i, v in enumerate(lists):
                want, cnt = ref.embed_row(v, default, t, combiner)
                assert counts[i] == cnt and same(out[i].copy(), want), (combiner, default, i)


def test_group_lanes(SE):
    """the lane group of a row: the power of two that covers its chunks, 64 at the most"""
    assert [SE.se_group_lanes(c) for c in (1, 2, 3, 4, 5, 16, 17, 64, 65, 130)] == \
        [1, 2, 4, 4, 8, 16, 32, 64, 64, 64]


def test_new_entry_is_exported_bound_and_declared():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    name = "euler_gpu_sparse_feature_embedding"
    assert name in _lib.SIGNATURES
    assert hasattr(L, name)
    assert name + "(" in hdr
    assert len(_lib.SIGNATURES[name][1]) == 15
    from euler_amd import Graph, euler_ops
    from euler_amd.euler_ops import feature_ops
    assert euler_ops.sparse_feature_embedding is feature_ops.sparse_feature_embedding
    assert callable(Graph.sparse_feature_embedding)


def test_header_and_kernel_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "sparse_embed.h" in mk and "feature_kernels.hip" in mk
