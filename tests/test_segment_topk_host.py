"""The shared pieces of the fused per-column top-k (euler_amd/csrc/mp_topk.h), compiled with the
host compiler alone and driven over whole calls, against the numpy restatement
tests/segment_topk_ref.py: values and selected positions are bit-equal.  Also: the restatement
tells a non-sticky insertion chain apart, and the new C-ABI entries are exported and bound.
CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import segment_topk_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CODE = {"f32": 0, "bf16": 1, "f16": 2}
DIMS = [1, 3, 4, 8, 12, 64, 130]
KS = [1, 2, 3, 4, 5, 8, 16]


@pytest.fixture(scope="module")
def TK():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libsegment_topk_check.so")
    src = os.path.join(HERE, "csrc", "segment_topk_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h)
                    for h in ("mp_topk.h", "kg_score.h", "sparse_embed.h", "mp_weighted.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the host compiler alone, no HIP header
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.tk_call.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                          C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_void_p]
    L.tk_call.restype = C.c_int
    L.tk_chunk_width.argtypes = [C.c_int64, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.c_int32]
    L.tk_precedes.argtypes = [C.c_float, C.c_float]
    return L


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host(L, params, dt, gather, size, k, seg_ptr=None, count=0, fill=0.0, out_dt=None, e=None, want_sel=True):
    """one call of the host build -> (out, sel); out starts as a pattern no result has"""
    out_dt = out_dt or dt
    params = np.ascontiguousarray(params)
    if e is None:
        e = len(gather) if gather is not None else (size * count if seg_ptr is None else params.shape[0])
    d = params.shape[1]
    out = np.full((size, k, d), 0x7fc1 if out_dt != "f32" else 12345.0, ref.NP[out_dt])
    sel = np.full((size, k, d), -7, np.int32) if want_sel else None
    sp = None if seg_ptr is None else np.ascontiguousarray(seg_ptr, np.int64)
    rc = L.tk_call(ptr(params), CODE[dt], params.shape[0], ptr(gather),
                   int(gather is not None and gather.dtype == np.int64), ptr(sp), count, e, d, size, k, fill,
                   ptr(out), CODE[out_dt], ptr(sel))
    assert rc == 0
    return out, sel


def check(L, params, dt, gather, size, k, tag, **kw):
    got, sel = host(L, params, dt, gather, size, k, **kw)
    kw.pop("want_sel", None)
    want, want_sel = ref.topk(params, dt, gather, size, k, seg_ptr=kw.pop("seg_ptr", None),
                              count=kw.pop("count", 0) or None, **kw)
    out_dt = kw.get("out_dt") or dt
    assert ref.same(got, want, out_dt), tag
    assert np.array_equal(sel, want_sel), tag


@pytest.mark.parametrize("d", DIMS)
def test_host_build_equals_the_restatement(TK, d):
    """every k x storage type over tie-heavy tables; uniform (count) and ragged (seg_ptr) segments,
    k above the segment length, gather as int32 / int64 ids with ids that name no row / None,
    out as the input dtype and as fp32, fill 0 and -1e9"""
    rng = np.random.default_rng(200 + d)
    n = 0
    for k in KS:
        for dt in ref.DTYPES:
            rows = 23
            params = ref.tie_table(rng, (rows, d), dt)
            out_dt = "f32" if n % 2 else dt
            fill = -1e9 if n % 3 == 0 else 0.0
            size, count = 9, (1, 2, 3, 10, 17)[n % 5]
            e = size * count
            g32 = rng.integers(0, rows, e).astype(np.int32)
            ids = g32.astype(np.int64)
            ids[1::5] = np.resize(np.array([-1, rows, 2 ** 40, -2 ** 63], np.int64), len(ids[1::5]))
            tag = (d, k, dt, out_dt, count)
            check(TK, params, dt, g32, size, k, tag, count=count, fill=fill, out_dt=out_dt)
            check(TK, params, dt, ids, size, k, tag + ("ids",), count=count, fill=fill, out_dt=out_dt)
            ptr_ = ref.ragged_ptr(rng, size, max_len=20)
            e = int(ptr_[-1]) + 4
            ids = rng.integers(-2, rows + 2, e).astype(np.int64)
            check(TK, params, dt, ids, size, k, tag + ("ragged",), seg_ptr=ptr_, fill=fill, out_dt=out_dt)
            if n % 4 == 0:      # no gather array: position p reads row p, positions past the table read +0
                ptr_ = np.array([0, 5, 5, rows - 2, rows + 3], np.int64)
                check(TK, params, dt, None, 4, k, tag + ("none",), seg_ptr=ptr_, e=rows + 6, fill=fill, out_dt=out_dt)
            n += 1


def test_values_do_not_depend_on_sel(TK):
    """the kernel family without positions returns the same values"""
    rng = np.random.default_rng(3)
    params = ref.tie_table(rng, (30, 12), "bf16")
    g = rng.integers(0, 30, 70).astype(np.int32)
    for k in (1, 3, 16):
        a, _ = host(TK, params, "bf16", g, 7, k, count=10)
        b, none = host(TK, params, "bf16", g, 7, k, count=10, want_sel=False)
        assert none is None and ref.same(a, b, "bf16")


def non_sticky(values, k):
    """the WRONG insertion: a chain of independent compare-swaps that re-tests every slot"""
    slot, pos = [None] * k, [-1] * k
    for p, v in enumerate(values):
        for j in range(k):
            if pos[j] < 0 or v > slot[j]:
                slot[j], v = v, slot[j]
                pos[j], p = p, pos[j]
            if p < 0:
                break
    return pos


def test_the_restatement_tells_a_non_sticky_chain_apart(TK):
    values = np.array([[2.5], [2.5], [np.inf]], np.float32)
    out, sel = ref.topk(values, "f32", None, 1, 2, count=3)
    assert sel[0, :, 0].tolist() == [2, 0] and out[0, :, 0].tolist() == [np.inf, 2.5]
    assert non_sticky(values[:, 0], 2) == [2, 1]
    got, got_sel = host(TK, values, "f32", None, 1, 2, count=3)
    assert got_sel[0, :, 0].tolist() == [2, 0] and ref.same(got, out, "f32")


def test_order_and_special_values(TK):
    """NaN greatest, +0 == -0 and NaN == NaN keep position order, the bits of -0 survive"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for a, b, want in ((1.0, 0.5, 1), (0.5, 1.0, 0), (1.0, 1.0, 0), (0.0, -0.0, 0), (-0.0, 0.0, 0), (nan, inf, 1),
                       (inf, nan, 0), (nan, nan, 0), (-inf, nan, 0), (1e-45, 0.0, 1), (inf, -inf, 1)):
        assert TK.tk_precedes(a, b) == want, (a, b)
    v = np.array([[-0.0], [0.0], [np.nan], [-np.inf], [np.nan], [-0.0]], np.float32)
    out, sel = host(TK, v, "f32", None, 1, 5, count=6)
    assert sel[0, :, 0].tolist() == [2, 4, 0, 1, 5]
    assert out.view(np.uint32)[0, 2:, 0].tolist() == [0x80000000, 0, 0x80000000]


def test_capacity_chunk_width_and_einval(TK):
    assert [TK.tk_capacity(k) for k in range(1, 17)] == [1, 2, 4, 4, 8, 8, 8, 8] + [16] * 8
    # (d, params, params_f32, out, out_f32, sel, capacity)
    assert TK.tk_chunk_width(64, 32, 1, 64, 1, 0, 4) == 8 and TK.tk_chunk_width(64, 32, 1, 64, 1, 128, 4) == 8
    assert TK.tk_chunk_width(64, 32, 1, 64, 1, 128, 8) == 4 and TK.tk_chunk_width(64, 32, 1, 64, 1, 0, 16) == 4
    assert TK.tk_chunk_width(64, 32, 1, 64, 1, 128, 16) == 1
    assert TK.tk_chunk_width(12, 32, 1, 64, 1, 0, 1) == 4 and TK.tk_chunk_width(130, 32, 1, 64, 1, 0, 1) == 1
    assert TK.tk_chunk_width(64, 36, 1, 64, 1, 0, 1) == 1 and TK.tk_chunk_width(64, 32, 1, 64, 1, 132, 1) == 1
    assert TK.tk_chunk_width(64, 8, 0, 16, 0, 0, 1) == 4 and TK.tk_chunk_width(64, 34, 0, 16, 0, 0, 1) == 1
    p, o = np.zeros((4, 4), np.float32), np.zeros((2, 17, 4), np.float32)
    g = np.zeros(6, np.int32)
    sp = np.array([0, 3, 6], np.int64)

    def call(k=2, in_dt=0, out_dt=0, seg=None, count=3, e=6, params=p):
        return TK.tk_call(ptr(params), in_dt, 4, ptr(g), 0, ptr(seg), count, e, 4, 2, k, 0.0, ptr(o), out_dt, None)
    assert call() == 0 and call(seg=sp, count=0) == 0
    assert call(k=0) == -1 and call(k=17) == -1 and call(e=5) == -1 and call(in_dt=3) == -1
    assert call(in_dt=1, out_dt=2) == -1 and call(seg=sp) == -1 and call(count=0) == -1 and call(params=None) == -1


def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name, n_args in (("euler_gpu_gather_segment_topk", 16), ("euler_gpu_segment_topk_grad", 9)):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert name + "(" in hdr
        assert len(_lib.SIGNATURES[name][1]) == n_args


def test_sources_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "$(HERE)mp_topk.h" in mk and "segment_topk_kernels.hip" in mk


def test_op_is_public():
    from euler_amd import ops
    assert callable(ops.gather_segment_topk)
