"""The arithmetic of attention_aggregate (euler_amd/csrc/mp_attention.h), compiled with the host
compiler, against the numpy restatement tests/segment_attention_ref.py: bit equality, no
tolerance; the logit against float64 within the derived bound; alpha and out against the
restatements of edge_softmax and of the weighted fold.  CPU only.  Also: the new C-ABI entries are
exported and bound."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import edge_softmax_ref as es
import segment_attention_ref as ref
import weighted_mp_ref as wref

HERE = os.path.dirname(os.path.abspath(__file__))
f32p, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
NEW_SYMBOLS = ["euler_gpu_segment_attention", "euler_gpu_segment_attention_grad"]
LENGTHS = [0, 1, 7, 16, 17, 32, 33, 300]
KIND = {"dot": 0, "additive": 1}


@pytest.fixture(scope="module")
def ATT():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libsegment_attention_check.so")
    src = os.path.join(HERE, "csrc", "segment_attention_check.cc")
    inc = os.path.join(ROOT, "euler_amd", "csrc")
    deps = [src] + [os.path.join(inc, h) for h in ("mp_attention.h", "mp_softmax.h", "mp_weighted.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # -ffp-contract=off: every product and sum of the header is its own rounding on the host too
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + inc, src, "-o", so])
    L = C.CDLL(so)
    head = [C.c_int32, f32p, C.c_int64, i32p, f32p, C.c_int64, f32p, C.c_int64, i64p, i64p, C.c_int32, C.c_int64,
            C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_float]
    L.att_forward.argtypes = head + [f32p, f32p, f32p]
    L.att_backward.argtypes = head + [f32p, f32p, f32p, f32p]
    L.att_chunk.argtypes = L.att_lanes.argtypes = [C.c_int64]
    return L


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Case(object):
    """one call on seg_ptr form: 8 destinations of the LENGTHS (shuffled), a table of 41 rows, gather
    rows with a few past the table, q_index with repeats"""

    def __init__(self, kind, heads, width, shared, slope=0.2, scale=0.37, seed=0, with_q=True, v_width=None):
        rng = np.random.default_rng(seed + 1000 * heads + width)
        self.kind, self.heads, self.scale, self.slope = kind, heads, scale, slope
        lens = rng.permutation(LENGTHS)
        self.seg_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.size, self.e = len(lens), int(self.seg_ptr[-1])
        rows = 41
        d = heads if kind == "additive" else heads * width
        dv = d if shared else heads * (v_width or width)
        self.q = rng.standard_normal((5, d)).astype(np.float32) if with_q else None
        self.q_index = rng.integers(0, 5, self.size).astype(np.int32)
        self.k = rng.standard_normal((rows, d)).astype(np.float32)
        self.v = None if shared else rng.standard_normal((rows + 3, dv)).astype(np.float32)
        self.gi = rng.integers(0, rows + 2, self.e).astype(np.int64)
        self.grad = rng.standard_normal((self.size, dv)).astype(np.float32)
        self.d, self.dv = d, dv

    def head_args(self):
        v = self.v
        return [KIND[self.kind], _p(self.q, f32p), 5, _p(self.q_index, i32p), _p(self.k, f32p), self.k.shape[0],
                _p(v, f32p), v.shape[0] if v is not None else 0, _p(self.gi, i64p), _p(self.seg_ptr, i64p),
                self.size, self.e, self.d, self.dv, self.heads, self.scale, self.slope]

    def host_forward(self, L):
        x = np.full((self.e, self.heads), np.nan, np.float32)
        a = np.full_like(x, np.nan)
        out = np.full((self.size, self.dv), np.nan, np.float32)
        assert L.att_forward(*(self.head_args() + [_p(x, f32p), _p(a, f32p), _p(out, f32p)])) == 0
        return x, a, out

    def host_backward(self, L, alpha):
        ds = np.full((self.e, self.heads), np.nan, np.float32)
        dq = np.full((self.size, self.d), np.nan, np.float32)
        assert L.att_backward(*(self.head_args() + [_p(alpha, f32p), _p(self.grad, f32p), _p(ds, f32p),
                                                     _p(dq, f32p)])) == 0
        return ds, dq

    def ref_args(self):
        return (self.kind, self.q, self.k, self.v, self.gi, self.seg_ptr, self.heads)

    def ref_kw(self):
        return dict(q_index=self.q_index, scale=self.scale, slope=self.slope)


def check_case(L, c):
    x, a, out = c.host_forward(L)
    rx, ra, rout = ref.forward(*c.ref_args(), **c.ref_kw())
    assert same(x, rx) and same(a, ra) and same(out, rout)
    # 3: given the logits, alpha is edge_softmax's; given alpha, out is the weighted fold's
    assert same(a, es.edge_softmax_ref(rx, c.seg_ptr))
    tv = c.k if c.v is None else c.v
    dst = wref.segment_dst(c.size, seg_ptr=c.seg_ptr)
    assert same(out, wref.gather_scatter_ref("add", tv, ref.rows_of(c.gi, tv.shape[0]), dst, c.size, ra))
    # 2: the logit within the derived bound of float64, no margin
    x64, bound = ref.logits_f64(c.kind, c.q, c.k, c.gi, c.seg_ptr, c.heads, **c.ref_kw())
    err = np.abs(x.astype(np.float64) - x64)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    ds, dq = c.host_backward(L, a)
    rds, rdq = ref.backward(*c.ref_args(), alpha=ra, grad=c.grad, **c.ref_kw())
    assert same(ds, rds) and same(dq, rdq)
    # every destination's alpha sums to 1 within the softmax's own error; an empty one is a zero row
    for r in range(c.size):
        b, en = c.seg_ptr[r], c.seg_ptr[r + 1]
        if en == b:
            assert not out[r].any() and not dq[r].any()
        else:
            assert np.all(np.abs(a[b:en].astype(np.float64).sum(0) - 1) < 1e-4)


@pytest.mark.parametrize("width", [1, 4, 5, 32])
@pytest.mark.parametrize("heads", [1, 3, 4, 8])
def test_dot_equals_the_numpy_restatement(ATT, heads, width):
    check_case(ATT, Case("dot", heads, width, shared=False))
    check_case(ATT, Case("dot", heads, width, shared=True, seed=1))       # v=None: v is k


@pytest.mark.parametrize("width", [1, 4, 5, 32])
@pytest.mark.parametrize("heads", [1, 3, 4, 8])
def test_additive_equals_the_numpy_restatement(ATT, heads, width):
    check_case(ATT, Case("additive", heads, width, shared=False, slope=0.2))
    check_case(ATT, Case("additive", heads, width, shared=False, slope=1.0, seed=2))
    check_case(ATT, Case("additive", heads, width, shared=False, slope=1.0, seed=3, with_q=False))


def test_an_fma_would_change_the_logit(ATT):
    """dh = 4 is one partial: -1 from column 0, then q = k = 1 + 2^-12 in column 1.  The product
    1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 before it is added to the -1, where a fused multiply-add
    would keep the 2^-24"""
    c = Case("dot", 1, 4, shared=False, scale=1.0)
    c.q[:] = 0
    c.k[:] = 0
    c.q[:, 0] = -1.0
    c.k[:, 0] = 1.0
    c.q[:, 1] = c.k[:, 1] = np.float32(1 + 2.0 ** -12)
    x, _, _ = c.host_forward(ATT)
    rx = ref.logits(c.kind, c.q, c.k, c.gi, c.seg_ptr, c.heads, **c.ref_kw())
    assert same(x, rx)
    live = x[: c.e, 0]
    assert np.all(live == np.float32(2.0 ** -11))
    fused = (1 + 2.0 ** -12) ** 2 - 1.0
    assert np.float32(fused) != np.float32(2.0 ** -11)


def test_two_tables_of_different_widths(ATT):
    """Dv != D: the backward's dot runs over dv, its fold over d"""
    check_case(ATT, Case("dot", 4, 5, shared=False, v_width=32))
    check_case(ATT, Case("dot", 3, 32, shared=False, v_width=1, seed=4))
    check_case(ATT, Case("additive", 8, 1, shared=False, v_width=5, seed=5))


def test_the_header_lane_layout_equals_the_restatement(ATT):
    for dh in list(range(1, 700)) + [1024, 4096, 4100]:
        assert ATT.att_chunk(dh) == ref.chunk(dh), dh
        assert ATT.att_lanes(dh) == ref.lanes(dh), dh


def test_the_order_of_the_dot_is_a_function_of_dh_alone():
    assert [(ref.chunk(d), ref.lanes(d)) for d in (1, 4, 5, 20, 32, 128, 1024)] == \
        [(1, 1), (4, 1), (1, 8), (4, 8), (4, 8), (4, 32), (4, 64)]
    rng = np.random.default_rng(3)
    for dh in (1, 4, 5, 20, 32, 300):
        a = rng.standard_normal((6, dh)).astype(np.float32)
        b = rng.standard_normal((6, dh)).astype(np.float32)
        got = ref.dot(a, b)
        v, L = ref.chunk(dh), ref.lanes(dh)
        for i in range(6):                     # the restatement itself, against plain loops
            part = [np.float32(0)] * L
            for l in range(L):
                for j in range(l, dh // v, L):
                    for c in range(j * v, j * v + v):
                        part[l] = np.float32(part[l] + np.float32(a[i, c] * b[i, c]))
            off = L // 2
            while off >= 1:
                part = [np.float32(part[l] + part[l ^ off]) for l in range(L)]
                off //= 2
            assert part[0].view(np.uint32) == got[i].view(np.uint32)


def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    from euler_amd import ops
    assert callable(ops.attention_aggregate)


def test_header_and_kernels_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "mp_attention.h" in mk and "segment_attention_kernels.hip" in mk
