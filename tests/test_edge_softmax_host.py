"""The arithmetic of edge_softmax (euler_amd/csrc/mp_softmax.h), compiled with the host compiler,
against the numpy restatement tests/edge_softmax_ref.py: bit equality, no tolerance.  The error E
of ExpNonPositive is re-measured on a fixed subsample and held against the recorded constant, and
the float64 bounds of DESIGN 4.11 are checked on the host results.  CPU only.  Also: the new C-ABI
entries are exported and bound."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import edge_softmax_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
NEW_SYMBOLS = ["euler_gpu_edge_softmax", "euler_gpu_edge_softmax_grad"]


@pytest.fixture(scope="module")
def SMX():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libedge_softmax_check.so")
    src = os.path.join(HERE, "csrc", "edge_softmax_check.cc")
    inc = os.path.join(ROOT, "euler_amd", "csrc")
    deps = [src] + [os.path.join(inc, h) for h in ("mp_softmax.h", "mp_weighted.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # -ffp-contract=off: every product and sum of the header is its own rounding on the host too
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + inc, src, "-o", so])
    L = C.CDLL(so)
    L.smx_floor.restype = C.c_float
    L.smx_exp.argtypes = [f32p, C.c_int64, f32p]
    L.smx_exp_error.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    L.smx_exp_error.restype = C.c_double
    L.smx_forward.argtypes = [f32p, C.c_int64, C.c_int32, f32p]
    L.smx_backward.argtypes = [f32p, f32p, C.c_int64, C.c_int32, f32p]
    return L


def host_exp(L, d):
    d = np.ascontiguousarray(d, np.float32)
    out = np.empty_like(d)
    L.smx_exp(d.ctypes.data_as(f32p), d.size, out.ctypes.data_as(f32p))
    return out


def host_forward(L, x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.full_like(x, np.nan)
    assert L.smx_forward(x.ctypes.data_as(f32p), x.shape[0], x.shape[1], y.ctypes.data_as(f32p)) == 0
    return y


def host_backward(L, y, g):
    y, g = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(g, np.float32)
    gx = np.full_like(y, np.nan)
    assert L.smx_backward(y.ctypes.data_as(f32p), g.ctypes.data_as(f32p), y.shape[0], y.shape[1],
                          gx.ctypes.data_as(f32p)) == 0
    return gx


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_exp_equals_the_numpy_restatement_on_the_subsample(SMX):
    assert SMX.smx_floor() == ref.T
    d = ref.exp_subsample().view(np.float32)
    assert d.size > 500_000 and d.max() == 0 and d.min() == ref.T
    got = host_exp(SMX, d)
    assert same(got, ref.exp_nonpositive(d))
    # every result is +0 or a normal number: nothing can depend on the handling of denormals
    assert np.all((got == 0) | (got >= np.float32(2.0 ** -126))) and not np.any(np.signbit(got))


def test_exp_fixed_points(SMX):
    below = np.nextafter(ref.T, np.float32(-np.inf))
    d = np.array([0.0, -0.0, ref.T, below, -1e30, -np.inf, np.nan], np.float32)
    got = host_exp(SMX, d)
    assert same(got, ref.exp_nonpositive(d))
    assert got[0].view(np.uint32) == np.float32(1).view(np.uint32) and got[1] == 1
    assert got[2] > 0
    assert np.all(got[3:].view(np.uint32) == 0)          # exactly +0.0f


def test_exp_error_does_not_exceed_the_recorded_constant(SMX):
    """E_ULP was measured over every fp32 value in [T, 0]; here: the same measure on the subsample,
    by the check program (float64 exp of libm) and by numpy, held against it."""
    bits = ref.exp_subsample()
    d = bits.view(np.float32)
    by_numpy = ref.ulp_error(host_exp(SMX, d), d).max()
    worst = C.c_uint32(0)
    lo, hi = 0x80000000, int(np.array(ref.T).view(np.uint32))
    strided = SMX.smx_exp_error(lo, hi, 4099, C.byref(worst))
    windows = 0.0
    for ex in list(range(-126, 7)) + [None]:
        c = hi - 2048 if ex is None else int(np.array(np.float32(-(2.0 ** ex))).view(np.uint32))
        windows = max(windows, SMX.smx_exp_error(max(lo, c - 2048), min(hi, c + 2048), 1, C.byref(worst)))
    print("E on the subsample: numpy %.6f, check program %.6f (stride) %.6f (windows); recorded %.4f"
          % (by_numpy, strided, windows, ref.E_ULP))
    assert by_numpy <= ref.E_ULP
    assert strided <= ref.E_ULP and windows <= ref.E_ULP


def logits(rng, n, heads, kind):
    x = (rng.standard_normal((n, heads)) * 3).astype(np.float32)
    if kind == "threshold" and n > 1:          # differences to the maximum on both sides of T
        x[0] = 40.0
        x[1:] = (40.0 + np.float64(ref.T) + rng.uniform(-3, 3, (n - 1, heads))).astype(np.float32)
        x[1] = np.float32(40.0) + ref.T - np.float32(1.5)    # below T: flushed
        if n > 2:
            x[2] = np.float32(40.0) + ref.T               # d == T exactly
    elif kind == "neg_inf" and n > 1:
        x[rng.integers(0, n)] = -np.inf
        x[0, 0] = 1.0                                       # (a finite maximum in every head)
        x[0] = np.where(np.isfinite(x[0]), x[0], 1.0)
    elif kind == "equal_max":
        x[: max(1, n // 2)] = np.float32(2.5)
        x = np.minimum(x, np.float32(2.5))
    return x


# 0; 1; 7 and 32: the one-lane order (n <= 32); 33 and 300: the 256-partial tree with one term a
# partial at most / with partials of two terms; 5000: partials that loop, four loads at a time
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("n", [0, 1, 7, 32, 33, 300, 5000])
@pytest.mark.parametrize("kind", ["plain", "threshold", "neg_inf", "equal_max"])
def test_forward_and_backward_equal_the_numpy_restatement(SMX, heads, n, kind):
    rng = np.random.default_rng(1000 * heads + n)
    x = logits(rng, n, heads, kind)
    y = host_forward(SMX, x)
    if n == 0:
        return
    want = ref.forward_batch(x[None], heads)[0]
    assert same(y, want)
    sp = np.array([0, n], np.int64)
    assert same(want, ref.edge_softmax_ref(x, sp))
    if kind == "neg_inf" and n > 1:
        assert np.all(y[np.isneginf(x)].view(np.uint32) == 0)
    if kind == "threshold" and n > 2:
        assert np.any(y == 0) and np.any((y > 0) & (y < 1e-30))
    if kind == "equal_max":
        assert np.all(y.max(axis=0) == y[0])
    # contract B, forward, on the host bits
    err = np.abs(y.astype(np.float64) - ref.forward_f64(x, sp))
    bound = ref.forward_bound(x, sp, ref.E_ULP)
    assert np.all(err <= bound), float((err / bound).max())
    g = (rng.standard_normal((n, heads)) * 2).astype(np.float32)
    gx = host_backward(SMX, y, g)
    assert same(gx, ref.backward_batch(y[None], g[None], heads)[0])
    assert same(gx, ref.edge_softmax_ref(y, sp, g))
    err = np.abs(gx.astype(np.float64) - ref.backward_f64(y, g, sp))
    assert np.all(err <= ref.backward_bound(y, g, sp))


def test_heads_that_do_not_divide_64_take_one_head_at_a_time(SMX):
    rng = np.random.default_rng(5)
    for heads in (3, 8, 64):
        x = (rng.standard_normal((700, heads)) * 4).astype(np.float32)
        y = host_forward(SMX, x)
        assert same(y, ref.forward_batch(x[None], heads)[0])
        g = rng.standard_normal((700, heads)).astype(np.float32)
        assert same(host_backward(SMX, y, g), ref.backward_batch(y[None], g[None], heads)[0])
    assert [ref.heads_per_wave(h) for h in (1, 3, 8, 64, 128)] == [1, 1, 8, 64, 1]


@pytest.mark.parametrize("n", [7, 32, 33, 300])
def test_a_nan_logit_is_left_out_of_the_maximum_whatever_the_length(SMX, n):
    """Outside the contract, but documented: every fold of the maximum starts from -inf, so a NaN
    logit - the first of its segment included - gets 0 and the others their softmax."""
    rng = np.random.default_rng(n)
    for at in (0, n // 2, n - 1):
        x = (rng.standard_normal((n, 2)) * 3).astype(np.float32)
        x[at, 0] = np.nan
        y = host_forward(SMX, x)
        assert y[at, 0].view(np.uint32) == 0
        rest = np.delete(y[:, 0], at)
        assert np.all(np.isfinite(rest)) and abs(float(rest.astype(np.float64).sum()) - 1) < 1e-5
        with np.errstate(invalid="ignore"):
            want = ref.forward_batch(x[None], 2)[0]
        assert same(y[:, 1].copy(), want[:, 1].copy())                              # the other head
        if n <= ref.SHORT:          # (+0 added to the sum leaves its bits: the softmax of the others)
            others = np.delete(x[:, :1], at, axis=0)
            assert same(rest, ref.forward_batch(others[None], 1)[0][:, 0].copy())


def test_restatement_against_plain_loops():
    """the restatement itself: the vectorised sum == the stated order written as loops"""
    rng = np.random.default_rng(11)
    for n, heads in ((20, 2), (300, 4), (300, 3)):
        t = rng.random((1, n, heads)).astype(np.float32)
        got = ref.ordered_sum(t, heads)[0]
        for h in range(heads):
            if n <= ref.SHORT:
                s = np.float32(0)
                for p in range(n):
                    s = np.float32(s + t[0, p, h])
            else:
                w = ref.BLOCK // ref.heads_per_wave(heads)
                part = []
                for l in range(w):
                    s = np.float32(0)
                    for p in range(l, n, w):
                        s = np.float32(s + t[0, p, h])
                    part.append(s)
                run = w // 4
                off = run // 2
                while off >= 1:
                    part = [np.float32(part[l] + part[(l // run) * run + ((l % run) ^ off)]) for l in range(w)]
                    off //= 2
                s = np.float32(np.float32(part[0] + part[run]) + np.float32(part[2 * run] + part[3 * run]))
            assert s.view(np.uint32) == got[h].view(np.uint32)


def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    from euler_amd import ops
    from euler_amd.euler_ops import mp_ops
    assert mp_ops.edge_softmax is ops.edge_softmax


def test_header_and_kernels_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "mp_softmax.h" in mk and "edge_softmax_kernels.hip" in mk
