"""The 12-bit header + window lines of euler_amd/csrc/wb_hw2.h - hop 2 of the plain-graph fanout
step with two index requests per draw (tuning key 76) - compiled for the HOST by
tests/csrc/hw2_check.hip and compared with the oracle's RandomSelect: build, then draw, then
(index, weight).  The lines of wb_hw.h are built over the same rows, so that the share of draws
the new header does not settle with its first window is compared with the share the current
header sends to its second entry, on the same draws.  CPU only; the kernels' lane mapping is
covered by tests/test_fanout_hw2_gpu.py.  Skipped when hipcc is absent."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
u64p, i64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
f32p, u32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_double)

EDGE_U = (0.0, 1.0 - 2.0 ** -53, 0.5, 2.0 ** -40)
DEGS = [0, 1, 2, 3, 9, 10, 11, 12, 13, 17, 20, 21, 37, 40, 41, 64, 65, 100, 257, 1000, 4099]


def _p(a, t):
    return a.ctypes.data_as(t)


@pytest.fixture(scope="module")
def HW2():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libhw2_check.so")
    src = os.path.join(HERE, "csrc", "hw2_check.hip")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", f)
                    for f in ("wb_hw2.h", "wb_hw.h", "wb_index.h", "device_fns.h", "common.h", "philox.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(
            [hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
             "-ffp-contract=off", "-I" + os.path.join(ROOT, "euler_amd", "csrc"),
             "-I" + os.path.join(ROOT, "include"), src, "-o", so])
    L = C.CDLL(so)
    L.hw2_build.restype = C.c_void_p
    L.hw2_build.argtypes = [C.c_int64, i64p, f32p, u64p]
    L.hw2_destroy.argtypes = [C.c_void_p]
    L.hw2_lines.restype = C.c_int64
    L.hw2_lines.argtypes = [C.c_void_p]
    L.hw2_overflows.restype = C.c_int64
    L.hw2_overflows.argtypes = [C.c_void_p]
    L.hw2_line.argtypes = [C.c_void_p, C.c_int64, C.c_int32, u32p]
    L.hw2_sample.argtypes = [C.c_void_p, i64p, f64p, C.c_int64, u64p, f32p, i32p, i32p]
    return L


def _buckets(d):
    return 0 if d == 0 else 1 if d <= 10 else (d + 3) // 4


def _codes(ln):
    """the eight 12-bit codes of a line's words 0 .. 2"""
    bits = int(ln[0]) | (int(ln[1]) << 32) | (int(ln[2]) << 64)
    return [(bits >> (12 * k)) & 4095 for k in range(8)]


class Case:
    """Rows of the given degrees with weights from weight_fn(deg); neighbour ids are distinct, so
    an id names its edge."""

    def __init__(self, L, O, degs, weight_fn, rng):
        self.L, self.degs = L, list(degs)
        ws = [np.asarray(weight_fn(d), np.float32) for d in degs]
        assert all(len(w) == d for w, d in zip(ws, degs))
        segs = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
        w_all = np.concatenate(ws) if ws else np.zeros(0, np.float32)
        nbr = (rng.permutation(len(w_all)).astype(np.uint64) + np.uint64(1)) * np.uint64(2 ** 33 + 7)
        n = len(degs)
        self.csr = O.csr_from_raw(np.arange(1, n + 1, dtype=np.uint64), segs, nbr, w_all, 1)
        self.row_ptr = np.ascontiguousarray(self.csr.row_ptr, np.int64)
        self.pw = np.ascontiguousarray(self.csr.prefix_w, np.float32)
        self.nbr = np.ascontiguousarray(self.csr.nbr, np.uint64)
        self.h = L.hw2_build(n, _p(self.row_ptr, i64p), _p(self.pw, f32p), _p(self.nbr, u64p))
        self.lines = L.hw2_lines(self.h)
        self.overflows = L.hw2_overflows(self.h)

    def __del__(self):
        self.L.hw2_destroy(self.h)

    def line(self, i, which=0):
        out = np.zeros(32, np.uint32)
        self.L.hw2_line(self.h, i, which, _p(out, u32p))
        return out

    def check_build(self):
        """every line: words 3 .. 31 are those of the line wb_hw.h builds for the same bucket (nine
        consecutive edges behind an exact sum, +inf / id 0 past the row's end, the flat index of
        entry 0); the eight codes are non-decreasing over the real entries, at most 4094 there
        and 4095 past the row's end; a sum inside the bucket's span has a code below 4094"""
        assert self.lines == sum(_buckets(d) for d in self.degs)
        at = 0
        for r, d in enumerate(self.degs):
            b = int(self.row_ptr[r])
            sw = self.pw[b:b + d]
            nbk = _buckets(d)
            for j in range(nbk):
                ln, old = self.line(at), self.line(at, 1)
                at += 1
                assert np.array_equal(ln[3:], old[3:])
                s = int(ln[31]) - b
                assert 0 <= s < d and (j > 0 or s == 0)
                c = _codes(ln)
                with np.errstate(all="ignore"):
                    scale = np.float32(nbk) / sw[-1]
                for k in range(8):
                    if s + k < d:
                        assert c[k] <= 4094 and (k == 0 or c[k] >= c[k - 1])
                        with np.errstate(all="ignore"):
                            pos = np.float32(sw[s + k] * scale) - np.float32(j)
                        if np.isfinite(pos):
                            assert (c[k] == 4094) == bool(pos >= 1), (r, j, k, pos, c[k])
                            if pos < 0:
                                assert c[k] == 0
                            elif pos < 1:
                                assert c[k] == min(4093, int(np.float32(pos * np.float32(4094))))
                    else:
                        assert c[k] == 4095

    def draw(self, O, rng, per_row=64, extra_u=EDGE_U):
        """counts {draws, first, second, cold, old_second} after checking every hot draw against
        the oracle, bit for bit; a cold draw is the caller's RandomSelect by definition.
        old_second: the draws HwSampleHot (wb_hw.h) settles with the entry before its guess."""
        n = len(self.degs)
        rows = np.repeat(np.arange(n, dtype=np.int64), per_row + len(extra_u))
        us = np.concatenate([np.concatenate([rng.random(per_row), np.asarray(extra_u, np.float64)])
                             for _ in range(n)])
        ids = np.zeros(len(rows), np.uint64)
        w = np.zeros(len(rows), np.float32)
        win = np.zeros(len(rows), np.int32)
        old = np.zeros(len(rows), np.int32)
        self.L.hw2_sample(self.h, _p(rows, i64p), _p(us, f64p), len(rows), _p(ids, u64p), _p(w, f32p),
                          _p(win, i32p), _p(old, i32p))
        k = {"draws": 0, "first": 0, "second": 0, "cold": 0, "old_second": 0}
        for i in range(len(rows)):
            r = int(rows[i])
            d = self.degs[r]
            if d == 0:
                assert win[i] == -3
                continue
            k["draws"] += 1
            k["old_second"] += int(old[i] == 2)
            b = int(self.row_ptr[r])
            sw = self.pw[b:b + d]
            if win[i] <= 0:
                k["cold"] += 1
                assert ids[i] == 0 and w[i] == 0          # a cold draw reports nothing
                # a draw that rounds up to the row's total never sees a line
                rounds_up = not (np.float64(sw[-1]) > np.float64(us[i]) * np.float64(sw[-1]))
                assert (win[i] == 0) == rounds_up, (r, d, us[i])
                continue
            want = O.random_select(sw, 0, d - 1, float(us[i]))
            assert ids[i] == self.nbr[b + want], (r, d, us[i], want, int(win[i]))
            ww = np.float32(sw[want]) - (np.float32(sw[want - 1]) if want else np.float32(0))
            assert w[i:i + 1].view(np.uint32)[0] == np.asarray([ww], np.float32).view(np.uint32)[0]
            k["first"] += int(win[i] == 1)
            k["second"] += int(win[i] == 2)
        assert k["draws"] == k["first"] + k["second"] + k["cold"]
        return k


def _giant(rng):
    def f(d):
        w = np.full(d, 1e-3)
        if d:
            w[int(rng.integers(0, d))] = 1e6
        return w
    return f


def _families(rng):
    return [
        ("uniform", lambda d: 0.5 + 7.5 * rng.random(d)),
        ("equal", lambda d: np.full(d, 0.37)),
        ("ones", lambda d: np.ones(d)),
        ("pareto", lambda d: rng.pareto(0.7, d) + 1e-3),
        ("zeros mixed in", lambda d: np.where(rng.random(d) < 0.4, 0.0, rng.random(d))),
        ("giant among dust", _giant(rng)),
        ("ramp up", lambda d: np.arange(1, d + 1, dtype=np.float64)),
        ("ramp down", lambda d: np.arange(d, 0, -1, dtype=np.float64) ** 2),
        ("all zero", lambda d: np.zeros(d)),
        ("denormal", lambda d: np.full(d, 1e-42)),
        ("huge", lambda d: np.full(d, 1e36)),
    ]


def test_hw2_lines_vs_random_select(HW2, O):
    """Every weight family of tests/test_host_check.py's weight-bucket test, over rows of 1, 9, 10
    and 11 edges, rows with equal consecutive sums (zero weights), rows whose sums share quanta
    (dust beside a giant) and a row of 4 099 edges: the lines are built as documented, and every
    draw either returns exactly RandomSelect's (id, weight) or reports cold."""
    rng = np.random.default_rng(212)
    for name, fn in _families(rng):
        small = name in ("all zero", "denormal", "huge")
        c = Case(HW2, O, [1, 5, 10, 30, 200] if small else DEGS, fn, rng)
        c.check_build()
        k = c.draw(O, rng, per_row=8 if small else 64)
        if name == "all zero":
            assert k["cold"] == k["draws"]        # total 0: every draw rounds up to it
        if name in ("uniform", "equal", "ones", "ramp up"):
            assert k["first"] > 0.95 * k["draws"], (name, k)


def test_hw2_draws_that_round_up_to_the_total_are_cold(HW2, O):
    rng = np.random.default_rng(213)
    c = Case(HW2, O, [1, 9, 10, 11, 37], lambda d: 0.5 + 7.5 * rng.random(d), rng)
    k = c.draw(O, rng, per_row=0, extra_u=(1.0,))
    assert k["draws"] == 5 and k["cold"] == 5
    k = c.draw(O, rng, per_row=0, extra_u=(1.0 - 2.0 ** -53,))
    assert k["draws"] == 5 and k["first"] + k["second"] >= 4     # (the row of 10 edges: its last edge is not in the line)
    z = Case(HW2, O, [1, 9, 10, 11, 37], lambda d: np.zeros(d), rng)
    k = z.draw(O, rng, per_row=4, extra_u=(0.0,))
    assert k["cold"] == k["draws"] == 25


def test_hw2_overflowing_lines_go_cold(HW2, O):
    """A last bucket that holds more than nine edges' intervals, and a row of exactly 10 edges:
    the builder counts the overflow, the draws beyond the ninth entry are cold, the others exact."""
    rng = np.random.default_rng(214)

    def tail(d):
        w = np.full(d, 8.0)
        w[-14:] = 0.05
        return w
    c = Case(HW2, O, [37], tail, rng)
    c.check_build()
    assert c.overflows >= 1
    tot = float(c.pw[-1])
    us = tuple(1.0 - (i + 0.5) * 0.05 / tot for i in range(14))
    k = c.draw(O, rng, per_row=256, extra_u=us)
    assert k["cold"] >= 3 and k["first"] + k["second"] > 0.9 * k["draws"]
    c10 = Case(HW2, O, [10], lambda d: np.ones(d), rng)
    assert c10.overflows == 1
    k = c10.draw(O, rng, per_row=400, extra_u=(0.95, 0.999))
    assert k["cold"] >= 2 and 0.05 * k["draws"] < k["cold"] < 0.16 * k["draws"]


def test_hw2_shared_quanta_take_the_second_window_or_go_cold(HW2, O):
    """Dust behind giants: the dust's sums share one 12-bit code, so a draw aimed at it is guessed
    too high - by one (second window) or by more (cold) - and the keys still decide."""
    rng = np.random.default_rng(215)

    def w(d):
        x = np.full(d, 1e-4)
        x[::7] = 1e3
        x[1::7] = 3e-4
        return x
    c = Case(HW2, O, [37, 200, 1000], w, rng)
    c.check_build()
    b = int(c.row_ptr[1])
    sw = c.pw[b:b + c.degs[1]].astype(np.float64)
    us = [(sw[i] + 1e-4 * (1 + (i % 5))) / sw[-1] for i in range(0, c.degs[1] - 8, 7)][:5]
    k = c.draw(O, rng, per_row=64, extra_u=tuple(np.clip(us, 0, 1 - 1e-9)))
    assert k["second"] + k["cold"] > 0, k


def test_hw2_rates_on_uniform_weights(HW2, O):
    """i.i.d. uniform [0.5, 8) weights - the metric graph's - over rows of every degree from 1 to 64
    and a few large ones, equally many draws per row.  The three rates are printed (DESIGN 4.2
    records them); the condition: the draws the first window does not settle - second window and
    cold together - are fewer than the draws the CURRENT header (wb_hw.h, HwSampleHot's
    `windows`) sends to its second entry, on the same rows and the same draws."""
    rng = np.random.default_rng(216)
    degs = list(range(1, 65)) + [100, 257, 1000, 4099]
    c = Case(HW2, O, degs, lambda d: 0.5 + 7.5 * rng.random(d), rng)
    assert c.overflows <= 0.002 * c.lines + 1          # (+1: the row of exactly 10 edges)
    k = c.draw(O, rng, per_row=160, extra_u=())
    n = float(k["draws"])
    print("hw2 uniform: draws %d first window %d (%.4f) second window %d (%.5f) cold %d (%.5f); "
          "wb_hw.h second entry %d (%.5f)" % (k["draws"], k["first"], k["first"] / n, k["second"], k["second"] / n,
                                               k["cold"], k["cold"] / n, k["old_second"], k["old_second"] / n))
    assert k["second"] + k["cold"] < k["old_second"], k
