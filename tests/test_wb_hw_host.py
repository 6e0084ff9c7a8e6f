"""The header + window lines of euler_amd/csrc/wb_hw.h - what hop 2 of the plain-graph fanout
step draws through - compiled for the HOST by tests/csrc/hw_check.hip and compared with the
oracle's RandomSelect: build, then draw, then (index, weight).  CPU only; the kernels' lane
mapping is covered by tests/test_fanout_hw_gpu.py.  Skipped when hipcc is absent."""
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
def HW():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libhw_check.so")
    src = os.path.join(HERE, "csrc", "hw_check.hip")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", f)
                    for f in ("wb_hw.h", "wb_index.h", "device_fns.h", "common.h", "philox.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(
            [hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
             "-ffp-contract=off", "-I" + os.path.join(ROOT, "euler_amd", "csrc"),
             "-I" + os.path.join(ROOT, "include"), src, "-o", so])
    L = C.CDLL(so)
    L.hw_build.restype = C.c_void_p
    L.hw_build.argtypes = [C.c_int64, i64p, f32p, u64p]
    L.hw_destroy.argtypes = [C.c_void_p]
    L.hw_lines.restype = C.c_int64
    L.hw_lines.argtypes = [C.c_void_p]
    L.hw_overflows.restype = C.c_int64
    L.hw_overflows.argtypes = [C.c_void_p]
    L.hw_line.argtypes = [C.c_void_p, C.c_int64, u32p]
    L.hw_sample.argtypes = [C.c_void_p, i64p, f64p, C.c_int64, u64p, f32p, i32p]
    return L


def _buckets(d):
    return 0 if d == 0 else 1 if d <= 10 else (d + 3) // 4


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
        self.h = L.hw_build(n, _p(self.row_ptr, i64p), _p(self.pw, f32p), _p(self.nbr, u64p))
        self.lines = L.hw_lines(self.h)
        self.overflows = L.hw_overflows(self.h)

    def __del__(self):
        self.L.hw_destroy(self.h)

    def line(self, i):
        out = np.zeros(32, np.uint32)
        self.L.hw_line(self.h, i, _p(out, u32p))
        return out

    def check_build(self):
        """every line: nine consecutive edges of its row behind an exact `base`, +inf / id 0 past
        the row's end, the window of entry i = {sum before, id, sum}, quantised offsets
        non-decreasing with 255 for padding, and a start that reaches into the bucket"""
        assert self.lines == sum(_buckets(d) for d in self.degs)
        at = 0
        for r, d in enumerate(self.degs):
            b = int(self.row_ptr[r])
            sw = self.pw[b:b + d]
            for j in range(_buckets(d)):
                ln = self.line(at)
                at += 1
                s = int(ln[31]) - b
                assert 0 <= s < d and (j > 0 or s == 0)
                base = ln[3:4].view(np.float32)[0]
                assert base == (sw[s - 1] if s else np.float32(0))
                q = np.concatenate([ln[1:2].view(np.uint8), ln[2:3].view(np.uint8)])
                for i in range(9):
                    win = ln[3 + 3 * i:7 + 3 * i]
                    before, sm = win[0:1].view(np.float32)[0], win[3:4].view(np.float32)[0]
                    ident = int(win[1]) | (int(win[2]) << 32)
                    if s + i < d:
                        assert sm == sw[s + i] and ident == int(self.nbr[b + s + i])
                        assert before == (sw[s + i - 1] if s + i else np.float32(0))
                        if i < 8:
                            assert q[i] <= 254 and (i == 0 or q[i] >= q[i - 1])
                    else:
                        assert np.isposinf(sm) and ident == 0
                        if i < 8:
                            assert q[i] == 255
                with np.errstate(all="ignore"):
                    scale = np.float32(_buckets(d)) / sw[-1] if d else np.float32(0)
                if d > 10 and j > 0 and np.isfinite(scale) and scale > 0:
                    # the first edge whose sum exceeds the bucket's lower bound, or an earlier one
                    # (the builder's safety margin); a total without a finite scale starts at 0
                    lower = np.float64(j) / np.float64(scale)
                    first = int(np.searchsorted(sw.astype(np.float64), lower, side="right"))
                    assert s <= min(first, d - 1) and (s == d - 1 or np.float64(sw[s]) > lower * (1 - 2e-6))

    def draw(self, O, rng, per_row=64, extra_u=EDGE_U):
        """(draws, draws the guessed entry answered, draws the entry before it answered, cold draws) after checking every hot draw
        against the oracle; a cold draw is the caller's RandomSelect by definition"""
        n = len(self.degs)
        rows = np.repeat(np.arange(n, dtype=np.int64), per_row + len(extra_u))
        us = np.concatenate([np.concatenate([rng.random(per_row), np.asarray(extra_u, np.float64)])
                             for _ in range(n)])
        ids = np.zeros(len(rows), np.uint64)
        w = np.zeros(len(rows), np.float32)
        win = np.zeros(len(rows), np.int32)
        self.L.hw_sample(self.h, _p(rows, i64p), _p(us, f64p), len(rows), _p(ids, u64p), _p(w, f32p),
                         _p(win, i32p))
        total = one = two = cold = 0
        for i in range(len(rows)):
            r = int(rows[i])
            d = self.degs[r]
            if d == 0:
                assert win[i] == -2
                continue
            total += 1
            b = int(self.row_ptr[r])
            sw = self.pw[b:b + d]
            if win[i] <= 0:
                cold += 1
                # a draw that rounds up to the row's total never sees a line
                rounds_up = not (np.float64(sw[-1]) > np.float64(us[i]) * np.float64(sw[-1]))
                assert (win[i] == 0) == rounds_up, (r, d, us[i])
                continue
            want = O.random_select(sw, 0, d - 1, float(us[i]))
            assert ids[i] == self.nbr[b + want], (r, d, us[i], want, int(win[i]))
            ww = np.float32(sw[want]) - (np.float32(sw[want - 1]) if want else np.float32(0))
            assert w[i:i + 1].view(np.uint32)[0] == np.asarray([ww], np.float32).view(np.uint32)[0]
            one += int(win[i] == 1)
            two += int(win[i] == 2)
        return total, one, two, cold


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


def test_hw_lines_vs_random_select(HW, O):
    """Every weight family of tests/test_host_check.py's weight-bucket test, rows of 1, 9, 10, 11
    and 37 edges among them: the lines are built as documented, and every draw either returns
    exactly RandomSelect's (id, weight) or reports cold."""
    rng = np.random.default_rng(12)
    for name, fn in _families(rng):
        small = name in ("all zero", "denormal", "huge")
        c = Case(HW, O, [1, 5, 10, 30, 200] if small else DEGS, fn, rng)
        c.check_build()
        total, one, two, cold = c.draw(O, rng, per_row=8 if small else 64)
        assert total == one + two + cold, name
        if name == "all zero":
            assert cold == total        # total 0: every draw rounds up to it
        if name in ("uniform", "equal", "ones", "ramp up"):
            assert one > 0.8 * total, (name, total, one, two, cold)


def test_hw_draws_that_round_up_to_the_total_are_cold(HW, O):
    """r = u * total that is not below the total (u = 1, or any u on a row whose total is 0) never
    looks at a line: cold, as in WbSampleHot.  The largest u a draw can have, 1 - 2^-53, stays
    below the total in fp64 and must be served exactly (Case.draw checks which of the two applies)."""
    rng = np.random.default_rng(13)
    c = Case(HW, O, [1, 9, 10, 11, 37], lambda d: 0.5 + 7.5 * rng.random(d), rng)
    total, one, two, cold = c.draw(O, rng, per_row=0, extra_u=(1.0,))
    assert total == 5 and cold == 5
    total, one, two, cold = c.draw(O, rng, per_row=0, extra_u=(1.0 - 2.0 ** -53,))
    assert total == 5 and one + two >= 4           # (the row of 10 edges: its last edge is not in the line)
    z = Case(HW, O, [1, 9, 10, 11, 37], lambda d: np.zeros(d), rng)
    total, one, two, cold = z.draw(O, rng, per_row=4, extra_u=(0.0,))
    assert cold == total == 25


def test_hw_last_bucket_overflow_goes_cold(HW, O):
    """A row of 37 edges whose last bucket holds more than nine edges' intervals (dust behind
    giants): the builder counts the overflow and the draws beyond the ninth entry are cold, the
    others exact.  A row of exactly 10 edges overflows its single line the same way."""
    rng = np.random.default_rng(14)

    def tail(d):
        w = np.full(d, 8.0)
        w[-14:] = 0.05
        return w
    c = Case(HW, O, [37], tail, rng)
    c.check_build()
    assert c.overflows >= 1
    # draws over the dusty tail: u in the last 14 * 0.05 of the total
    tot = float(c.pw[-1])
    us = tuple(1.0 - (k + 0.5) * 0.05 / tot for k in range(14))
    total, one, two, cold = c.draw(O, rng, per_row=256, extra_u=us)
    assert cold >= 3 and one + two > 0.9 * total
    c10 = Case(HW, O, [10], lambda d: np.ones(d), rng)
    assert c10.overflows == 1
    total, one, two, cold = c10.draw(O, rng, per_row=400, extra_u=(0.95, 0.999))
    assert cold >= 2 and 0.05 * total < cold < 0.16 * total


def test_hw_heavy_tail_most_guesses_miss(HW, O):
    """One giant among dust in every line's range: the dust shares a quantum, so the header's
    guess is usually wrong - and the keys still decide: every draw is exact or cold."""
    rng = np.random.default_rng(15)

    def w(d):
        x = np.full(d, 1e-4)
        x[::7] = 1e3
        x[1::7] = 3e-4
        return x
    c = Case(HW, O, [37, 200, 1000], w, rng)
    c.check_build()
    # aim at the dust: u just behind a giant's running sum
    us = []
    for r in range(3):
        b = int(c.row_ptr[r])
        sw = c.pw[b:b + c.degs[r]].astype(np.float64)
        us.append([(sw[k] + 1e-4 * (1 + (k % 5))) / sw[-1] for k in range(0, c.degs[r] - 8, 7)][:5])
    total, one, two, cold = c.draw(O, rng, per_row=64, extra_u=tuple(np.clip(us[1], 0, 1 - 1e-9)))
    assert two + cold > 0, (total, one, two, cold)


def test_hw_cold_share_on_uniform_weights(HW, O):
    """i.i.d. uniform [0.5, 8) weights - the metric graph's: fewer than 0.5 % of the draws are
    cold (the cap that keeps an always-cold build from passing), over rows of every degree from
    1 to 64 and a few large ones, equally many draws per row; and the guess is right for most."""
    rng = np.random.default_rng(16)
    degs = list(range(1, 65)) + [100, 257, 1000, 4099]
    c = Case(HW, O, degs, lambda d: 0.5 + 7.5 * rng.random(d), rng)
    assert c.overflows <= 0.002 * c.lines + 1          # (+1: the row of exactly 10 edges)
    total, one, two, cold = c.draw(O, rng, per_row=160, extra_u=())
    print("hw uniform: draws %d guessed entry %d entry before %d cold %d" % (total, one, two, cold))
    assert cold < 0.005 * total, (total, cold)
    assert two < 0.15 * total, (total, two)
