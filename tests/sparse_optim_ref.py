"""The fused sparse-row optimiser steps (euler_amd/csrc/sparse_optim.h) restated in numpy: `step`
is the contract in fp32, one rounding per fl(); every comparison with it is bit equality.
`step64` is its float64 twin: the same formulas in float64, with a RUNNING ERROR BOUND carried
forward per element.

Storage, the 16-bit helpers, `same` and `sensitive_values` are those of embed_store_ref.py.

The bound of step64.  Write x^ for a value the fp32 code computes, x for the twin's value of the
same quantity and bx >= |x^ - x|.  Inputs (table, state of the first step, gradient rows, scalars)
are the same numbers on both sides: b = 0.  One fp32 operation computes z^ = fl(w), w = x^ op y^
taken exactly, and a correctly rounded operation has |fl(w) - w| <= u |w|, u = 2^-24.  So

    bz = P + u (|z| + P),     P >= |w - z| the propagated part:

    sum, difference   P = bx + by
    product           P = |x| by + |y| bx + bx by
    quotient          P = (bx + |z| by) / (|y| - by)               (by < |y|, asserted)
    square root       P = bx / (sqrt(x) + sqrt(max(x - bx, 0)))    (sqrt(bx) where that is 0 / 0)

The first-order terms are u |z|, bx + by, |x| by + |y| bx, (bx + |z| by) / |y| and
bx / (2 sqrt(x)); what the lines above add to them (u P, bx by, the by in the denominator, the
bx under the root) is the exact second-order remainder, carried instead of estimated, so the bound
also holds where a sum of gradients cancels and its relative error is large.  No result of the
tests is subnormal (u |w| bounds the rounding of normal results only).  The state a step returns
carries its bound into the next step.  The only constants are u and F = 1 + 2^-20, which every
bound is multiplied by once at the end: it covers the roundings of the twin's own float64
operations, each 2^-29 of an fp32 rounding.  With u = 2^-53 the same rules bound the distance of
the twin itself from the exact value.

`free=True` is the form used against ANOTHER implementation of the same formulas (torch's
optimisers in float64, u = 2^-53), whose sums may associate differently:
  - the rounding of a sum or difference is bounded by u (|x| + |y| + P) instead of u (|z| + P):
    |z| <= |x| + |y|, and the right side does not shrink when the terms cancel;
  - each of the n - 1 additions of a row's gradient chain is bounded by u (A + P), A = sum |x_i|
    over the row's n occurrences: whatever the order or the tree of the additions, every partial
    sum is a sum over a subset of the x_i and so at most A in magnitude.
Call B the free bound of a row's element.  The twin is within B of the exact value.

How far another implementation is from the twin, in units of B (`torch_factor`):
  - adam, adagrad: torch coalesces the gradient (a sum of the n occurrences in some order) and
    then performs the operations of the contract, one rounding each, up to the order of the
    operands of a sum; where it fuses p + alpha * x into one rounding it rounds less, never more.
    So it is within B of the exact value as well, and within 2 B of the twin.
  - sgd: torch may fold an uncoalesced gradient into the row occurrence by occurrence,
    p_k = fl(p_(k-1) - fl(lr x_k)), k = 1..n.  The n products round by u lr |x_k| each, in sum
    u lr A; every p_k is at most |p| + lr A, so the n subtractions round by at most
    n u (|p| + lr A).  B holds u (|p| + lr |g|) for the twin's one subtraction and, for n >= 2,
    (n - 1) u lr A for the chain, so (n + 1) B >= (n + 1) u |p| + (n + 1)(n - 1) u lr A covers
    both sums (for n = 1 the fold IS the contract's step, and B alone covers it).  The bound that
    comes in from the steps before passes through p - lr g with factor 1, so by induction over
    the steps torch is within (N + 1) B of the exact value, N the most occurrences THAT ROW had
    in any step so far, and within (N + 2) B of the twin.  A row that coalesces first is within
    B, which is less.
In both cases the second-order terms (the factors above squared times u^2) are far below F - 1."""
from collections import OrderedDict
import math

import numpy as np

import embed_store_ref as es

KINDS = ("sgd", "momentum", "adagrad", "adam")
N_STATE = {"sgd": 0, "momentum": 1, "adagrad": 1, "adam": 2}
U = es.U                                          # unit roundoff of fp32
U64 = 2.0 ** -53
F = 1 + 2.0 ** -20                                # the twin's own float64 roundings


def scalars(kind, lr, momentum=0.0, eps=None, betas=(0.9, 0.999), step=1, fp32=True):
    """the scalars of a call, computed in double; fp32: each rounded once to fp32 (held as a
    Python float), as the host passes them to the kernel"""
    if eps is None:
        eps = {"adagrad": 1e-10, "adam": 1e-8}.get(kind, 0.0)
    b1, b2 = betas
    s = {"lr": float(lr), "mu": float(momentum), "eps": float(eps), "om1": 1 - b1, "om2": 1 - b2,
         "step_size": lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)}
    if fp32:
        s = {k: float(np.float32(v)) for k, v in s.items()}
    return s


def occurrences(ids, rows, m, row_index=None, count=None, reverse=False):
    """distinct live id -> the source rows of its occurrences in increasing (reverse: decreasing)
    position; ids and row_index entries that name no row are left out"""
    occ = OrderedDict()
    order = range(len(ids) - 1, -1, -1) if reverse else range(len(ids))
    for p in order:
        i = int(ids[p])
        s = es.source_row(p, m, row_index, count)
        if es.in_range(i, rows) and s is not None:
            occ.setdefault(i, []).append(s)
    return occ


def step(kind, table, dt, state, ids, grad, gdt, sc, row_index=None, count=None, reverse=False):
    """one step in fp32 -> (the table afterwards, the list of state arrays afterwards); nothing
    passed in is changed.  sc: scalars(..., fp32=True)"""
    es._check(ids, grad, row_index, count)
    assert len(state) == N_STATE[kind]
    c = {k: np.float32(v) for k, v in sc.items()}
    out = np.array(table, copy=True)
    st = [np.array(s, dtype=np.float32, copy=True) for s in state]
    for r, src in occurrences(ids, out.shape[0], grad.shape[0], row_index, count, reverse).items():
        g = es.widen(grad[src[0]], gdt).copy()
        for s in src[1:]:
            g = (g + es.widen(grad[s], gdt)).astype(np.float32)
        p = es.widen(out[r], dt)
        if kind == "sgd":
            p = p - c["lr"] * g
        elif kind == "momentum":
            st[0][r] = c["mu"] * st[0][r] + g
            p = p - c["lr"] * st[0][r]
        elif kind == "adagrad":
            st[0][r] = st[0][r] + g * g
            p = p - c["lr"] * (g / (np.sqrt(st[0][r]) + c["eps"]))
        else:
            st[0][r] = st[0][r] + (g - st[0][r]) * c["om1"]
            st[1][r] = st[1][r] + (g * g - st[1][r]) * c["om2"]
            p = p - c["step_size"] * (st[0][r] / (np.sqrt(st[1][r]) + c["eps"]))
        assert p.dtype == np.float32 and all(s.dtype == np.float32 for s in st)
        out[r] = es.narrow(p, dt)
    return out, st


# ---- the float64 twin ----------------------------------------------------------------------------
class _Ops(object):
    """(value, bound) pairs under the rules of the module's docstring"""

    def __init__(self, u, free):
        self.u, self.free = u, free

    def _round(self, z, prop, mag=None):
        return z, prop + self.u * ((np.abs(z) if mag is None else mag) + prop)

    def add(self, a, b, sign=1.0, mag=None):
        """mag: a bound of |z| given by the caller (free form only)"""
        (x, bx), (y, by) = a, b
        if self.free and mag is None:
            mag = np.abs(x) + np.abs(y)
        return self._round(x + sign * y, bx + by, mag if self.free else None)

    def sub(self, a, b):
        return self.add(a, b, -1.0)

    def mul(self, a, b):
        (x, bx), (y, by) = a, b
        return self._round(x * y, np.abs(x) * by + np.abs(y) * bx + bx * by)

    def div(self, a, b):
        (x, bx), (y, by) = a, b
        assert np.all(by < np.abs(y)), "the divisor is not bounded away from 0"
        z = x / y
        return self._round(z, (bx + np.abs(z) * by) / (np.abs(y) - by))

    def sqrt(self, a):
        x, bx = a
        z = np.sqrt(x)
        den = z + np.sqrt(np.maximum(x - bx, 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            prop = np.where(den > 0, bx / np.where(den > 0, den, 1), np.sqrt(bx))
        return self._round(z, prop)


def step64(kind, table, state, ids, grad, sc, u=U, row_index=None, count=None, bounds=None, free=False):
    """the twin: table / state / grad as float64 (or anything exactly convertible), sc a dict of
    floats -> (table', [state']), (bound of table', [bounds of state']); the bounds already carry
    the factor F.  bounds: what a previous step64 returned as its second value (None: the inputs
    are exact)"""
    assert len(state) == N_STATE[kind]
    o = _Ops(u, free)
    out = np.array(table, dtype=np.float64, copy=True)
    st = [np.array(s, dtype=np.float64, copy=True) for s in state]
    grad = np.asarray(grad, np.float64)
    ob = np.zeros_like(out) if bounds is None else bounds[0] / F
    sb = [np.zeros_like(out) for _ in st] if bounds is None else [b / F for b in bounds[1]]
    zero = np.zeros(out.shape[1])
    k = lambda name: (np.full(out.shape[1], sc[name]), zero)                  # noqa: E731
    for r, src in occurrences(ids, out.shape[0], grad.shape[0], row_index, count).items():
        g = (grad[src[0]].copy(), zero)
        total = np.abs(grad[src]).sum(0)                                      # A of the free form
        for s in src[1:]:
            g = o.add(g, (grad[s], zero), mag=total)
        p = (out[r], ob[r])
        if kind == "sgd":
            p = o.sub(p, o.mul(k("lr"), g))
        elif kind == "momentum":
            a = o.add(o.mul(k("mu"), (st[0][r], sb[0][r])), g)
            p = o.sub(p, o.mul(k("lr"), a))
            st[0][r], sb[0][r] = a
        elif kind == "adagrad":
            s = o.add((st[0][r], sb[0][r]), o.mul(g, g))
            p = o.sub(p, o.mul(k("lr"), o.div(g, o.add(o.sqrt(s), k("eps")))))
            st[0][r], sb[0][r] = s
        else:
            m0, v0 = (st[0][r], sb[0][r]), (st[1][r], sb[1][r])
            m = o.add(m0, o.mul(o.sub(g, m0), k("om1")))
            v = o.add(v0, o.mul(o.sub(o.mul(g, g), v0), k("om2")))
            p = o.sub(p, o.mul(k("step_size"), o.div(m, o.add(o.sqrt(v), k("eps")))))
            st[0][r], sb[0][r] = m
            st[1][r], sb[1][r] = v
        out[r], ob[r] = p
    return (out, st), (ob * F, [b * F for b in sb])


def rotation(n):
    """case n of the bit tests' walk over E x rows x kind (kind n % 4; k = n // 4 counts the
    (E, rows) pairs) -> (index into es.PATTERNS, whether ids that name no row are mixed in).  The
    pattern is k mod 6; the switch flips with k and once more after every six, so that each
    pattern meets both settings within 18 pairs"""
    k = n // 4
    return k % len(es.PATTERNS), bool((k + k // len(es.PATTERNS)) % 2)


def torch_factor(kind, most):
    """[rows]: how many free bounds the torch optimiser of a kind may be from the twin (the
    module's docstring); most: int [rows], the most occurrences each row had in any step so far"""
    return most + 2 if kind == "sgd" else np.full(len(most), 2)


def occurrence_counts(ids, rows, m, row_index=None, count=None):
    """int [rows]: how many live occurrences name each row"""
    n = np.zeros(rows, np.int64)
    for r, src in occurrences(ids, rows, m, row_index, count).items():
        n[r] = len(src)
    return n
