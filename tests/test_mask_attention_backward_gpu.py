"""ops.mask_attention(backward="fused") (csrc/mp_mask_attention_backward.h) against float64 autograd of the reference of
test_mask_attention_gpu.py: exact on powers of two across every block, tile and tail boundary of both kernels, real
values within the derived bound, same bits, and sources without neighbours.

THE BOUND of test_real_values_within_bound.  Every gradient element is a sum of terms alpha (G . |z| + G . mag) (the
`terms` of test_mask_attention_gpu.test_gradients); it is held to unit x that sum, with, per the contract:
  the exponent's fp32 roundings of e_c, M and e_c - M, in numerator and denominator (2 x 6 max|e|):  12 max|e| u32
  four chained fp32 reductions - the sums l, the matrix accumulation over K = m (kernel 1) or n (kernel 2), the dot
  over dh and the 16 column lanes, and D re-entering W - of at most K + 1 + dh terms, K + 3 units each:
                                                                              4 (max(m, n) + 1 + dh + 3) u32
  the hardware exp in numerator and denominator, 2 EXP_REL each as in the forward's bound:          4 EXP_REL
  16 bits: the rounded numerators, in the product and in l, and the rounded G~ operand:              3 u_p
and one unit of the output dtype on |want| for d z and d root.
fp16 below 2^-14 is subnormal, spacing 2^-24: a stored d z or d root element carries the absolute 2^-25 instead, and so do
the operands of d z = sum_i p_ic G~_i - G~'s absolute error times p <= 1 and p's times |G~| <= |g| (den >= 1: the largest
numerator is exactly 1) - which adds 2^-25 sum_{i in N(c)} (1 + |g_i|) to d z, as the forward's bound does for its p.
Largest error / bound measured (MI355X): f32 0.012, bf16 0.643, f16 0.798."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mask_aggregate_ref import pack
from test_mask_attention_gpu import DT, EXP_REL, FORMS, KB, THIN, CASES, U32, UNIT, inputs64, make, reference, run

pytestmark = pytest.mark.gpu

FT = 16 * 2                                                           # the column tile: kMaskAttBwdMaxNt = 2
NAMES = ("z", "s_src", "s_nb", "root", "s_root")
USED = {"none": NAMES[:3], "root": NAMES[:4], "renorm": NAMES}
EDGES = {
    "base": {},
    **{"m%s" % m: dict(m=m) for m in (1, 63, 65, "KB+1", "2KB+33")},
    **{"n%s" % n: dict(n=n) for n in (1, 17, 129, "2KB+33")},         # n is the contraction of kernel 2
    **{"h%dx%d" % hd: dict(hd=hd) for hd in ((1, 1), (3, 24), (1, FT + 1))},
    "batch3": dict(batch=3), "off": dict(off=1),
    "cap": dict(batch=130, n=3, m=65, hd=(8, 1)),                     # 1 040 items > kMaskMaxBlocks in both kernels
}


def remask(a, bits, off=0):
    """a's adjacency replaced by bits [batch * n, m]; stray bits SET beyond m, the words `off` words off"""
    full = np.ones((bits.shape[0], (a.m + 63) // 64 * 64), bool)
    full[:, :a.m] = bits
    a.bits = torch.as_tensor(bits.copy()).view(a.batch, a.n, a.m)
    words = np.concatenate([np.zeros(off, np.int64), pack(full).reshape(-1)])
    a.mask = torch.as_tensor(words).cuda()[off:].view(a.batch * a.n, -1)


def fused(a, form, grad, **kw):
    """-> (out, {name: gradient}) of the fused route on fresh leaves"""
    leaf = SimpleNamespace(**vars(a))
    for k in USED[form]:
        setattr(leaf, k, getattr(a, k).detach().requires_grad_(True))
    out = run(leaf, form, backward="fused", **kw)
    out.backward(grad)
    return out.detach(), {k: getattr(leaf, k).grad for k in USED[form]}


def wanted(a, form, slope):
    """the float64 leaves and the reference's pre-activation output, mag, max|e| and alpha"""
    x = [t if t is None or t.dtype == torch.bool else t.requires_grad_(True) for t in inputs64(a, form)]
    pre, _, mag, emax, alpha = reference(*x, slope)
    return dict(zip(NAMES, x[1:])), pre, mag, emax, alpha


def noise(a, dt, seed):
    """a seeded incoming gradient [batch * n, d] of the output's dtype"""
    g = np.random.default_rng(seed).standard_normal((a.batch * a.n, a.heads * a.dh))
    return torch.as_tensor(g, dtype=DT[dt]).cuda()


def gated(grad, out, act, shape):
    """grad past the relu, the gate taken from the op's own output"""
    g = grad.double().cpu().view(shape)
    return g * (out.double().cpu().view(shape) > 0) if act else g


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("name", sorted(EDGES))
def test_exact_on_powers_of_two(name, dt, form):
    """zero scores, small integers, 0 / 1 / 2 / 4 / 8 softmax terms per source (the self term of renorm counted): every
    alpha is a power of two and every sum exact, so all five gradients EQUAL the reference's rounded once"""
    case = dict(EDGES[name])
    if case.get("n") == "2KB+33":
        case["n"] = 2 * KB[dt] + 33
    a = make(case, dt, scores=False)
    rng = np.random.default_rng(7)
    bits = np.zeros((a.batch * a.n, a.m), bool)
    for r in range(bits.shape[0]):
        own = int(form == "renorm")
        terms = rng.choice([t for t in (0, 1, 2, 4, 8) if 0 <= t - own <= a.m])
        bits[r, rng.choice(a.m, terms - own, replace=False)] = True
    remask(a, bits, case.get("off", 0))
    grad = torch.as_tensor(rng.integers(-8, 9, (a.batch * a.n, a.heads * a.dh)), dtype=DT[dt]).cuda()
    out, got = fused(a, form, grad, activation="relu")
    x, pre, _, _, _ = wanted(a, form, 0.2)
    pre.backward(gated(grad, out, True, pre.shape))
    for k in USED[form]:
        rows = x[k].shape[0] * x[k].shape[1]
        want = x[k].grad.reshape(rows, -1).to(got[k].dtype)
        assert torch.equal(got[k][:rows].cpu(), want) and not got[k][rows:].any(), (name, dt, form, k)
    assert not got["s_src"].any()


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("name", THIN)
def test_real_values_within_bound(name, dt):
    a = make(CASES[name], dt, real=True, seed=1)
    bits = a.bits.view(a.batch * a.n, a.m).numpy().copy()
    lone = [100 + r for r in range(a.batch)]                          # nobody's neighbour, score +1e4
    for r, c in enumerate(lone):
        bits[r * a.n:(r + 1) * a.n, c] = False
        a.s_nb[r * a.m + c] = 1e4
    remask(a, bits, CASES[name].get("off", 0))
    grad = noise(a, dt, 11)
    u_p = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[dt]
    worst, bad = 0.0, []
    for form in FORMS:
        for slope in (0.2, 1.0):
            x, pre, mag, emax, alpha = wanted(a, form, slope)
            unit = (12 * emax + 4 * (max(a.m, a.n) + 1 + a.dh + 3)) * U32 + 4 * EXP_REL + 3 * u_p
            for act in (None, "relu"):
                out, got = fused(a, form, grad, negative_slope=slope, activation=act)
                g = gated(grad, out, act, pre.shape)
                for t in x.values():
                    if t is not None:
                        t.grad = None
                pre.backward(g, retain_graph=True)
                with torch.no_grad():                                 # sum |terms| per element, as in test_gradients
                    big, nb = g.abs(), alpha[:, :, :a.m]
                    dot = (big * mag).sum(-1)
                    t = nb * (torch.einsum("bnhd,bmhd->bnmh", big, x["z"].abs()) + dot[:, :, None])
                    t0 = alpha[:, :, a.m] * ((big * x["root"].abs()).sum(-1) + dot) if form == "renorm" else 0 * dot
                    terms = {"z": torch.einsum("bnmh,bnhd->bmhd", nb, big), "s_src": t.sum(2) + t0, "s_nb": t.sum(1),
                             "s_root": t0, "root": big * alpha[:, :, a.m, :, None] if form == "renorm" else big}
                for k in USED[form]:
                    rows = x[k].shape[0] * x[k].shape[1]
                    have, want = got[k].double().cpu(), x[k].grad
                    assert torch.isfinite(have).all() and not have[rows:].any(), k
                    lim = unit * terms[k] + (UNIT[DT[dt]] * want.abs() if k in ("z", "root") else 0)
                    if dt == "f16" and k in ("z", "root"):
                        lim = lim + 2.0 ** -25
                    if dt == "f16" and k == "z":
                        lim = lim + 2.0 ** -25 * torch.einsum("bnm,bnhd->bmhd", a.bits.double(), 1 + big)
                    err = (have[:rows].reshape(want.shape) - want).abs()
                    ratio = float((err / lim.clamp_min(1e-300)).max())
                    worst = max(worst, ratio)
                    bad += [(form, slope, act, k, ratio)] * (ratio > 1.0)
                for r, c in enumerate(lone):
                    assert not got["z"][r * a.m + c].any() and not got["s_nb"][r * a.m + c].any()
    print("mask_attention backward %s %s: largest error / bound = %.3f" % (name, dt, worst))
    assert not bad, (name, dt, bad)


@pytest.mark.parametrize("dt", sorted(DT))
def test_same_bits(dt):
    a = make(dict(m=2 * KB[dt] + 33, n=129), dt, real=True, seed=2)
    grad = noise(a, dt, 11)
    same = lambda p, q: torch.equal(p.view(torch.uint8), q.view(torch.uint8))
    for form in FORMS:
        first = fused(a, form, grad, activation="relu")[1]
        with torch.cuda.stream(torch.cuda.Stream()):
            other = fused(a, form, grad, activation="relu")[1]
        torch.cuda.synchronize()
        again, rows = fused(a, form, grad, activation="relu")[1], []
        for r in range(a.batch):
            s, c = slice(r * a.n, (r + 1) * a.n), slice(r * a.m, (r + 1) * a.m)
            one = SimpleNamespace(mask=a.mask[s], z=a.z[c], s_src=a.s_src[s], s_nb=a.s_nb[c], root=a.root[s], s_root=a.s_root[s],
                                  batch=1, n=a.n, m=a.m, heads=a.heads)
            rows.append(fused(one, form, grad[s], activation="relu")[1])
        for k in USED[form]:
            split = torch.cat([r[k] for r in rows])
            assert same(first[k], again[k]) and same(first[k], other[k]) and same(first[k][:len(split)], split), (form, k)


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("slope", [0.0, 0.2])
@pytest.mark.parametrize("m", [0, 130])
def test_sources_without_neighbours(m, slope, dt):
    """no bit set (m = 130) and no candidate at all (m = 0): every gradient +0 but d root = grad, in both root forms; and
    a grad on a neighbourless source's row alone reaches nothing else"""
    a = make(dict(fill=0), dt, real=True, seed=5)
    if m == 0:
        a.m, a.mask = 0, torch.zeros((a.batch * a.n, 0), dtype=torch.int64, device="cuda")
    grad = noise(a, dt, 11)
    for form in FORMS:
        got = fused(a, form, grad, negative_slope=slope)[1]
        assert all(not got[k].any() for k in USED[form] if k != "root"), form
        assert form == "none" or torch.equal(got["root"].view(torch.uint8), grad.view(torch.uint8)), form
    if m:
        b = make({}, dt, real=True, seed=6)
        bits = b.bits.view(b.batch * b.n, b.m).numpy().copy()
        bits[0] = False
        remask(b, bits)
        only0 = torch.zeros_like(grad)
        only0[0] = grad[0]
        for form in FORMS:
            got = fused(b, form, only0, negative_slope=slope)[1]
            assert all(not got[k].any() for k in USED[form] if k != "root"), form
