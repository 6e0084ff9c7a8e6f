"""ops.mask_attention (csrc/mp_mask_attention.h) against a float64 statement of the reference's
AttentionAggregator: the bits of mask_aggregate at zero scores, a selector that only a per-source shift and a
select by the bit pass, real values within the derived bound, same bits, and gradients.

THE BOUND of test_real_values_within_bound, from the contract, per output element (alpha, e of the float64
reference; u32 = 2^-24; u_p = 2^-8 / 2^-11 / 0 the operand rounding of p; mag = sum alpha |z| incl. the self term):
  a numerator p carries the relative error  r = u_p + 2 EXP_REL + 6 u32 max|e|  - its one rounding to the
  operand type, the hardware exp (EXP_REL: the largest relative error of v_exp_f32 on fl(x log2e) against float64
  exp over [-30, 0] as measured on the device, DESIGN 4.34, doubled because that sweep is finite), and the fp32
  roundings of e_c, M and e_c - M in the exponent (2 |e_c| + 2 |M| + |e_c - M| <= 6 max|e| units);
  numerator and denominator each move the quotient by r to first order:                2 r mag
  fp16 p below 2^-14 is subnormal, absolute 2^-25 per term over l >= 1:                2^-25 (sum_N |z_c| + deg |A|)
  fp32 accumulation, self term, division and the root add (the form of DESIGN 4.33):   (4 (deg + 3) + 2) u32 (mag + |root|)
  one rounding to the output dtype:                                                    unit |want|
Largest error / bound measured (MI355X): f32 0.022, bf16 0.707, f16 0.658.
GRADIENTS are those of the fp32 recomputation in torch ops; each element is held to (12 max|e| + 4 (m + dh + 4)) 2^-24
times the sum of the absolute values of its own terms in the float64 reference (derived in test_gradients).
Largest error / bound measured (MI355X): 0.008 - the bound counts every reduction at its worst case."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mask_aggregate_ref import pack, plan

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U32 = 2.0 ** -24
EXP_REL = 1.77e-6
KB = {dt: plan(1 << 20, 128, dt == "f32")[2] for dt in DT}          # the candidate block
FT = 16 * 4                                                           # the column tile: kMaskAttMaxNt = 4
FORMS = ("none", "root", "renorm")
AGG = {"none": "mean", "root": "gcn", "renorm": "gcn_renorm"}
BASE = dict(batch=2, n=33, m=130, hd=(3, 8), density=0.1, fill=None, off=0)
CASES = {
    "base": {},
    **{"m%s" % m: dict(m=m) for m in (1, 63, 65, "KB+1", "2KB+33")},
    **{"n%d" % n: dict(n=n) for n in (1, 17, 129)},
    **{"h%dx%d" % hd: dict(hd=hd) for hd in ((1, 1), (1, 24), (3, 24), (4, 16), (1, FT + 1))},
    "batch1": dict(batch=1), "batch3": dict(batch=3), "off": dict(off=1),
    "zeros": dict(fill=0), "ones": dict(fill=1), "zero-word": dict(fill="gap", m=200),
}
THIN = ("base", "m2KB+33", "n129", "h3x24", "h1x%d" % (FT + 1), "batch3", "off")


def make(case, dt, real=False, seed=0, scores=True):
    """device tensors of a case; stray bits SET beyond m; mask and z are views `off` words / elements off"""
    c = dict(BASE, **case)
    rng = np.random.default_rng(seed)
    m = c["m"] if not isinstance(c["m"], str) else {"KB+1": KB[dt] + 1, "2KB+33": 2 * KB[dt] + 33}[c["m"]]
    batch, n, off, (heads, dh) = c["batch"], c["n"], c["off"], c["hd"]
    d = heads * dh
    bits = rng.random((batch * n, (m + 63) // 64 * 64)) < c["density"]
    if c["fill"] in (0, 1):
        bits[:] = bool(c["fill"])
    elif c["fill"] == "gap":                                          # full rows around one all-zero word
        bits[:] = True
        bits[:, 64:128] = False
    live = torch.as_tensor(bits[:, :m].copy()).view(batch, n, m)
    bits[:, m:] = True
    words = pack(bits).reshape(-1)
    mask = torch.as_tensor(np.concatenate([np.zeros(off, np.int64), words])).cuda()[off:].view(batch * n, -1)
    val = (lambda *s: rng.standard_normal(s)) if real else (lambda *s: rng.integers(-8, 9, s))
    rows = batch * m + 2                                              # (rows past batch * m are never read)
    flat = torch.zeros(rows * d + 8, dtype=DT[dt])
    flat[off:off + rows * d] = torch.as_tensor(val(rows * d), dtype=DT[dt])
    z = flat.cuda()[off:off + rows * d].view(rows, d)
    root = torch.as_tensor(val(batch * n, d), dtype=DT[dt]).cuda()
    score = lambda r: torch.as_tensor(rng.standard_normal((r, heads)) * scores, dtype=torch.float32).cuda()
    return SimpleNamespace(mask=mask, z=z, root=root, s_src=score(batch * n), s_nb=score(rows), s_root=score(batch * n),
                           batch=batch, n=n, m=m, heads=heads, dh=dh, bits=live)


def run(a, form, **kw):
    from euler_amd import ops
    return ops.mask_attention(a.mask, a.z, a.s_src, a.s_nb, a.batch, a.n, a.m, heads=a.heads,
                              root=None if form == "none" else a.root, s_root=a.s_root if form == "renorm" else None, **kw)


def reference(bits, z, s_src, s_nb, root, s_root, slope):
    """float64: bits [B, n, m] bool, z [B, m, H, dh], s_src [B, n, H], s_nb [B, m, H], root [B, n, H, dh] | None,
    s_root [B, n, H] | None -> (out, A, sum alpha |z| incl. the self term, each [B, n, H, dh]; max |e|; alpha [B, n, m (+ 1), H])"""
    m = bits.shape[2]
    leaky = lambda a: torch.where(a < 0, a * slope, a)
    e = leaky(s_src[:, :, None] + s_nb[:, None]).masked_fill(~bits[..., None], -math.inf)
    if s_root is not None:
        e = torch.cat([e, leaky(s_src + s_root)[:, :, None]], 2)
    top = e.amax(2, keepdim=True)
    p = torch.exp(e - torch.where(top.isfinite(), top, torch.zeros_like(top)))
    total = p.sum(2, keepdim=True)
    alpha = p / torch.where(total > 0, total, torch.ones_like(total))
    agg = torch.einsum("bnmh,bmhd->bnhd", alpha[:, :, :m], z)
    mag = torch.einsum("bnmh,bmhd->bnhd", alpha[:, :, :m], z.abs())
    if s_root is not None:
        agg, mag = agg + alpha[:, :, m, :, None] * root, mag + alpha[:, :, m, :, None] * root.abs()
    out = root + agg if root is not None and s_root is None else agg
    return out, agg, mag, float(e.detach()[e.isfinite()].abs().max()) if e.isfinite().any() else 0.0, alpha.detach()


def inputs64(a, form):
    """the stored values of a case as float64 CPU tensors in the reference's shapes"""
    b, n, m, h = a.batch, a.n, a.m, a.heads
    wide = lambda t, r: t.detach()[:b * r].double().cpu().view(b, r, h, -1)
    return (a.bits, wide(a.z, m), wide(a.s_src, n)[..., 0], wide(a.s_nb, m)[..., 0],
            None if form == "none" else wide(a.root, n), wide(a.s_root, n)[..., 0] if form == "renorm" else None)


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("name", sorted(CASES))
def test_zero_scores_are_mask_aggregate(name, dt):
    from euler_amd import ops
    a = make(CASES[name], dt, scores=False)
    for form in FORMS:
        want = ops.mask_aggregate(AGG[form], a.mask, a.z, a.batch, a.n, a.m, root=None if form == "none" else a.root)
        assert torch.equal(run(a, form).view(torch.uint8), want.view(torch.uint8)), (name, dt, form)


@pytest.mark.parametrize("dt", sorted(DT))
def test_selector(dt):
    """per batch row and head h ONE candidate pair scores 0 (even sources neighbour the first of the pair, odd ones the
    second), every other candidate -1e4 - exp(-2000) is 0 - and one candidate that is nobody's neighbour +1e4"""
    a = make({}, dt, real=True, seed=4)
    b, n, m, h, dh = a.batch, a.n, a.m, a.heads, a.dh
    bits = a.bits.clone()
    s_nb = torch.full((b, m, h), -1e4)
    pick = torch.zeros((b, n, h), dtype=torch.int64)
    even = torch.arange(n) % 2 == 0
    for r in range(b):
        bits[r, :, 100 + r] = False
        s_nb[r, 100 + r] = 1e4
        for k in range(h):
            first, second = 7 * r + 11 * k, 7 * r + 11 * k + 3
            s_nb[r, first, k] = s_nb[r, second, k] = 0.0
            bits[r, :, first], bits[r, :, second] = even, ~even
            pick[r, :, k] = torch.where(even, first, second)
    a.mask = torch.as_tensor(pack(bits.view(b * n, m).numpy())).cuda()
    a.s_nb = torch.cat([s_nb.view(b * m, h), torch.zeros(2, h)]).cuda()
    zs = a.z[:b * m].cpu().view(b, m, h, dh)
    want = torch.stack([zs[r, pick[r], torch.arange(h)] for r in range(b)]).reshape(b * n, h * dh)
    assert torch.equal(run(a, "none").cpu(), want)
    assert torch.equal(run(a, "root").float().cpu(), (a.root.float() + want.cuda().float()).to(DT[dt]).float().cpu())
    a.s_root = torch.full_like(a.s_root, 1e4)
    assert torch.equal(run(a, "renorm").cpu(), a.root.cpu())


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("name", THIN)
def test_real_values_within_bound(name, dt):
    a = make(CASES[name], dt, real=True, seed=1)
    u_p = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[dt]
    worst = 0.0
    for form in FORMS:
        x = inputs64(a, form)
        deg = a.bits.sum(2).double()[:, :, None, None]
        absz = torch.einsum("bnm,bmhd->bnhd", a.bits.double(), x[1].abs())
        for slope in (0.2, 1.0):
            want, agg, mag, emax, _ = reference(*x, slope)
            rel = u_p + 2 * EXP_REL + 6 * U32 * emax
            lim = 2 * rel * mag + (4 * (deg + 3) + 2) * U32 * (mag + (x[4].abs() if form == "root" else 0))
            if dt == "f16":
                lim = lim + 2.0 ** -25 * (absz + deg * agg.abs())
            for act in (None, "relu"):
                out = run(a, form, negative_slope=slope, activation=act).double().cpu().view(want.shape)
                goal = torch.relu(want) if act else want
                err, full = (out - goal).abs(), lim + UNIT[DT[dt]] * goal.abs()
                worst = max(worst, float((err / full.clamp_min(1e-300)).max()))
                assert (err <= full).all(), (name, dt, form, slope, act, worst)
    print("mask_attention %s %s: largest error / bound = %.3f" % (name, dt, worst))


@pytest.mark.parametrize("dt", sorted(DT))
def test_same_bits(dt):
    a = make(dict(m=2 * KB[dt] + 33, n=129), dt, real=True, seed=2)
    same = lambda p, q: torch.equal(p.view(torch.uint8), q.view(torch.uint8))
    for form in FORMS:
        first = run(a, form)
        with torch.cuda.stream(torch.cuda.Stream()):
            other = run(a, form)
        torch.cuda.synchronize()
        rows = []
        for r in range(a.batch):
            s, c = slice(r * a.n, (r + 1) * a.n), slice(r * a.m, (r + 1) * a.m)
            one = SimpleNamespace(mask=a.mask[s], z=a.z[c], s_src=a.s_src[s], s_nb=a.s_nb[c], root=a.root[s], s_root=a.s_root[s],
                                  batch=1, n=a.n, m=a.m, heads=a.heads)
            rows.append(run(one, form))
        assert same(first, run(a, form)) and same(first, other) and same(first, torch.cat(rows)), form


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("slope", [0.0, 0.2])
@pytest.mark.parametrize("m", [0, 130])
def test_sources_without_neighbours(m, slope, dt):
    """no bit set (m = 130) and no candidate at all (m = 0): +0, root, and - the self term alone - root, at slope 0 too"""
    a = make(dict(fill=0), dt, real=True, seed=5)
    if m == 0:
        a.m, a.mask = 0, torch.zeros((a.batch * a.n, 0), dtype=torch.int64, device="cuda")
    for form, want in (("none", torch.zeros_like(a.root)), ("root", a.root), ("renorm", a.root)):
        assert torch.equal(run(a, form, negative_slope=slope).view(torch.uint8), want.view(torch.uint8)), form


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hd", [(3, 8), (3, 24)])
def test_gradients(hd, form):
    """all five inputs against float64 autograd of the reference, element by element; source 0 has no neighbour and
    its row of grad reaches neither z, s_nb nor a score"""
    a = make(dict(hd=hd, fill=None), "f32", real=True, seed=3)
    a.bits[0, 0] = False
    a.mask = torch.as_tensor(pack(a.bits.view(a.batch * a.n, a.m).numpy())).cuda()
    grad = torch.randn(a.batch * a.n, hd[0] * hd[1], device="cuda")
    names = ("z", "s_src", "s_nb") + {"none": (), "root": ("root",), "renorm": ("root", "s_root")}[form]
    for k in names:
        setattr(a, k, getattr(a, k).clone().requires_grad_(True))
    run(a, form, activation="relu").backward(grad)
    x = [t if t is None or t.dtype == torch.bool else t.requires_grad_(True) for t in inputs64(a, form)]
    pre, _, mag, emax, alpha = reference(*x, 0.2)
    torch.relu(pre).backward(grad.double().cpu().view(pre.shape))
    # sum |terms| of every gradient element, from the reference: with G = |grad| past the relu, d out / d e_c has the
    # terms alpha_c (G . |z_c| + G . mag), summed over candidates for s_src and over sources for s_nb (|leaky'| <= 1)
    with torch.no_grad():
        big = (grad.double().cpu().view(pre.shape) * (pre > 0)).abs()
        nb, dot = alpha[:, :, :a.m], (big * mag).sum(-1)
        t = nb * (torch.einsum("bnhd,bmhd->bnmh", big, x[1].abs()) + dot[:, :, None])
        t0 = alpha[:, :, a.m] * ((big * x[4].abs()).sum(-1) + dot) if form == "renorm" else 0 * dot
        terms = {"z": torch.einsum("bnmh,bnhd->bmhd", nb, big), "s_src": t.sum(2) + t0, "s_nb": t.sum(1), "s_root": t0,
                 "root": big * alpha[:, :, a.m, :, None] if form == "renorm" else big}
    # every weight carries the exponent's fp32 roundings in numerator and denominator (2 x 6 max|e| units, as in the
    # forward bound) and four chained fp32 reductions of at most K = m + 1 + dh terms add K + 3 units each
    unit = (12 * emax + 4 * (a.m + 1 + a.dh + 3)) * U32
    worst = 0.0
    for k, want in zip(("z", "s_src", "s_nb", "root", "s_root"), x[1:]):
        if k not in names:
            continue
        got = getattr(a, k).grad.double().cpu()
        rows = want.shape[0] * want.shape[1]
        assert torch.isfinite(got).all() and not got[rows:].any(), k
        err = (got[:rows].reshape(want.shape) - want.grad).abs()
        worst = max(worst, float((err / (unit * terms[k]).clamp_min(1e-300)).max()))
        assert (err <= unit * terms[k]).all(), (k, worst)
    print("mask_attention gradients %s %s: largest error / bound = %.3f" % (hd, form, worst))
    only0 = torch.zeros_like(grad)
    only0[0] = grad[0]
    for got in torch.autograd.grad(run(a, form, activation="relu"), [getattr(a, k) for k in names if k != "root"], only0):
        assert not got.any()
