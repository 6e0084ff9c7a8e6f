"""ops.aggregate_dense(backward="fused") (csrc/mp_dense_backward.h) against float64 autograd of
aggregate_dense_backward_ref.composed64: exact on small integers, within a derived bound on real values, the forward's
mask, same bits, partial needs, and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from aggregate_dense_backward_ref import composed64

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
U = 2.0 ** -24
HUB = [0, 1, 300, 0, 0, 1, 5, 16, 17, 0, 33, 2, 0]
NAMES = ("table", "w", "b", "root", "ws")

BASE = dict(dt="bf16", op="add", act="relu", combine="add", d=64, ds=64, f=64, fs=None, count=4, size=65, gather="int32",
            lens=None, off=0, grad="f32", scale=None, bias="f32")
# one-axis sweeps around BASE.  Slabs of the weight kernel: 1024 destinations; grid caps: 512 workgroups x 64 destinations,
# 512 jobs of (slab, 64 k, 64 f) - 171 slabs x 3 f tiles at the last case; d tiles of kernel 2: 16 NT columns, NT by d.
EXACT = {
    "base": {}, "f32": dict(dt="f32"), "f16": dict(dt="f16"), "none": dict(act="none"), "none-same": dict(act="none", grad="same"),
    "mean": dict(op="mean"), "mean-f32-8": dict(op="mean", dt="f32", count=8), "concat": dict(combine="concat", fs=40),
    "fold": dict(combine="fold"), "fold-scale": dict(combine="fold", scale=2.0), "fold-mean": dict(combine="fold", op="mean", count=3),
    "no-root": dict(combine=None), "no-bias": dict(bias=None), "bias-same": dict(bias="same"), "grad-same": dict(grad="same"),
    **{"d%d" % d: dict(d=d) for d in (1, 7, 8, 31, 32, 33, 128, 129)},
    **{"ds%d" % d: dict(ds=d) for d in (1, 7, 8, 31, 32, 33, 128, 129)},
    **{"F%d" % f: dict(f=f) for f in (1, 15, 16, 17, 130)},
    **{"size%d" % s: dict(size=s) for s in (1, 15, 16, 17, 257, 1024, 1025)},
    "seg": dict(lens=HUB), "seg-f32-fold": dict(lens=HUB, dt="f32", combine="fold"), "seg-none": dict(lens=HUB, gather=None),
    "gather-none": dict(gather=None), "gather-int64": dict(gather="int64"), "gather-int32-bad": dict(gather="int32-bad"),
    "gather-int64-bad-mean": dict(gather="int64-bad", op="mean"), "off4": dict(off=2), "off4-f32": dict(dt="f32", off=1),
    "d256-F512-f32": dict(dt="f32", d=256, ds=256, f=512, size=17), "d256-F512": dict(d=256, ds=256, f=512, size=17),
    "d-tile-f32-F512-d33": dict(dt="f32", d=33, ds=33, f=512, size=17),
    "grid-caps": dict(d=8, ds=8, f=130, size=170 * 1024 + 1),
}


def make(case, real=False, seed=0):
    """-> (c, float64 CPU tensors of the stored values by name, gi, seg, g_out, device tensors by name)"""
    c = dict(BASE, **case)
    rng = np.random.default_rng(seed)
    d, f, dt, comb = c["d"], c["f"], DT[c["dt"]], c["combine"]
    ds, fs = (d, 1) if comb == "fold" else (c["ds"], c["fs"] or f)
    seg = np.arange(c["size"] + 1) * c["count"] if c["lens"] is None else np.concatenate([[0], np.cumsum(c["lens"])])
    size, e = len(seg) - 1, int(seg[-1])
    rows = max(e, 1) if c["gather"] is None else 97
    cols = fs + f if comb == "concat" else f
    if real:
        sigma = np.sqrt(c["count"]) if c["op"] == "add" else 1 / np.sqrt(c["count"])     # of a pre-activation without its bias
        v = dict(table=rng.standard_normal((rows, d)), b=3 * sigma * np.where(np.arange(f) % 2, 1.0, -1.0),
                 root=rng.standard_normal((size, ds)), w=rng.standard_normal((d, f)) / np.sqrt(d),
                 ws=rng.standard_normal((ds, fs)) / np.sqrt(ds))
        g_out = rng.standard_normal((size, cols))
    else:
        def sparse(k, n, hits):                          # about `hits` entries of -2 .. 2 per column
            a, at = np.zeros(k * n, dtype=np.int8), rng.integers(0, k * n, int(min(1.0, hits / k) * k * n))
            a[at] = rng.integers(-2, 3, len(at))
            return a.reshape(k, n)
        v = dict(table=rng.integers(-2, 3, (rows, d)), b=rng.integers(-2, 3, f), root=rng.integers(-2, 3, (size, ds)),
                 w=sparse(d, f, 6.0), ws=sparse(ds, fs, 6.0))
        g_out = sparse(size, cols, 6.0)                  # a few terms per column, so that every sum over r stays small
    flat = torch.zeros(rows * d + 8, dtype=dt)
    flat[c["off"]:c["off"] + rows * d] = torch.as_tensor(v["table"].reshape(-1), dtype=dt)
    dev = {k: torch.as_tensor(v[k], dtype=torch.float32 if k == "b" and c["bias"] == "f32" else dt).cuda() for k in NAMES}
    dev["table"] = flat.cuda()[c["off"]:c["off"] + rows * d].view(rows, d)
    for k, live in (("b", c["bias"] is not None), ("root", comb is not None), ("ws", comb in ("add", "concat"))):
        if not live:
            dev[k] = None
    gi = None
    if c["gather"] is not None:
        gi = rng.integers(0, rows, e).astype(np.int64 if c["gather"].startswith("int64") else np.int32)
        if c["gather"].endswith("bad"):
            gi[::3] = np.resize([-1, rows] + ([2 ** 40, 2 ** 32 + 3] if gi.dtype == np.int64 else []), len(gi[::3]))
    cpu = {k: None if dev[k] is None else dev[k].detach().double().cpu() for k in NAMES}
    g_t = torch.as_tensor(g_out, dtype=torch.float32 if c["grad"] == "f32" else dt)
    return c, cpu, gi, torch.as_tensor(seg), g_t, dev


def run(c, dev, gi, seg, g_t, needs=NAMES, as_seg=None, backward="fused"):
    """forward + backward on the device -> (out, the gradients by name)"""
    from euler_amd import ops
    leaf = {k: None if t is None else t.detach().requires_grad_(k in needs) for k, t in dev.items()}
    form = dict(seg_ptr=seg.cuda()) if (c["lens"] is not None if as_seg is None else as_seg) else dict(count=c["count"])
    out = ops.aggregate_dense(c["op"], leaf["table"], leaf["w"], None if gi is None else torch.as_tensor(gi).cuda(), len(seg) - 1,
                              root=leaf["root"], root_weight=leaf["ws"], combine=c["combine"] or "add", root_scale=c["scale"],
                              bias=leaf["b"], activation=c["act"], out_dtype=g_t.dtype, backward=backward, **form)
    out.backward(g_t.cuda())
    return out, {k: t.grad for k, t in leaf.items() if t is not None and k in needs}


def reference(c, cpu, gi, seg, g64, masks=None, a_pad=0.0):
    """float64 autograd -> (the gradients by name, the pre-activations)"""
    leaf = {k: None if t is None else t.clone().requires_grad_(True) for k, t in cpu.items()}
    g = torch.arange(int(seg[-1])) if gi is None else torch.as_tensor(gi.astype(np.int64))
    out, zs = composed64(c["op"], c["combine"], c["scale"], c["act"], seg, leaf["table"], leaf["w"], leaf["b"], leaf["root"],
                         leaf["ws"], g, masks=masks, a_pad=a_pad)
    out.backward(g64)
    return {k: t.grad for k, t in leaf.items() if t is not None}, [z.detach() for z in zs]


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_integers(name):
    """every gradient is an integer or dyadic value its dtype holds (asserted on the reference first): compared with =="""
    c, cpu, gi, seg, g_t, dev = make(EXACT[name])
    want, _ = reference(c, cpu, gi, seg, g_t.double())
    for k, t in want.items():
        assert torch.equal(t.to(dev[k].dtype).double(), t), (name, k, "the reference does not fit the dtype")
    _, got = run(c, dev, gi, seg, g_t)
    for k, t in want.items():
        wrong = torch.nonzero(got[k].double().cpu() != t)
        assert got[k].dtype == dev[k].dtype and len(wrong) == 0, (name, k, len(wrong), wrong[:5])


REAL = [dict(dt=dt, op=op, combine=comb, size=37, d=24, ds=12, f=20, fs=9 if comb == "concat" else None, scale=sc)
        for dt in sorted(DT) for op, comb, sc in (("mean", "add", None), ("add", "concat", None), ("mean", "fold", 1.5), ("add", None, None))]


@pytest.mark.parametrize("case", REAL, ids=lambda c: "-".join(str(c[k]) for k in ("dt", "op", "combine")))
def test_real_values_within_bound(case):
    """Against float64 autograd on the stored values, grad in fp32.  No pre-activation lies within the forward's bound of 0
    (checked first; neighbour path: test_real_values_within_bound of the forward's test; self path: the root is an exact
    operand, only the accumulation term), so the masks agree.  Bound of a gradient element: M, the same graph on absolute
    values with the masks held, times 4 (terms + 2) 2^-24 - terms = e + d + ds + F bounds the rounded fp32 operations behind
    it (fold, division, accumulations, the slab sums, the grouped add), x4 because an MFMA's rounding is undocumented - plus
    three narrowings of unit roundoff u of the table's dtype on the path: A, the dZ operand, the stored gradient:
    (1 + u)^3 - 1.  fp16: a narrowing also errs by up to 2^-25 absolutely below the normal range, u (|x| + 2^-14) in all:
    M is taken with 2^-14 added to |A| and to |grad|, and 2^-25 is added for the stored gradient."""
    c, cpu, gi, seg, g_t, dev = make(case, real=True, seed=5)
    want, zs = reference(c, cpu, gi, seg, g_t.double())
    masks = [(z > 0).double() for z in zs]
    u, pad = UNIT[c["dt"]], 2.0 ** -14 if c["dt"] == "f16" else 0.0
    mag, m_zs = reference(c, {k: None if t is None else t.abs() for k, t in cpu.items()}, gi, seg, g_t.double().abs() + pad,
                          masks=masks, a_pad=pad)
    assert torch.all(zs[0].abs() > (4 * (c["d"] + 2) * U + (c["count"] + 4) * U + u) * m_zs[0])
    assert all(torch.all(z.abs() > 4 * (c["ds"] + 2) * U * m) for z, m in zip(zs[1:], m_zs[1:]))
    _, got = run(c, dev, gi, seg, g_t)
    terms = int(seg[-1]) + c["d"] + c["ds"] + c["f"]
    for k, t in want.items():
        bound = ((1 + u) ** 3 - 1 + 4 * (terms + 2) * U) * mag[k] + (2.0 ** -25 if pad else 0.0)
        err = (got[k].double().cpu() - t).abs()
        print("%s %s: worst error / bound %.3f" % ("-".join(str(v) for v in case.values()), k, float((err / bound)[bound > 0].max())))
        assert torch.all(err <= bound), k


@pytest.mark.parametrize("dt", sorted(DT))
def test_mask_is_the_forwards(dt):
    """relu, no root, grad = ones: d_bias counts, per column, the destinations whose fused forward output is > 0"""
    c, _, gi, seg, _, dev = make(dict(dt=dt, op="mean", combine=None, size=300, count=5), real=True, seed=6)
    dev["b"] = torch.zeros_like(dev["b"])                  # pre-activations around 0
    out, got = run(c, dev, gi, seg, torch.ones((300, c["f"])), needs=("b",))
    assert torch.equal(got["b"], (out > 0).sum(0).to(got["b"].dtype))


@pytest.mark.parametrize("case", [{}, dict(dt="f32", op="mean", combine="fold"), dict(combine="concat", fs=24, size=1100)],
                         ids=["add", "fold", "concat-slabs"])
def test_same_bits(case):
    c, _, gi, seg, g_t, dev = make(case, real=True, seed=2)
    _, first = run(c, dev, gi, seg, g_t)
    _, again = run(c, dev, gi, seg, g_t)
    _, by_seg = run(c, dev, gi, seg, g_t, as_seg=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _, other = run(c, dev, gi, seg, g_t)
    side.synchronize()
    for k, t in first.items():
        for o in (again, by_seg, other):
            assert torch.equal(t.view(torch.int16 if t.element_size() == 2 else torch.int32),
                               o[k].view(torch.int16 if t.element_size() == 2 else torch.int32)), k
    assert set(first) == {k for k in NAMES if dev[k] is not None}


def test_partial_needs():
    c, _, gi, seg, g_t, dev = make({}, real=True, seed=3)
    _, full = run(c, dev, gi, seg, g_t)
    _, part = run(c, dev, gi, seg, g_t, needs=("w", "b"))
    assert set(part) == {"w", "b"} and all(torch.equal(part[k], full[k]) for k in part)


def test_example_fused_backward():
    run_ = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "sage_mean_minibatch.py"), "--nodes", "2000",
                           "--batch", "64", "--steps", "2", "--fused-backward"],
                          cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = run_.stdout.decode()
    assert run_.returncode == 0, text[-2000:]
    assert "fused backward agrees within the bound" in text, text[-2000:]
