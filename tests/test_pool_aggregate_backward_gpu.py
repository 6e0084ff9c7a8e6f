"""ops.pool_aggregate(backward="fused") (csrc/mp_pool_backward.h) against float64 autograd of the plain composed form -
gather with the range rule, matmul, relu, amax / sum / mean: exact on small integers, within a derived bound on real
values, the forward's mask and selection, same bits, partial needs, and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
U = 2.0 ** -24
HUB = [0, 1, 300, 0, 0, 1, 5, 16, 17, 0, 33, 2, 0]
NAMES = ("table", "w", "b")

BASE = dict(dt="bf16", op="max", act="relu", d=64, f=64, count=4, size=65, gather="int32", lens=None, off=0, grad="f32",
            bias="f32")
# one-axis sweeps around BASE.  Grid cap of the walk kernels: 1024 workgroups x 64 destinations; slabs of the weight
# kernel: 1024 positions, 512 jobs of (slab, 64 k, 64 f) - 172 slabs x 3 f tiles at the last case.
EXACT = {
    "base": {}, "f32": dict(dt="f32"), "f16": dict(dt="f16"), "add": dict(op="add"), "mean": dict(op="mean"),
    "none": dict(act="none"), "add-none": dict(op="add", act="none"), "mean-none-same": dict(op="mean", act="none", grad="same"),
    **{"d%d" % d: dict(d=d) for d in (1, 7, 8, 31, 32, 33, 160, 161, 256)},
    **{"F%d" % f: dict(f=f) for f in (1, 15, 16, 17, 130)}, "F512": dict(f=512, d=256, size=17),
    "f32-d65-F130": dict(dt="f32", d=65, f=130),
    **{"size%d" % s: dict(size=s) for s in (1, 15, 16, 17, 257)},
    "seg-max": dict(lens=HUB), "seg-add": dict(lens=HUB, op="add"), "seg-max-none": dict(lens=HUB, gather=None),
    "seg-add-none": dict(lens=HUB, op="add", gather=None),
    "gather-none": dict(gather=None), "gather-int64": dict(gather="int64"), "gather-int32-bad": dict(gather="int32-bad"),
    "gather-int64-bad": dict(gather="int64-bad"), "off4": dict(off=2), "no-bias": dict(bias=None), "bias-same": dict(bias="same"),
    "grad-same": dict(grad="same"),
    "walk-grid-cap": dict(size=65536 + 17, count=1, d=8, f=16), "weight-jobs": dict(size=171 * 1024 + 1, count=1, d=8, f=130),
}


def make(case, real=False, seed=0):
    """-> (c, float64 CPU tensors of the stored values by name, gi, seg, g_out, device tensors by name)"""
    c = dict(BASE, **case)
    rng = np.random.default_rng(seed)
    d, f, dt = c["d"], c["f"], DT[c["dt"]]
    seg = np.arange(c["size"] + 1) * c["count"] if c["lens"] is None else np.concatenate([[0], np.cumsum(c["lens"])])
    size, e = len(seg) - 1, int(seg[-1])
    hub_max = c["lens"] is not None and c["op"] == "max" and not real
    rows = max(e, 1) if c["gather"] is None else (e + 7 if real else 192 if hub_max else 97)

    def sparse(k, n, hits):                              # about `hits` entries of -2 .. 2 per column
        a, at = np.zeros(k * n, dtype=np.int64), rng.integers(0, k * n, int(min(1.0, hits / k) * k * n))
        a[at] = rng.integers(-2, 3, len(at))
        return a.reshape(k, n)
    if real:
        v = dict(table=rng.standard_normal((rows, d)), b=0.5 * np.where(np.arange(f) % 2, 1.0, -1.0),
                 w=rng.standard_normal((d, f)) / np.sqrt(d))
        g_out = rng.standard_normal((size, f))
    elif hub_max:
        # a long segment: every column of h holds a value at most twice per segment.  Each feature is a permutation of
        # distinct integers, each column of W reads ONE feature, a row is gathered at most twice per segment; one even
        # grad per column, so that every weight gradient is one table value times a power of two
        v = dict(table=np.stack([rng.permutation(rows) - rows // 2 for _ in range(d)], 1), b=rng.integers(-2, 3, f),
                 w=np.zeros((d, f), dtype=np.int64))
        v["w"][rng.permutation(d)[np.arange(f) % d], np.arange(f)] = rng.choice([-1, 1], f)
    else:
        v = dict(table=rng.integers(-2, 3, (rows, d)), b=rng.integers(-2, 3, f), w=sparse(d, f, 6.0))
    if not real and c["lens"] is not None:               # the long segment: one even grad per column
        g_out = np.zeros((size, f), dtype=np.int64)
        g_out[rng.choice(np.nonzero(np.diff(seg))[0], f), np.arange(f)] = rng.choice([-4, -2, 2, 4], f)
    elif not real:
        # a few terms per column, so that every sum over r stays small; max: multiples of 12, which 1 .. 4 ties divide
        g_out = sparse(size, f, 6.0) * (12 if c["op"] == "max" else 1)
    flat = torch.zeros(rows * d + 8, dtype=dt)
    flat[c["off"]:c["off"] + rows * d] = torch.as_tensor(v["table"].reshape(-1), dtype=dt)
    dev = {k: torch.as_tensor(v[k], dtype=torch.float32 if k == "b" and c["bias"] == "f32" else dt).cuda() for k in NAMES}
    dev["table"] = flat.cuda()[c["off"]:c["off"] + rows * d].view(rows, d)
    if c["bias"] is None:
        dev["b"] = None
    gi = None
    if c["gather"] is not None:
        kind = np.int64 if c["gather"].startswith("int64") else np.int32
        if hub_max:
            gi = np.concatenate([rng.permutation(np.tile(np.arange(rows), 2))[:n] for n in c["lens"]]).astype(kind)
        else:                                            # real values: no row twice, so that no two candidates tie
            gi = (rng.permutation(rows)[:e] if real else rng.integers(0, rows, e)).astype(kind)
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
    out = ops.pool_aggregate(c["op"], leaf["table"], leaf["w"], None if gi is None else torch.as_tensor(gi).cuda(), len(seg) - 1,
                             bias=leaf["b"], activation=c["act"], out_dtype=g_t.dtype, backward=backward, **form)
    out.backward(g_t.cuda())
    return out, {k: t.grad for k, t in leaf.items() if t is not None and k in needs}


def composed64(c, seg, table, w, b, gi, picked=None):
    """the plain composed form in float64 -> (out, z, h); picked: a held mask [e, F] instead of relu and the selection"""
    g = torch.arange(int(seg[-1])) if gi is None else torch.as_tensor(gi.astype(np.int64))
    ok = (g >= 0) & (g < table.shape[0])
    z = (table[torch.where(ok, g, torch.zeros_like(g))] * ok[:, None]) @ w
    z = z if b is None else z + b
    h = z * picked if picked is not None else (torch.relu(z) if c["act"] == "relu" else z)
    how = "add" if picked is not None else c["op"]         # (a held selection: the picked terms are summed)
    fold = lambda t, dim: t.sum(dim) if how == "add" else t.mean(dim) if how == "mean" else t.amax(dim)
    if c["lens"] is None:                                # equal segments: one reshape
        out = fold(h.view(len(seg) - 1, c["count"], -1), 1)
    else:
        out = torch.stack([fold(h[a:b_], 0) if b_ > a else h.new_zeros(h.shape[1]) for a, b_ in zip(seg[:-1], seg[1:])])
    return out, z, h


def reference(c, cpu, gi, seg, g64, picked=None):
    leaf = {k: None if t is None else t.clone().requires_grad_(True) for k, t in cpu.items()}
    out, z, h = composed64(c, seg, leaf["table"], leaf["w"], leaf["b"], gi, picked)
    out.backward(g64)
    return {k: t.grad for k, t in leaf.items() if t is not None}, out.detach(), z.detach(), h.detach()


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_integers(name):
    """every gradient is an integer or dyadic value its dtype holds (asserted on the reference first): compared with =="""
    c, cpu, gi, seg, g_t, dev = make(EXACT[name])
    want = reference(c, cpu, gi, seg, g_t.double())[0]
    for k, t in want.items():
        assert torch.equal(t.to(dev[k].dtype).double(), t), (name, k, "the reference does not fit the dtype")
    _, got = run(c, dev, gi, seg, g_t)
    for k, t in want.items():
        wrong = torch.nonzero(got[k].double().cpu() != t)
        assert got[k].dtype == dev[k].dtype and len(wrong) == 0, (name, k, len(wrong), wrong[:5])


REAL = [dict(dt=dt, op=op, size=37, d=24, f=20, count=5) for dt in sorted(DT) for op in ("max", "mean", "add")]


@pytest.mark.parametrize("case", REAL, ids=lambda c: "%s-%s" % (c["dt"], c["op"]))
def test_real_values_within_bound(case):
    """Against float64 autograd on the stored values, grad in fp32.  Checked first, with the forward's bound 4 (d + 2) 2^-24
    (|x| |w| + |b|) of a pre-activation: none lies within it of 0, and for max the two largest candidates of every
    (segment, column) are more than twice it apart or all are dead - so the masks and the selection agree.  Bound of a
    gradient element: M, the same graph on absolute values with the masks and the selection held, times 4 (terms + 2) 2^-24
    - terms = e + d + F bounds the rounded fp32 operations behind it (the share, the accumulations, the slab sums, the
    grouped add), x4 because an MFMA's rounding is undocumented - plus two narrowings of unit roundoff u of the table's
    dtype, the dZ operand and the stored gradient: (1 + u)^2 - 1.  fp16: a narrowing also errs by up to 2^-25 absolutely
    below the normal range, u (|x| + 2^-14) in all: M is taken with 2^-14 added to |grad|, and 2^-25 is added for the
    stored gradient."""
    c, cpu, gi, seg, g_t, dev = make(case, real=True, seed=7)     # (a seed at which the preconditions hold for every case)
    want, out, z, h = reference(c, cpu, gi, seg, g_t.double())
    count, u, pad = c["count"], UNIT[c["dt"]], 2.0 ** -14 if c["dt"] == "f16" else 0.0
    picked = (z > 0).double()
    if c["op"] == "max":
        picked = picked * (h == out.repeat_interleave(count, 0))
    scale = 1.0 / count if c["op"] == "mean" else 1.0
    absolute = {k: t.abs() for k, t in cpu.items()}
    mag = reference(c, absolute, gi, seg, (g_t.double().abs() + pad) * scale, picked=picked)[0]
    fwd = 4 * (c["d"] + 2) * U * composed64(dict(c, act="none"), seg, absolute["table"], absolute["w"], absolute["b"], gi)[1]
    assert torch.all(z.abs() > fwd)
    if c["op"] == "max":
        top = torch.topk(h.view(-1, count, c["f"]), 2, dim=1).values
        dead = (z + fwd).view(-1, count, c["f"]).amax(1) < 0
        assert torch.all((top[:, 0] - top[:, 1] > 2 * fwd.view(-1, count, c["f"]).amax(1)) | dead)
    _, got = run(c, dev, gi, seg, g_t)
    terms = int(seg[-1]) + c["d"] + c["f"]
    for k, t in want.items():
        bound = ((1 + u) ** 2 - 1 + 4 * (terms + 2) * U) * mag[k] + (2.0 ** -25 if pad else 0.0)
        err = (got[k].double().cpu() - t).abs()
        print("%s-%s %s: worst error / bound %.3f" % (c["dt"], c["op"], k, float((err / bound)[bound > 0].max())))
        assert torch.all(err <= bound), k


@pytest.mark.parametrize("dt", sorted(DT))
def test_mask_and_selection_are_the_forwards(dt):
    """relu, max, grad = ones: the shares of a segment sum to 1 where its maximum is > 0, so d_bias counts, per column,
    the destinations whose fused forward output is > 0"""
    c, _, gi, seg, _, dev = make(dict(dt=dt, size=300, count=5), real=True, seed=6)
    dev["b"] = torch.zeros_like(dev["b"])                  # pre-activations around 0
    out, got = run(c, dev, gi, seg, torch.ones((300, c["f"])), needs=("b",))
    assert torch.equal(got["b"], (out > 0).sum(0).to(got["b"].dtype))


@pytest.mark.parametrize("case", [{}, dict(op="add", size=1100)], ids=["max", "add-slabs"])
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
    assert set(first) == set(NAMES)


def test_partial_needs():
    c, _, gi, seg, g_t, dev = make({}, real=True, seed=3)
    _, full = run(c, dev, gi, seg, g_t)
    _, part = run(c, dev, gi, seg, g_t, needs=("w", "b"))
    assert set(part) == {"w", "b"} and all(torch.equal(part[k], full[k]) for k in part)


def test_example_fused_backward():
    run_ = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "sage_pool_minibatch.py"), "--nodes", "2000",
                           "--batch", "64", "--steps", "2", "--fused-backward"],
                          cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = run_.stdout.decode()
    assert run_.returncode == 0, text[-2000:]
    assert "fused backward agrees within the bound" in text, text[-2000:]
