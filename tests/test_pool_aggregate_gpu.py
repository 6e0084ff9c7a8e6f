"""ops.pool_aggregate (csrc/mp_pool.h) against the float64 reference of pool_aggregate_ref.py: exact on
small integers (a wrong fragment layout, tail, tile plan or fold boundary is a wrong integer), within
the derived bound on real values, same bits, and gradients against float64 autograd."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from pool_aggregate_ref import pool_ref

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
U = 2.0 ** -24
HUB = [0, 1, 300, 0, 0, 1, 5, 16, 17, 0, 33, 2, 0]          # segment lengths of the seg_ptr cases

BASE = dict(dt="bf16", op="max", act="relu", d=64, f=64, count=10, size=65, gather="int32", lens=None, out="f32",
            off=0, bias="f32")
# one-axis sweeps around BASE; the tiling boundaries are those of PoolMakePlan (mp_pool.h)
EXACT = {
    "base": {},
    "f32": dict(dt="f32"), "f16": dict(dt="f16"),
    "mean": dict(op="mean", count=8), "add": dict(op="add"), "none": dict(act="none"),
    **{"d%d" % d: dict(d=d) for d in (1, 7, 8, 31, 32, 33, 130)},
    **{"F%d" % f: dict(f=f) for f in (1, 15, 16, 17, 130)},
    **{"count%d" % c: dict(count=c, op="add") for c in (1, 3, 16, 17, 25)},
    **{"size%d" % s: dict(size=s) for s in (0, 1, 257)},
    "seg-max": dict(lens=HUB), "seg-add": dict(lens=HUB, op="add"),
    "gather-none": dict(gather=None), "gather-int32-bad": dict(gather="int32-bad"), "gather-int64-bad": dict(gather="int64-bad"),
    "off4": dict(off=2), "off4-f32": dict(dt="f32", off=1),
    "out-bf16": dict(out="same", d=16), "out-f16": dict(dt="f16", out="same", d=16), "bias-same": dict(bias="same"),
    "no-bias": dict(bias=None),
    # F tile 128 | 64 (16-bit: d 160 | 161), two F passes each
    "tile-d160-F130": dict(d=160, f=130, op="add"), "tile-d161-F130": dict(d=161, f=130, op="add"),
    "tile-f32-d64-F130": dict(dt="f32", d=64, f=130), "tile-f32-d65-F130": dict(dt="f32", d=65, f=130),
    # F tile 32, nine passes: W does not fit one LDS residency
    "tile-d520-F272": dict(d=520, f=272),
    # K tile boundary: W^T of 16 columns fits up to d = 1440 (fp32 704); beyond, K is tiled and the waves run in lockstep
    "ktile-d1440": dict(d=1440, f=17, size=9), "ktile-d1441-seg": dict(d=1441, f=17, lens=HUB, op="add"),
    "ktile-f32-d704": dict(dt="f32", d=704, f=16, size=9), "ktile-f32-d705-seg": dict(dt="f32", d=705, f=16, lens=HUB),
    # past the launcher's grid cap: 1024 workgroups x 4 runs x 16 destinations
    "grid-cap": dict(d=8, f=16, count=1, size=65536 + 17, op="add"),
}


def make(case, real=False, seed=0):
    """-> (args for ops.pool_aggregate on the device, args for pool_ref)"""
    c = dict(BASE, **case)
    rng = np.random.default_rng(seed)
    d, f, size, dt = c["d"], c["f"], c["size"], DT[c["dt"]]
    seg = np.arange(size + 1) * c["count"] if c["lens"] is None else np.concatenate([[0], np.cumsum(c["lens"])])
    size, e = len(seg) - 1, int(seg[-1])
    rows = e if c["gather"] is None else 97
    if real:
        table, w, b = rng.standard_normal((rows, d)), rng.standard_normal((d, f)) / np.sqrt(d), rng.standard_normal(f)
    else:
        table = rng.integers(-2, 3, (rows, d))
        w = rng.integers(-2, 3, (d, f)) * (rng.random((d, f)) < min(1.0, 6.0 / d))
        b = rng.integers(-2, 3, f)
    flat = torch.zeros(rows * d + 8, dtype=dt)
    flat[c["off"]:c["off"] + rows * d] = torch.as_tensor(table.reshape(-1), dtype=dt)
    table_t = flat.cuda()[c["off"]:c["off"] + rows * d].view(rows, d)
    w_t = torch.as_tensor(w, dtype=dt).cuda()
    b_t = None if c["bias"] is None else torch.as_tensor(b, dtype=torch.float32 if c["bias"] == "f32" else dt).cuda()
    gi = None
    if c["gather"] is not None:
        gi = rng.integers(0, rows, e).astype(np.int64 if c["gather"].startswith("int64") else np.int32)
        if c["gather"].endswith("bad"):
            bad = [-1, rows] + ([2 ** 40, 2 ** 32 + 3] if gi.dtype == np.int64 else [])
            gi[::3] = np.resize(bad, len(gi[::3]))
    gi_t = None if gi is None else torch.as_tensor(gi).cuda()
    kw = dict(bias=b_t, activation=c["act"], out_dtype=torch.float32 if c["out"] == "f32" else None)
    if c["lens"] is None:
        kw["count"] = c["count"]
    else:
        kw["seg_ptr"] = torch.as_tensor(seg).cuda()
    stored = lambda t: None if t is None else t.double().cpu().numpy()
    return (c["op"], table_t, w_t, gi_t, size), kw, (c["op"], stored(table_t), stored(w_t), gi, seg, stored(b_t), c["act"])


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_integers(name):
    from euler_amd import ops
    args, kw, ref_args = make(EXACT[name])
    out = ops.pool_aggregate(*args, **kw)
    want = pool_ref(*ref_args)
    assert out.shape == want.shape and out.dtype == (kw["out_dtype"] or args[1].dtype)
    got = out.double().cpu().numpy()
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, (name, len(wrong), wrong[:5], got[tuple(wrong[0])], want[tuple(wrong[0])])


REAL = [dict(dt=dt, op=op, **shape) for dt in DT for op in ("max", "mean", "add") for shape in ({}, dict(d=130, f=130))]


@pytest.mark.parametrize("case", REAL, ids=lambda c: "-".join(str(v) for v in c.values()))
def test_real_values_within_bound(case):
    """|s^ - s| <= (d + 2) 2^-24 (sum |x||w| + |b|) before the activation; relu and max are 1-Lipschitz; add / mean
    add len 2^-24 sum |h| for the fold.  4x on the accumulation term: an MFMA's rounding is not documented."""
    from euler_amd import ops
    args, kw, ref_args = make(case, real=True, seed=1)
    got = ops.pool_aggregate(*args, **kw).double().cpu().numpy()
    op, table, w, gi, seg, b, _ = ref_args
    want = pool_ref(*ref_args)
    absolute = pool_ref(op, np.abs(table), np.abs(w), gi, seg, np.abs(b), "none")
    acc = (table.shape[1] + 2) * U * absolute
    fold = 0.0 if op == "max" else BASE["count"] * U * absolute
    ratio = (np.abs(got - want) / (acc + fold)).max()
    print("pool_aggregate error / bound (no margin): %s %.3f" % (case, ratio))
    assert np.all(np.abs(got - want) <= 4 * acc + fold)


@pytest.mark.parametrize("op", ["max", "add"])
def test_same_bits(op):
    from euler_amd import ops
    args, kw, _ = make(dict(op=op), real=True, seed=2)
    first = ops.pool_aggregate(*args, **kw)
    again = ops.pool_aggregate(*args, **kw)
    seg = torch.arange(BASE["size"] + 1, device="cuda") * BASE["count"]
    as_seg = ops.pool_aggregate(*args, **dict({k: v for k, v in kw.items() if k != "count"}, seg_ptr=seg))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.pool_aggregate(*args, **kw)
    side.synchronize()
    for t in (again, as_seg, other):
        assert torch.equal(first.view(torch.int32), t.view(torch.int32))


def composed64(op, table, w, b, gi, seg, act):
    """the composed form in float64 torch on the CPU, for autograd"""
    ok = (gi >= 0) & (gi < table.shape[0])
    x = table[torch.where(ok, gi, torch.zeros_like(gi))] * ok[:, None]
    z = x @ w + b
    h = torch.relu(z) if act == "relu" else z
    rows = []
    for r in range(len(seg) - 1):
        t = h[seg[r]:seg[r + 1]]
        rows.append(t.amax(0) if op == "max" else t.sum(0) if op == "add" else t.mean(0))
    return torch.stack(rows), h, z


def _grads(op, count, real, monkeypatch):
    from euler_amd import ops
    monkeypatch.setattr(ops, "POOL_GRAD_CHUNK_ROWS", 10 * count)      # 37 destinations: four chunks
    rng = np.random.default_rng(3)
    rows, d, f, size = 4 * 37 * count, 24, 20, 37
    seg = np.arange(size + 1) * count
    draw = rng.standard_normal if real else (lambda s: rng.integers(-2, 3, s).astype(np.float64))
    table, w, b, g_out = draw((rows, d)), draw((d, f)), draw(f), draw((size, f))
    gi = rng.permutation(rows)[:size * count].astype(np.int64)       # (no row twice: a max has one position)
    gi[5], gi[17] = -1, 2 ** 40
    dev = [torch.tensor(t, dtype=torch.float32, device="cuda", requires_grad=True) for t in (table, w, b)]
    out = ops.pool_aggregate(op, dev[0], dev[1], torch.as_tensor(gi).cuda(), size, bias=dev[2], count=count,
                             activation="relu")
    out.backward(torch.tensor(g_out, dtype=torch.float32, device="cuda"))
    cpu = [torch.tensor(t.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True) for t in dev]
    want, h, z = composed64(op, *cpu, torch.as_tensor(gi), seg, "relu")
    want.backward(torch.tensor(g_out))
    return dev, cpu, (gi, g_out, want, h, z)


@pytest.mark.parametrize("op,count", [("add", 5), ("mean", 4)])
def test_gradients_exact_integers(op, count, monkeypatch):
    dev, cpu, _ = _grads(op, count, False, monkeypatch)
    for got, want in zip(dev, cpu):
        assert torch.equal(got.grad.double().cpu(), want.grad)


def test_gradients_max(monkeypatch):
    """Real values.  The selection cannot flip: the gap between the two largest candidates of every
    (segment, column) exceeds the forward bound.  Bound of a gradient element: the reference on absolute
    values times (terms + 2) 2^-24, x4; terms = F for the table (no row is gathered twice), e for dW and db."""
    count = 5
    dev, cpu, (gi, g_out, want, h, z) = _grads("max", count, True, monkeypatch)
    table, w, b = [t.detach() for t in cpu]
    top = torch.topk(h.detach().view(-1, count, h.shape[1]), 2, dim=1).values
    fwd_bound = 4 * (table.shape[1] + 2) * U * (table.abs().max(0).values @ w.abs() + b.abs())
    dead = (z.detach().view(-1, count, h.shape[1]).amax(1) < -fwd_bound)      # every candidate below 0: no gradient
    assert torch.all((top[:, 0] - top[:, 1] > 2 * fwd_bound) | dead)
    absolute = [torch.tensor(t.numpy(), requires_grad=True) for t in (table.abs(), w.abs(), b.abs())]
    ok = torch.as_tensor((gi >= 0) & (gi < table.shape[0]))
    x = absolute[0][torch.as_tensor(np.where(ok, gi, 0))] * ok[:, None]
    picked = ((h.detach() == want.detach().repeat_interleave(count, 0)) & (z.detach() > 0)).double()      # the reference's selection
    ((x @ absolute[1] + absolute[2]) * picked * torch.tensor(np.abs(g_out)).repeat_interleave(count, 0)).sum().backward()
    for got, ref, mag, terms in zip(dev, cpu, absolute, (w.shape[1], len(gi), len(gi))):
        bound = 4 * (terms + 2) * U * mag.grad
        assert torch.all((got.grad.double().cpu() - ref.grad).abs() <= bound)


def test_example_routes_agree():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "sage_pool_minibatch.py"),
                          "--nodes", "2000", "--batch", "64", "--steps", "2", "--composed", "--check"],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = run.stdout.decode()
    assert run.returncode == 0, text[-2000:]
    assert "routes agree within the bound" in text, text[-2000:]
