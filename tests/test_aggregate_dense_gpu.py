"""ops.aggregate_dense (csrc/mp_dense.h) against the float64 reference of aggregate_dense_ref.py: exact on
small integers (a wrong fragment layout, tail, plan boundary or predicated walk is a wrong integer), today's
gather_segment_reduce under an identity weight, within the derived bound on real values, same bits, and
gradients against float64 autograd."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from aggregate_dense_ref import dense_ref

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}       # unit roundoff of the narrowing
U = 2.0 ** -24
HUB = [0, 1, 300, 0, 0, 1, 5, 16, 17, 0, 33, 2, 0]          # segment lengths of the seg_ptr cases

BASE = dict(dt="bf16", op="add", act="relu", combine="add", d=64, ds=64, f=64, fs=None, count=10, size=65,
            gather="int32", lens=None, out="f32", off=0, bias="f32", scale=None)
# one-axis sweeps around BASE; the plan boundaries are those of DenseMakePlan (mp_dense.h)
EXACT = {
    "base": {},
    "f32": dict(dt="f32"), "f16": dict(dt="f16"),
    "mean": dict(op="mean", count=8), "mean-f32": dict(op="mean", count=4, dt="f32"), "none": dict(act="none"),
    "concat": dict(combine="concat", fs=40), "concat-wide-self": dict(combine="concat", f=17, fs=130),
    "fold": dict(combine="fold"), "fold-gin": dict(combine="fold", scale=3.0, act="none"),
    "fold-mean": dict(combine="fold", op="mean", count=7), "no-root": dict(combine=None),
    "no-root-mean-seg": dict(combine=None, op="mean", lens=[0, 2, 256, 0, 4, 16, 32, 0, 8]),
    **{"d%d" % d: dict(d=d) for d in (1, 7, 8, 31, 32, 33, 128, 129, 136)},
    **{"ds%d" % d: dict(ds=d) for d in (1, 7, 8, 31, 32, 33, 128, 129, 136)},
    **{"fold-d%d" % d: dict(d=d, combine="fold", dt="f32") for d in (7, 129, 136)},
    **{"F%d" % f: dict(f=f) for f in (1, 15, 16, 17, 130)},
    **{"count%d" % c: dict(count=c) for c in (1, 3, 16, 17, 25)},
    **{"size%d" % s: dict(size=s) for s in (0, 1, 15, 16, 17, 257)},
    "seg": dict(lens=HUB), "seg-f32-fold": dict(lens=HUB, dt="f32", combine="fold"),
    "gather-none": dict(gather=None), "gather-int32-bad": dict(gather="int32-bad"),
    "gather-int64-bad": dict(gather="int64-bad"), "gather-bad-mean": dict(gather="int64-bad", op="mean", count=8),
    "off4": dict(off=2), "off4-f32": dict(dt="f32", off=1),
    "out-bf16": dict(out="same"), "out-f16": dict(dt="f16", out="same"), "bias-same": dict(bias="same"),
    "no-bias": dict(bias=None),
    # NT by F: 1 | 2 | 4 | 8 at F 16 | 17, 32 | 33, 64 | 65
    "nt-F32": dict(f=32), "nt-F33": dict(f=33), "nt-F65": dict(f=65),
    # NT by the 64 KB of both paths' W: 8 | 4 at d = ds = 128 | 129 (128: packed columns, exactly 64 KB),
    # 4 | 2 at 256 | 257, 2 | 1 at 512 | 513
    "lds-d128-F130": dict(d=128, ds=128, f=130), "lds-d129-F130": dict(d=129, ds=129, f=130),
    "lds-d256-F40": dict(d=256, ds=256, f=40, size=17), "lds-d257-F40": dict(d=257, ds=257, f=40, size=17),
    "lds-d512-F20": dict(d=512, ds=512, f=20, size=17), "lds-d513-F20": dict(d=513, ds=513, f=20, size=17),
    "lds-d1024-F17": dict(d=1024, ds=1024, f=17, size=9, count=3),
    # fp32: both paths' 16 columns fit up to d = ds = 512; beyond, K is tiled and the waves run in lockstep
    "lock-f32-d512": dict(dt="f32", d=512, ds=512, f=16, size=17), "lock-f32-d513-seg": dict(dt="f32", d=513, ds=512, f=17, lens=HUB),
    "lock-f32-d1024": dict(dt="f32", d=1024, ds=1000, f=16, size=70, count=3),
    # past the launcher's grid cap: 512 workgroups x 4 runs x 16 destinations, twice over
    "grid-cap": dict(d=8, ds=8, f=16, count=1, size=65536 + 17),
}


def make(case, real=False, seed=0):
    """-> (positional args, keyword args for ops.aggregate_dense on the device, args for dense_ref)"""
    c = dict(BASE, **case)
    rng = np.random.default_rng(seed)
    d, f, dt, comb = c["d"], c["f"], DT[c["dt"]], c["combine"]
    ds, fs = (d, None) if comb == "fold" else (c["ds"], c["fs"] or f)
    seg = np.arange(c["size"] + 1) * c["count"] if c["lens"] is None else np.concatenate([[0], np.cumsum(c["lens"])])
    size, e = len(seg) - 1, int(seg[-1])
    rows = max(e, 1) if c["gather"] is None else 97
    if real:
        table, b, root = rng.standard_normal((rows, d)), rng.standard_normal(f), rng.standard_normal((size, ds))
        w, ws = rng.standard_normal((d, f)) / np.sqrt(d), rng.standard_normal((ds, fs or 1)) / np.sqrt(ds)
    else:
        sparse = lambda k, n: rng.integers(-2, 3, (k, n)) * (rng.random((k, n)) < min(1.0, 6.0 / k))
        table, b, root = rng.integers(-2, 3, (rows, d)), rng.integers(-2, 3, f), rng.integers(-2, 3, (size, ds))
        w, ws = sparse(d, f), sparse(ds, fs or 1)
    flat = torch.zeros(rows * d + 8, dtype=dt)
    flat[c["off"]:c["off"] + rows * d] = torch.as_tensor(table.reshape(-1), dtype=dt)
    table_t = flat.cuda()[c["off"]:c["off"] + rows * d].view(rows, d)
    dev = lambda a, t=dt: torch.as_tensor(a, dtype=t).cuda()
    b_t = None if c["bias"] is None else dev(b, torch.float32 if c["bias"] == "f32" else dt)
    root_t = None if comb is None else dev(root)
    ws_t = dev(ws) if comb in ("add", "concat") else None
    w_t = dev(w)
    gi = None
    if c["gather"] is not None:
        gi = rng.integers(0, rows, e).astype(np.int64 if c["gather"].startswith("int64") else np.int32)
        if c["gather"].endswith("bad"):
            bad = [-1, rows] + ([2 ** 40, 2 ** 32 + 3] if gi.dtype == np.int64 else [])
            gi[::3] = np.resize(bad, len(gi[::3]))
    kw = dict(root=root_t, root_weight=ws_t, combine=comb or "add", root_scale=c["scale"], bias=b_t, activation=c["act"],
              out_dtype=torch.float32 if c["out"] == "f32" else None)
    kw.update(dict(count=c["count"]) if c["lens"] is None else dict(seg_ptr=torch.as_tensor(seg).cuda()))
    stored = lambda t: None if t is None else t.double().cpu().numpy()
    ref = dict(root=stored(root_t), ws=stored(ws_t), combine=comb, scale=c["scale"])
    return ((c["op"], table_t, w_t, None if gi is None else torch.as_tensor(gi).cuda(), size), kw,
            ((c["op"], stored(table_t), stored(w_t), gi, seg, stored(b_t), c["act"], dt), ref))


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_integers(name):
    from euler_amd import ops
    args, kw, (ref_args, ref_kw) = make(EXACT[name])
    out = ops.aggregate_dense(*args, **kw)
    want = torch.as_tensor(dense_ref(*ref_args, **ref_kw)).to(out.dtype).double().numpy()
    assert out.shape == want.shape and out.dtype == (kw["out_dtype"] or args[1].dtype)
    got = out.double().cpu().numpy()
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, (name, len(wrong), wrong[:5], got[tuple(wrong[0])], want[tuple(wrong[0])])


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("op,count", [("mean", 10), ("add", 10), ("mean", 1)])
def test_identity_weight_is_gather_segment_reduce(dt, op, count):
    """d == F, weight = I, no bias, no activation, no root: the fold and the narrowing are today's op"""
    from euler_amd import ops
    args, kw, _ = make(dict(dt=dt, op=op, count=count, combine=None, out="same", f=BASE["d"]), real=True, seed=4)
    _, table, _, gi, size = args
    eye = torch.eye(BASE["d"], dtype=table.dtype, device="cuda")
    out = ops.aggregate_dense(op, table, eye, gi, size, activation="none", count=count)
    assert torch.equal(out, ops.gather_segment_reduce(op, table, gi, size, count=count))


REAL = [dict(dt=dt, op=op, **shape) for dt in sorted(DT) for op in ("mean", "add")
        for shape in ({}, dict(d=130, ds=33, f=130), dict(combine="concat", fs=24), dict(combine="fold", scale=1.5))]


@pytest.mark.parametrize("case", REAL, ids=lambda c: "-".join(str(v) for v in c.values()))
def test_real_values_within_bound(case):
    """With M = the reference on absolute values, no activation and no narrowing (sum |a||w| + |b| of both paths;
    relu is 1-Lipschitz): the fold's len roundings carry len 2^-24 M; mean's denominator fl(len + 1e-7f) and its
    division 3 x 2^-24 M; the narrowing of A one unit roundoff of the table's dtype times M (none for fp32); the fp32
    accumulation (d + ds + 2) 2^-24 M, x4 as for pool_aggregate: an MFMA's rounding is not documented; the output is
    fp32 here, so its rounding is inside the accumulation term."""
    from euler_amd import ops
    c = dict(BASE, **case)
    args, kw, (ref_args, ref_kw) = make(case, real=True, seed=1)
    got = ops.aggregate_dense(*args, **kw).double().cpu().numpy()
    want = dense_ref(*ref_args, **ref_kw)
    op, table, w, gi, seg, b, _, _ = ref_args
    mag = dense_ref(op, np.abs(table), np.abs(w), gi, seg, np.abs(b), "none", None,
                    **{k: np.abs(v) if isinstance(v, np.ndarray) else v for k, v in ref_kw.items()})
    ds = 0 if c["combine"] == "fold" else c["ds"]
    plain = ((c["count"] + 1) * U + (3 * U if op == "mean" else 0.0) + UNIT[c["dt"]]) * mag
    acc = (c["d"] + ds + 2) * U * mag
    assert np.all(np.abs(got - want) <= 4 * acc + plain)


@pytest.mark.parametrize("case", [{}, dict(dt="f32", op="mean", combine="fold")], ids=["add", "fold"])
def test_same_bits(case):
    from euler_amd import ops
    args, kw, _ = make(case, real=True, seed=2)
    first = ops.aggregate_dense(*args, **kw)
    again = ops.aggregate_dense(*args, **kw)
    seg = torch.arange(BASE["size"] + 1, device="cuda") * BASE["count"]
    as_seg = ops.aggregate_dense(*args, **dict({k: v for k, v in kw.items() if k != "count"}, seg_ptr=seg))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.aggregate_dense(*args, **kw)
    side.synchronize()
    for t in (again, as_seg, other):
        assert torch.equal(first.view(torch.int32), t.view(torch.int32))


def composed64(op, comb, scale, count, table, w, b, root, ws, gi, masks=None):
    """the formula in float64 torch on the CPU, for autograd; masks: fixed relu masks (for magnitudes)"""
    ok = (gi >= 0) & (gi < table.shape[0])
    x = (table[torch.where(ok, gi, torch.zeros_like(gi))] * ok[:, None]).view(-1, count, table.shape[1])
    a, n = x.sum(1), count
    if comb == "fold":
        a, n = a + scale * root, count + 1
    zs = [(a / n if op == "mean" else a) @ w + b] + ([root @ ws] if comb in ("add", "concat") else [])
    hs = [torch.relu(z) if masks is None else z * m for z, m in zip(zs, masks or zs)]
    out = hs[0] if len(hs) == 1 else hs[0] + hs[1] if comb == "add" else torch.cat([hs[1], hs[0]], 1)
    return out, zs


@pytest.mark.parametrize("op,comb", [("mean", "add"), ("add", "concat"), ("mean", "fold"), ("add", None)])
def test_gradients(op, comb, monkeypatch):
    """fp32 on the device against float64 autograd.  No pre-activation of the case lies within the forward bound
    of 0 (checked here), so the masks agree.  Bound of a gradient element: the same graph on absolute values with
    the masks held, times (terms + 2) 2^-24, x4; terms = e + d + ds + F bounds the rounded operations behind it."""
    from euler_amd import ops
    count, size, d, ds, f, fs, scale = 4, 37, 24, 24 if comb == "fold" else 12, 20, 20 if comb != "concat" else 9, 1.5
    monkeypatch.setattr(ops, "POOL_GRAD_CHUNK_ROWS", 10 * count)      # 37 destinations: four chunks
    rng = np.random.default_rng(3)
    rows = 50
    gi = rng.integers(0, rows, size * count)
    gi[5], gi[17] = -1, 2 ** 40
    shapes = dict(table=(rows, d), w=(d, f), b=(f,), root=(size, ds), ws=(ds, fs))
    names = ["table", "w", "b"] + (["root"] if comb else []) + (["ws"] if comb in ("add", "concat") else [])
    vals = {k: rng.standard_normal(shapes[k]) for k in shapes}
    g_out = rng.standard_normal((size, f + fs if comb == "concat" else f))
    dev = {k: torch.tensor(vals[k], dtype=torch.float32, device="cuda", requires_grad=True) for k in names}
    out = ops.aggregate_dense(op, dev["table"], dev["w"], torch.as_tensor(gi).cuda(), size, root=dev.get("root"),
                              root_weight=dev.get("ws"), combine=comb or "add", root_scale=scale if comb == "fold" else None,
                              bias=dev["b"], count=count)
    out.backward(torch.tensor(g_out, dtype=torch.float32, device="cuda"))
    cpu = {k: torch.tensor(dev[k].detach().cpu().numpy() if k in dev else vals[k], dtype=torch.float64,
                           requires_grad=k in dev) for k in shapes}
    order = lambda t: [t[k] for k in ("table", "w", "b", "root", "ws")]
    want, zs = composed64(op, comb, scale, count, *order(cpu), torch.as_tensor(gi))
    want.backward(torch.tensor(g_out))
    mag = {k: cpu[k].detach().abs().requires_grad_(k in dev) for k in shapes}
    m_out, m_zs = composed64(op, comb, scale, count, *order(mag), torch.as_tensor(gi), masks=[(z > 0).double() for z in zs])
    for z, m in zip(zs, m_zs):
        assert torch.all(z.detach().abs() > 4 * (d + ds + count + 2) * U * m.detach())
    (m_out * torch.tensor(np.abs(g_out))).sum().backward()
    terms = size * count + d + ds + f
    for k in names:
        assert torch.all((dev[k].grad.double().cpu() - cpu[k].grad).abs() <= 4 * (terms + 2) * U * mag[k].grad), k


def test_example_routes_agree():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "sage_mean_minibatch.py"),
                          "--nodes", "2000", "--batch", "64", "--steps", "2", "--composed"],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = run.stdout.decode()
    assert run.returncode == 0, text[-2000:]
    assert "routes agree within the bound" in text, text[-2000:]
