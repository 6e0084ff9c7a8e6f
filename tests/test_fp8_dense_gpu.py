"""ops.aggregate_dense over an Fp8Rows table (csrc/mp_dense_fp8.h) against the float64 reference of
aggregate_dense_ref.py on fp8_ref.dequantize(q, scale): exact on small integers times power-of-two scales (a wrong
block layout, permutation of W, tail, plan boundary or root kind is a wrong integer), today's gather_segment_reduce
under an identity weight, within the derived bound on real values, same bits, and gradients against float64."""
import numpy as np
import pytest
import torch

import fp8_ref
from aggregate_dense_ref import dense_ref
from test_aggregate_dense_gpu import DT, HUB, U, UNIT, composed64

pytestmark = pytest.mark.gpu

BASE = dict(dt="bf16", op="add", act="relu", combine="add", root="index", d=64, ds=64, f=64, fs=None, count=10, size=65,
            gather="int32", lens=None, out="f32", off=0, bias="f32", scale=None)
EXACT = {
    "base": {},
    **{"d%d" % d: dict(d=d) for d in (1, 15, 16, 17, 48, 63, 64, 65, 96, 128, 129, 144, 192)},
    **{"F%d" % f: dict(f=f) for f in (1, 16, 17, 33, 65, 130)},
    **{"count%d" % c: dict(count=c) for c in (1, 3, 17, 25)},
    **{"size%d" % s: dict(size=s) for s in (0, 1, 15, 16, 17, 257)},
    "seg": dict(lens=HUB),
    "gather-none": dict(gather=None), "gather-int32-bad": dict(gather="int32-bad"),
    "gather-int64-bad": dict(gather="int64-bad"),
    "mean": dict(op="mean", count=8), "none": dict(act="none"),
    "f32": dict(dt="f32"), "f16": dict(dt="f16"),
    "out-same": dict(out="same", bias=None),
    "no-root": dict(combine=None), "root-dense": dict(root="dense", ds=33), "root-index-bad": dict(root="index64-bad"),
    "concat": dict(combine="concat", fs=40), "fold": dict(combine="fold"),
    "fold-gin": dict(combine="fold", scale=3.0), "fold-mean": dict(combine="fold", op="mean", count=7),
    "fold-dense": dict(combine="fold", root="dense"),
    # NT 4 | 2 by the 64 KB of both paths' W, at d rounded up to 64: 256 | 272 -> 320
    "lds-d256-F40": dict(d=256, f=40, size=17), "lds-d272-F40": dict(d=272, f=40, size=17),
    # fp32, both paths 576 k: K is tiled by 512 and the waves run in lockstep
    "lock-f32-d576": dict(dt="f32", d=576, f=16, size=17),
    "off1": dict(off=1),
    # past the launcher's grid cap: 512 workgroups x 4 runs x 16 destinations, twice over
    "grid-cap": dict(d=16, f=16, count=1, size=65536 + 17),
}


def make(case, real=False, seed=0):
    """-> (positional args, keyword args for ops.aggregate_dense on the device, args for dense_ref)"""
    from euler_amd import ops
    c = dict(BASE, **case)
    rng = np.random.default_rng(seed)
    d, f, dt, comb = c["d"], c["f"], DT[c["dt"]], c["combine"]
    index = comb is not None and c["root"].startswith("index")
    ds, fs = d if comb == "fold" or index else c["ds"], None if comb == "fold" else c["fs"] or f
    seg = np.arange(c["size"] + 1) * c["count"] if c["lens"] is None else np.concatenate([[0], np.cumsum(c["lens"])])
    size, e = len(seg) - 1, int(seg[-1])
    rows = max(e, 1) if c["gather"] is None else 97
    dev = lambda a, t=dt: torch.as_tensor(a, dtype=t).cuda()
    if real:
        t8 = ops.Fp8Rows.quantize(dev(rng.standard_normal((rows, d)), torch.float32))
        q, col_scale = t8.q.cpu().numpy(), t8.scale.cpu().numpy()
        b, root = rng.standard_normal(f), rng.standard_normal((size, ds))
        w, ws = rng.standard_normal((d, f)) / np.sqrt(d), rng.standard_normal((ds, fs or 1)) / np.sqrt(ds)
    else:
        sparse = lambda k, n: rng.integers(-2, 3, (k, n)) * (rng.random((k, n)) < min(1.0, 6.0 / k))
        q = fp8_ref.enc(rng.integers(-2, 3, (rows, d)).astype(np.float32))
        col_scale = rng.choice(np.float32([0.5, 1, 2, 4]), d)
        b, root, w, ws = rng.integers(-2, 3, f), rng.integers(-2, 3, (size, ds)), sparse(d, f), sparse(ds, fs or 1)
        flat = torch.zeros(rows * d + 32, dtype=torch.uint8)
        flat[c["off"]:c["off"] + rows * d] = torch.as_tensor(q.reshape(-1))
        t8 = ops.Fp8Rows(flat.cuda()[c["off"]:c["off"] + rows * d].view(rows, d), dev(col_scale, torch.float32))
        assert t8.q.data_ptr() % 16 == c["off"]
    table = fp8_ref.dequantize(q, col_scale).astype(np.float64)
    b_t = None if c["bias"] is None else dev(b, torch.float32 if c["bias"] == "f32" else dt)
    stored = lambda t: None if t is None else t.double().cpu().numpy()
    root_t = ri = root_ref = None
    if index:
        ri = rng.integers(0, rows, size).astype(np.int64 if "64" in c["root"] else np.int32)
        if c["root"].endswith("bad"):
            ri[::3] = np.resize([-1, rows, 2 ** 40, 2 ** 32 + 3], len(ri[::3]))
        ok = (ri >= 0) & (ri < rows)
        root_ref = table[np.where(ok, ri, 0)] * ok[:, None]
        if comb != "fold":              # the self path's operand is x^ rounded once to the weight's dtype
            root_ref = torch.as_tensor(root_ref).to(dt).double().numpy()
    elif comb is not None:
        root_t = dev(root)
        root_ref = stored(root_t)
    ws_t = dev(ws) if comb in ("add", "concat") else None
    w_t = dev(w)
    gi = None
    if c["gather"] is not None:
        gi = rng.integers(0, rows, e).astype(np.int64 if c["gather"].startswith("int64") else np.int32)
        if c["gather"].endswith("bad"):
            bad = [-1, rows] + ([2 ** 40, 2 ** 32 + 3] if gi.dtype == np.int64 else [])
            gi[::3] = np.resize(bad, len(gi[::3]))
    kw = dict(root=root_t, root_index=None if ri is None else torch.as_tensor(ri).cuda(), root_weight=ws_t,
              combine=comb or "add", root_scale=c["scale"], bias=b_t, activation=c["act"],
              out_dtype=torch.float32 if c["out"] == "f32" else None)
    kw.update(dict(count=c["count"]) if c["lens"] is None else dict(seg_ptr=torch.as_tensor(seg).cuda()))
    ref = dict(root=root_ref, ws=stored(ws_t), combine=comb, scale=c["scale"])
    return ((c["op"], t8, w_t, None if gi is None else torch.as_tensor(gi).cuda(), size), kw,
            ((c["op"], table, stored(w_t), gi, seg, stored(b_t), c["act"], dt), ref))


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_integers(name):
    from euler_amd import ops
    args, kw, (ref_args, ref_kw) = make(EXACT[name])
    out = ops.aggregate_dense(*args, **kw)
    want = torch.as_tensor(dense_ref(*ref_args, **ref_kw)).to(out.dtype).double().numpy()
    assert out.shape == want.shape and out.dtype == (kw["out_dtype"] or args[2].dtype)
    got = out.double().cpu().numpy()
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, (name, len(wrong), wrong[:5], got[tuple(wrong[0])], want[tuple(wrong[0])])


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("op", ["mean", "add"])
def test_identity_weight_is_gather_segment_reduce(dt, op):
    """d == F, weight = I, no bias, no activation, no root: the fold and the narrowing are today's op"""
    from euler_amd import ops
    args, kw, _ = make(dict(dt=dt, op=op, combine=None), real=True, seed=4)
    _, t8, _, gi, size = args
    eye = torch.eye(BASE["d"], dtype=DT[dt], device="cuda")
    out = ops.aggregate_dense(op, t8, eye, gi, size, activation="none", count=BASE["count"])
    assert torch.equal(out, ops.gather_segment_reduce(op, t8, gi, size, count=BASE["count"], out_dtype=DT[dt]))


REAL = [dict(dt=dt, op=op, **shape) for dt in sorted(DT) for op in ("mean", "add")
        for shape in ({}, dict(d=130, f=130), dict(combine="concat", fs=24), dict(combine="fold", scale=1.5))]


@pytest.mark.parametrize("case", REAL, ids=lambda c: "-".join(str(v) for v in c.values()))
def test_real_values_within_bound(case):
    """The bound of test_aggregate_dense_gpu.py::test_real_values_within_bound as it stands, with UNIT of the
    weight's dtype: the reference reads the same x^ (one exact-to-fp32 multiply), so quantisation adds no term."""
    from euler_amd import ops
    c = dict(BASE, **case)
    args, kw, (ref_args, ref_kw) = make(case, real=True, seed=1)
    got = ops.aggregate_dense(*args, **kw).double().cpu().numpy()
    want = dense_ref(*ref_args, **ref_kw)
    op, table, w, gi, seg, b, _, _ = ref_args
    mag = dense_ref(op, np.abs(table), np.abs(w), gi, seg, np.abs(b), "none", None,
                    **{k: np.abs(v) if isinstance(v, np.ndarray) else v for k, v in ref_kw.items()})
    ds = 0 if c["combine"] == "fold" else c["d"]
    plain = ((c["count"] + 1) * U + (3 * U if op == "mean" else 0.0) + UNIT[c["dt"]]) * mag
    acc = (c["d"] + ds + 2) * U * mag
    err = np.abs(got - want)
    print("largest error / bound:", float(np.max(err / (4 * acc + plain))))
    assert np.all(err <= 4 * acc + plain)


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


@pytest.mark.parametrize("op,comb", [("mean", "add"), ("add", "fold")])
def test_gradients(op, comb, monkeypatch):
    """fp32 weight and root_index on the device against float64 autograd on the dequantised table: the check and
    the bound of test_aggregate_dense_gpu.py::test_gradients; the table and root_index receive no gradient."""
    from euler_amd import ops
    count, size, d, f, scale, rows = 4, 37, 24, 20, 1.5, 50
    monkeypatch.setattr(ops, "POOL_GRAD_CHUNK_ROWS", 10 * count)      # 37 destinations: four chunks
    rng = np.random.default_rng(3)
    gi, ri = rng.integers(0, rows, size * count), rng.integers(0, rows, size)
    gi[5], gi[17] = -1, 2 ** 40                 # (a root row of +0 would put pre-activations of 0 into the check below)
    t8 = ops.Fp8Rows.quantize(torch.tensor(rng.standard_normal((rows, d)), dtype=torch.float32, device="cuda"))
    table = torch.as_tensor(fp8_ref.dequantize(t8.q.cpu().numpy(), t8.scale.cpu().numpy())).double()
    root = table[torch.as_tensor(ri)]
    names = ["w", "b"] + (["ws"] if comb == "add" else [])
    vals = dict(w=rng.standard_normal((d, f)), b=rng.standard_normal(f), ws=rng.standard_normal((d, f)))
    g_out = rng.standard_normal((size, f))
    dev = {k: torch.tensor(vals[k], dtype=torch.float32, device="cuda", requires_grad=True) for k in names}
    ri_t = torch.as_tensor(ri).cuda()
    out = ops.aggregate_dense(op, t8, dev["w"], torch.as_tensor(gi).cuda(), size, root_index=ri_t, root_weight=dev.get("ws"),
                              combine=comb, root_scale=scale if comb == "fold" else None, bias=dev["b"], count=count)
    out.backward(torch.tensor(g_out, dtype=torch.float32, device="cuda"))
    assert ri_t.grad is None and t8.q.grad is None and t8.scale.grad is None
    cpu = {k: torch.tensor(dev[k].detach().cpu().numpy() if k in dev else vals[k], dtype=torch.float64,
                           requires_grad=k in dev) for k in vals}
    want, zs = composed64(op, comb, scale, count, table, cpu["w"], cpu["b"], root, cpu["ws"], torch.as_tensor(gi))
    want.backward(torch.tensor(g_out))
    mag = {k: cpu[k].detach().abs().requires_grad_(k in dev) for k in vals}
    m_out, m_zs = composed64(op, comb, scale, count, table.abs(), mag["w"], mag["b"], root.abs(), mag["ws"],
                             torch.as_tensor(gi), masks=[(z > 0).double() for z in zs])
    for z, m in zip(zs, m_zs):
        assert torch.all(z.detach().abs() > 4 * (2 * d + count + 2) * U * m.detach())
    (m_out * torch.tensor(np.abs(g_out))).sum().backward()
    terms = size * count + 2 * d + f
    for k in names:
        assert torch.all((dev[k].grad.double().cpu() - cpu[k].grad).abs() <= 4 * (terms + 2) * U * mag[k].grad), k
