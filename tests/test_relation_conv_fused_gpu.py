"""ops.relation_conv(route="fused") (csrc/mp_relation_dense.h) against relation_reduce_ref.reduce_dest, its bucket
rounded to the dtype through torch, then a float64 matmul: exact on small integers (a wrong fragment layout, tail,
plan boundary, skipped relation or predicated walk is a wrong integer), relation_reduce's bits under a one-hot
weight, within the derived bound on real values, same bits, the composed route's gradients, and no [size, R, F]
block."""
import numpy as np
import pytest
import torch

from relation_reduce_ref import reduce_dest

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}       # unit roundoff of the narrowing
U = 2.0 ** -24
HUB = [0, 1, 300, 0, 0, 1, 5, 16, 17, 0, 33, 2, 0]          # segment lengths of the seg_ptr cases

# types "mixed": random relations with -1 and R among them, relation R - 3 in no destination at all and relation 2
# in none of the first run of 16; "pow2": count * t // R ... every bucket and every destination a power of two
BASE = dict(dt="bf16", aggr="add", f=64, dim=48, r=8, count=10, size=65, gather="int32", lens=None, out="f32", off=0,
            types="mixed")
# one-axis sweeps around BASE (phased: 8 matrices of 64 columns x 144 bytes pass 64 KB); the plan boundaries are
# those of RelDenseMakePlan (mp_relation_dense.h)
EXACT = {
    "base": {},
    "f32": dict(dt="f32"), "f16": dict(dt="f16"),
    "mean": dict(aggr="mean", count=8, types="pow2"), "mean-f32": dict(aggr="mean", count=8, types="pow2", dt="f32"),
    "mean_rel": dict(aggr="mean_rel", count=8, types="pow2"), "mean_rel-f16-R2": dict(aggr="mean_rel", count=8, types="pow2", dt="f16", r=2),
    **{"F%d" % f: dict(f=f) for f in (1, 7, 8, 31, 32, 33, 128, 129, 256)},
    **{"F%d-f32" % f: dict(f=f, dt="f32", size=33) for f in (7, 33, 129)},
    **{"dim%d" % d: dict(dim=d) for d in (1, 15, 16, 17, 130, 256)},
    **{"R%d" % r: dict(r=r) for r in (1, 2, 8, 64)},
    # 129: one past a group of 4 waves x 2 runs x 16 (BASE's 65 is one past 4 x 1 x 16, the group of dim > 128)
    **{"size%d" % s: dict(size=s) for s in (0, 1, 15, 16, 17, 129, 257)},
    **{"count%d" % c: dict(count=c) for c in (1, 3, 16, 17, 25)},
    "seg": dict(lens=HUB), "seg-f32": dict(lens=HUB, dt="f32"), "seg-resident": dict(lens=HUB, r=3, f=32),
    "gather-none": dict(gather=None), "gather-int32-bad": dict(gather="int32-bad"), "gather-int64-bad": dict(gather="int64-bad"),
    "off4": dict(off=2), "off4-f32": dict(dt="f32", off=1),
    "out-bf16": dict(out="same"), "out-f16": dict(dt="f16", out="same"),
    # resident | phased: 16 columns x 80 bytes x R against 64 KB
    "res-R51": dict(f=32, dim=16, r=51, count=25), "pha-R52": dict(f=32, dim=16, r=52, count=25),
    # packed 16-bit columns: F = dim = 128, one 64 KB tile a relation
    "pha-128": dict(f=128, dim=128, size=130),
    # column tiles, fp32: 128 columns x 512 bytes fill the window; 160 x 400 at F = 96; two fold tiles at F = 256
    "ct-f32-dim128": dict(dt="f32", f=128, dim=128, size=33, count=5), "ct-f32-dim130": dict(dt="f32", f=128, dim=130, size=33, count=5),
    "ct-f32-F96": dict(dt="f32", f=96, dim=256, size=33, count=5), "ct-f32-F256": dict(dt="f32", f=256, dim=256, size=33, count=5, r=3),
    # past the launcher's grid cap: 512 workgroups x 8 runs x 16 destinations
    "grid-cap": dict(f=8, dim=16, r=2, count=1, size=65536 + 17),
}


def make(case, real=False, seed=0):
    """-> (args, kwargs of ops.relation_conv on the device, what reference() needs)"""
    c = dict(BASE, **case)
    rng = np.random.default_rng(seed)
    f, dim, r, dt = c["f"], c["dim"], c["r"], DT[c["dt"]]
    seg = np.arange(c["size"] + 1) * c["count"] if c["lens"] is None else np.concatenate([[0], np.cumsum(c["lens"])])
    size, e = len(seg) - 1, int(seg[-1])
    rows = max(e, 1) if c["gather"] is None else 97
    if real:
        x, w = rng.standard_normal((rows, f)), rng.standard_normal((r, dim, f)) / np.sqrt(f)
    else:
        x = rng.integers(-2, 3, (rows, f))
        w = rng.integers(-2, 3, (r, dim, f)) * (rng.random((r, dim, f)) < min(1.0, 6.0 / (r * f)))
    if c["types"] == "pow2":
        types = np.tile(np.arange(c["count"]) * r // c["count"], size)
    else:
        types = rng.integers(-1, r + 1, e)
        types[types == r - 3] = 0
        first = types[:seg[min(16, size)]]
        first[first == 2] = 1
    flat = torch.zeros(rows * f + 8, dtype=dt)
    flat[c["off"]:c["off"] + rows * f] = torch.as_tensor(x.reshape(-1), dtype=dt)
    x_t = flat.cuda()[c["off"]:c["off"] + rows * f].view(rows, f)
    w_t = torch.as_tensor(w, dtype=dt).cuda()
    gi, read = None, np.arange(e)
    if c["gather"] is not None:
        gi = rng.integers(0, rows, e).astype(np.int64 if c["gather"].startswith("int64") else np.int32)
        if c["gather"].endswith("bad"):
            bad = [-1, rows] + ([2 ** 40, 2 ** 32 + 3] if gi.dtype == np.int64 else [])
            gi[::3] = np.resize(bad, len(gi[::3]))
        read = np.minimum(gi.astype(np.int64) & 0xFFFFFFFF, rows - 1)             # relation_reduce's clamp
    kw = dict(aggr=c["aggr"], route="fused", out_dtype=torch.float32 if c["out"] == "f32" else None)
    kw.update(dict(count=c["count"]) if c["lens"] is None else dict(seg_ptr=torch.as_tensor(seg).cuda()))
    args = (x_t, w_t, None if gi is None else torch.as_tensor(gi).cuda(), torch.as_tensor(types, dtype=torch.int32).cuda(), size)
    return args, kw, (c["aggr"], x_t.float().cpu().numpy(), w_t.double().cpu().numpy(), read, types, seg, dt)


def reference(aggr, x, w, read, types, seg, dt):
    """float64 [size, dim]: the buckets of reduce_dest rounded to dt through torch, times the stored matrices"""
    h = np.zeros((len(seg) - 1,) + w.shape[::2], np.float32)
    for i in range(len(seg) - 1):
        p = slice(seg[i], seg[i + 1])
        h[i], _ = reduce_dest(aggr, x, read[p], types[p], w.shape[0])
    return np.einsum("rtf,tdf->rd", torch.as_tensor(h).to(dt).double().numpy(), w)


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_integers(name):
    from euler_amd import ops
    args, kw, ref = make(EXACT[name])
    out = ops.relation_conv(*args, **kw)
    want = torch.as_tensor(reference(*ref)).to(out.dtype).double().numpy()
    assert out.shape == want.shape and out.dtype == (kw["out_dtype"] or args[0].dtype)
    got = out.double().cpu().numpy()
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, (name, len(wrong), wrong[:5], got[tuple(wrong[0])], want[tuple(wrong[0])])


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("aggr", ["add", "mean", "mean_rel"])
def test_one_hot_weight_is_relation_reduce(dt, aggr):
    """dim == F, weight[t0] = I, the other matrices 0: the fold, the denominators and the narrowing are the bits
    the composed route stores"""
    from euler_amd import ops
    (x, w, gi, et, size), kw, _ = make(dict(dt=dt, aggr=aggr, dim=BASE["f"], out="same", count=7), real=True, seed=4)
    t0 = 1
    w = torch.zeros_like(w)
    w[t0] = torch.eye(BASE["f"], dtype=w.dtype, device="cuda")
    out = ops.relation_conv(x, w, gi, et, size, **kw)
    assert torch.equal(out, ops.relation_reduce(aggr, x, gi, et, BASE["r"], size, count=7)[:, t0, :])


REAL = [dict(dt=dt, aggr=aggr, **shape) for dt in sorted(DT) for aggr in ("add", "mean", "mean_rel")
        for shape in ({}, dict(f=130, dim=33, r=3), dict(f=32, dim=16, r=5))]


@pytest.mark.parametrize("case", REAL, ids=lambda c: "-".join(str(v) for v in c.values()))
def test_real_values_within_bound(case):
    """With M = the reference on absolute values without the narrowing (sum_t sum |x| |w|, divided as the mean
    divides): the fold's len roundings carry len 2^-24 M; the denominator fl(n + 1e-7f) and the division 3 x 2^-24
    M; the narrowing of a bucket one unit roundoff of x's dtype times M (none for fp32); the fp32 accumulation over
    R F products (R F + 2) 2^-24 M, x4 as for pool_aggregate and aggregate_dense: an MFMA's rounding is not
    documented; the output is fp32 here, so its rounding is inside the accumulation term."""
    from euler_amd import ops
    c = dict(BASE, **case)
    args, kw, ref = make(case, real=True, seed=1)
    got = ops.relation_conv(*args, **kw).double().cpu().numpy()
    aggr, x, w, read, types, seg, dt = ref
    want = reference(*ref)
    mag = reference(aggr, np.abs(x), np.abs(w), read, types, seg, torch.float32)
    bound = ((c["count"] + 3 + 4 * (c["r"] * c["f"] + 2)) * U + UNIT[c["dt"]]) * mag
    err = np.abs(got - want)
    print("max error / bound: %.3f" % float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)


@pytest.mark.parametrize("case", [{}, dict(dt="f32", aggr="mean", r=3, f=32)], ids=["phased", "resident"])
def test_same_bits(case):
    """count against the equivalent seg_ptr, and two calls on two streams"""
    from euler_amd import ops
    args, kw, ref = make(case, real=True, seed=2)
    a = ops.relation_conv(*args, **kw)
    seg = torch.as_tensor(ref[5]).cuda()
    assert torch.equal(a, ops.relation_conv(*args, **dict(kw, count=None, seg_ptr=seg)))
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(ops.relation_conv(*args, **kw))
        s.synchronize()
    assert torch.equal(outs[0], a) and torch.equal(outs[1], a)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_gradients_are_the_composed_routes(dt, aggr):
    from euler_amd import ops
    (x, w, gi, et, size), kw, _ = make(dict(dt=dt, aggr=aggr, out="same"), real=True, seed=3)
    assert bool(((et < 0) | (et >= BASE["r"])).any())
    grad = torch.randn(size, BASE["dim"], device="cuda", generator=torch.Generator("cuda").manual_seed(5)).to(x.dtype)
    got = []
    for route in ("fused", "composed"):
        xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
        ops.relation_conv(xr, wr, gi, et, size, **dict(kw, route=route)).backward(grad)
        got.append((xr.grad, wr.grad))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert bool(got[0][0].any()) and bool(got[0][1].any())


def test_block_is_not_allocated():
    """size 4096, R 8, F = dim 128, bf16, no gradients: the peak grows by less than the [size, R, F] block"""
    from euler_amd import ops
    size, r, f, count = 4096, 8, 128, 10
    g = torch.Generator("cuda").manual_seed(6)
    x = torch.randn(1000, f, device="cuda", generator=g).bfloat16()
    w = torch.randn(r, f, f, device="cuda", generator=g).bfloat16()
    gi = torch.randint(0, 1000, (size * count,), device="cuda", generator=g, dtype=torch.int32)
    et = torch.randint(0, r, (size * count,), device="cuda", generator=g, dtype=torch.int32)
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        out = ops.relation_conv(x, w, gi, et, size, count=count, route="fused")
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
    assert out.shape == (size, f) and grown < size * r * f * 2, grown
