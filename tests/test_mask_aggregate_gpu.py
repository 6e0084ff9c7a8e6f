"""ops.mask_aggregate / ops.mask_transpose (csrc/mp_mask.h) against the float64 reference of
mask_aggregate_ref.py: exact on small integers (a wrong byte, fragment layout, tail, block boundary or row
offset is a wrong integer), real values within the derived bound, the transpose against numpy, same bits,
gradients against float64 autograd, past the grid cap, and through Graph.sample_neighbor_layerwise."""
import numpy as np
import pytest
import torch

from mask_aggregate_ref import mask_aggregate_ref, pack, plan, plan_lib, unpack

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # unit roundoff of the output
OPS = ("add", "mean", "gcn", "gcn_renorm")
KB = {dt: plan(1 << 20, 128, dt == "f32")[2] for dt in DT}          # the candidate block
FT = 16 * plan(1 << 20, 1024, False)[0]                             # the column tile
BASE = dict(batch=2, n=33, m=130, d=24, density=0.1, fill=None, off=0, out=None)
# one-axis sweeps around BASE; m in units of the dtype's candidate block where a string
CASES = {
    "base": {},
    **{"m%s" % m: dict(m=m) for m in (1, 63, 64, 65, "KB", "KB+1", "2KB+33")},
    **{"n%d" % n: dict(n=n) for n in (1, 15, 17, 65, 129)},          # 65, 129: the tile of a 2- / 4-wave workgroup + 1
    **{"d%d" % d: dict(d=d) for d in (1, 7, 16, FT, FT + 1)},
    "batch1": dict(batch=1), "batch3": dict(batch=3),
    "zeros": dict(fill=0), "ones": dict(fill=1), "zero-word": dict(fill="gap", m=200),
    "off": dict(off=1), "off-d7": dict(off=1, d=7), "out-f32": dict(out=torch.float32),
}
THIN = ("base", "m1", "mKB+1", "m2KB+33", "n129", "d%d" % (FT + 1), "batch3", "off")


def make(case, dt, real=False, seed=0):
    """-> (device mask, x, root, batch, n, m, out_dtype); stray bits SET beyond m; views `off` elements / words off"""
    c = dict(BASE, **case)
    rng = np.random.default_rng(seed)
    m = c["m"] if not isinstance(c["m"], str) else {"KB": KB[dt], "KB+1": KB[dt] + 1, "2KB+33": 2 * KB[dt] + 33}[c["m"]]
    batch, n, d, off = c["batch"], c["n"], c["d"], c["off"]
    bits = rng.random((batch * n, (m + 63) // 64 * 64)) < c["density"]
    if c["fill"] in (0, 1):
        bits[:] = bool(c["fill"])
    elif c["fill"] == "gap":                                          # full rows around one all-zero word
        bits[:] = True
        bits[:, 64:128] = False
    bits[:, m:] = True                                                # the stray bits
    words = pack(bits).reshape(-1)
    mask = torch.as_tensor(np.concatenate([np.zeros(off, np.int64), words])).cuda()[off:].view(batch * n, -1)
    val = (lambda *s: rng.standard_normal(s)) if real else (lambda *s: rng.integers(-8, 9, s))
    rows = batch * m + 2                                              # (rows past batch * m are never read)
    flat = torch.zeros(rows * d + 8, dtype=DT[dt])
    flat[off:off + rows * d] = torch.as_tensor(val(rows * d), dtype=DT[dt])
    x = flat.cuda()[off:off + rows * d].view(rows, d)
    root = torch.as_tensor(val(batch * n, d), dtype=DT[dt]).cuda()
    return mask, x, root, batch, n, m, c["out"]


def run(op, mask, x, root, batch, n, m, out_dtype, **kw):
    from euler_amd import ops
    return ops.mask_aggregate(op, mask, x, batch, n, m, root=root if op.startswith("gcn") else None,
                              out_dtype=out_dtype, **kw)


def ref(op, mask, x, root, batch, n, m, dtype=np.float64):
    return mask_aggregate_ref(op, mask.cpu().numpy(), x.double().cpu().numpy(),
                              root.double().cpu().numpy() if op.startswith("gcn") else None, batch, n, m, dtype)


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_integers(name, dt):
    args = make(CASES[name], dt)
    for op in OPS:
        out, deg = run(op, *args, return_degree=True)
        want, want_deg, _ = ref(op, *args[:6], dtype=np.float32)
        assert out.dtype == (args[6] or DT[dt]) and out.shape == want.shape
        assert torch.equal(out.cpu(), torch.as_tensor(want).to(out.dtype)), (name, dt, op)
        assert torch.equal(deg.cpu(), torch.as_tensor(want_deg)), (name, dt, op)


def bound(want, deg, mag, op, unit):
    """4 * (deg + 2) * 2^-24 * (|root| + sum |x_c|) / denom, plus one unit of the output dtype on the result"""
    denom = {"add": np.ones_like(deg), "gcn_renorm": 1.0 + deg}.get(op, np.maximum(deg, 1e-7)).reshape(-1, 1)
    return 4 * (deg.reshape(-1, 1) + 2) * 2.0 ** -24 * mag / denom + unit * np.abs(want)


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("name", THIN)
def test_real_values_within_bound(name, dt):
    args = make(CASES[name], dt, real=True, seed=1)
    worst = 0.0
    for op in OPS:
        out = run(op, *args)
        want, deg, mag = ref(op, *args[:6])
        err, lim = np.abs(out.double().cpu().numpy() - want), bound(want, deg, mag, op, UNIT[out.dtype])
        worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        assert (err <= lim).all(), (name, dt, op, worst)
    print("mask_aggregate %s %s: largest error / bound = %.3f" % (name, dt, worst))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n,m", [(1, 1), (64, 64), (65, 63), (130, 257)])
def test_mask_transpose(n, m, batch):
    from euler_amd import ops
    mask = make(dict(batch=batch, n=n, m=m, density=0.3), "f32")[0]
    want = unpack(mask.cpu().numpy(), m).reshape(batch, n, m)
    got = ops.mask_transpose(mask, batch, n, m)
    assert torch.equal(got.cpu(), torch.as_tensor(pack(want.transpose(0, 2, 1).reshape(batch * m, n))))
    assert torch.equal(ops.mask_transpose(got, batch, m, n).cpu(), torch.as_tensor(pack(want.reshape(batch * n, m))))


@pytest.mark.parametrize("dt", sorted(DT))
def test_same_bits(dt):
    mask, x, root, batch, n, m, _ = make(dict(m=2 * KB[dt] + 33, n=129), dt, real=True, seed=2)
    for op in OPS:
        first = run(op, mask, x, root, batch, n, m, None)
        with torch.cuda.stream(torch.cuda.Stream()):
            other = run(op, mask, x, root, batch, n, m, None)
        torch.cuda.synchronize()
        halves = [run(op, mask[b * n:(b + 1) * n], x[b * m:], root[b * n:(b + 1) * n], 1, n, m, None) for b in range(batch)]
        same = lambda a, b: torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        assert same(first, other) and same(first, torch.cat(halves))


@pytest.mark.parametrize("shape", [(2, 33, 130, 24), (1, 17, 65, FT + 1)])
@pytest.mark.parametrize("op", OPS)
def test_gradients(op, shape):
    batch, n, m, d = shape
    mask, x, root, _, _, _, _ = make(dict(batch=batch, n=n, m=m, d=d), "f32", real=True, seed=3)
    grad = torch.randn(batch * n, d, device="cuda")
    x, root = x.clone().requires_grad_(True), root.clone().requires_grad_(True)
    run(op, mask, x, root, batch, n, m, None).backward(grad)
    # float64 autograd through the dense formulation
    bits = torch.as_tensor(unpack(mask.cpu().numpy(), m).reshape(batch, n, m)).double()
    x64, r64 = x.detach().double().cpu().requires_grad_(True), root.detach().double().cpu().requires_grad_(True)
    s = (bits @ x64[:batch * m].reshape(batch, m, d)).reshape(batch * n, d)
    deg = bits.sum(2).reshape(-1, 1)
    lo = deg.clamp_min(1e-7)
    out = {"add": s, "mean": s / lo, "gcn": r64 + s / lo, "gcn_renorm": (r64 + s) / (1 + deg)}[op]
    out.backward(grad.double().cpu())
    # d_x[b, c] = sum over the sources i of candidate c of grad[i] / denom[i]: the forward's bound with n for deg
    denom = {"add": torch.ones_like(deg), "gcn_renorm": 1 + deg}.get(op, lo)
    mag = (bits.transpose(1, 2) @ (grad.double().cpu() / denom).abs().reshape(batch, n, d)).reshape(batch * m, d)
    err = (x.grad.double().cpu() - x64.grad)[:batch * m].abs()
    assert (err <= 4 * (n + 2) * 2.0 ** -24 * mag + 2.0 ** -24 * x64.grad[:batch * m].abs()).all(), float(err.max())
    assert torch.equal(x.grad[batch * m:].cpu(), torch.zeros(2, d))
    if op.startswith("gcn"):
        assert torch.allclose(root.grad.double().cpu(), r64.grad, rtol=2.0 ** -22, atol=0)
    else:
        assert root.grad is None


def test_past_the_grid_cap():
    """source tiles exceed the launcher's cap by one tile"""
    lib = plan_lib()
    n = lib.mask_max_blocks() * lib.mask_tile(1, 1 << 30, 1) + 1
    args = make(dict(batch=1, n=n, m=64, d=8, density=0.05), "bf16")
    for op in ("add", "gcn_renorm"):
        want = ref(op, *args[:6], dtype=np.float32)[0]
        assert torch.equal(run(op, *args).cpu(), torch.as_tensor(want).to(torch.bfloat16))


def test_through_the_graph():
    """adj_format="mask": the default format's neighbours, and an adjacency that aggregates to what its COO indices say"""
    import euler_amd
    from euler_amd import ops
    rng = np.random.default_rng(5)
    src, dst = rng.integers(1, 301, 4000), rng.integers(1, 301, 4000)
    g = euler_amd.Graph.from_edges(torch.as_tensor(src).cuda(), torch.as_tensor(dst).cuda())
    batch, n, m, d = 3, 20, 70, 8
    nodes = torch.as_tensor(rng.integers(1, 301, (batch, n))).cuda()
    g.set_seed(11)
    nb_coo, (ind, val, _shape) = g.sample_neighbor_layerwise(nodes, [0], m, call_id=4)
    nb, mask = g.sample_neighbor_layerwise(nodes, [0], m, call_id=4, adj_format="mask")
    assert torch.equal(nb, nb_coo) and mask.shape == (batch * n, 2)
    x = torch.as_tensor(rng.integers(-8, 9, (batch * m, d)), dtype=torch.float32).cuda()
    ind, val = ind.cpu().numpy(), val.cpu().numpy()
    dense = np.zeros((batch, n, m))
    dense[tuple(ind[val != 0].T)] = 1                                 # (the explicit zero entry at the corner left out)
    want = np.einsum("bnm,bmd->bnd", dense, x.double().cpu().numpy().reshape(batch, m, d)).reshape(batch * n, d)
    assert dense.sum() > 0
    assert torch.equal(ops.mask_aggregate("add", mask, x, batch, n, m).cpu(), torch.as_tensor(want, dtype=torch.float32))
