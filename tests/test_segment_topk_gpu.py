"""ops.gather_segment_topk on the GPU against the numpy restatement tests/segment_topk_ref.py: a
top-k is a pure selection, so values, selected positions and the per-edge gradient are compared
BIT FOR BIT (a NaN must be a NaN).  Shapes are the smallest at which each path of the kernel runs:
every chunk width with tails, every template capacity, more than one block, all segment forms."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import segment_topk_ref as ref

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 4, 8, 12, 64, 130, 260]
SIZES = [0, 1, 63, 64, 65, 257]
COUNTS = [1, 2, 3, 10, 17]
KS = [1, 2, 3, 4, 8, 16]               # every template capacity, and 3 between two of them
ROWS = 50


@pytest.fixture(scope="module")
def torch(torch_cuda):
    return torch_cuda


@pytest.fixture(scope="module")
def ops(EA):
    from euler_amd import ops
    return ops


def TDT(torch, dt):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dt]


def to_dev(torch, a, dt, misalign=False):
    """a stored numpy array on the device; misalign: a view that starts 4 bytes into its allocation"""
    t = torch.from_numpy(np.ascontiguousarray(a) if dt == "f32" else np.ascontiguousarray(a).view(np.int16))
    t = t.cuda() if dt == "f32" else t.cuda().view(TDT(torch, dt))
    if not misalign:
        return t
    pad = 1 if dt == "f32" else 2
    buf = torch.empty(t.numel() + pad, dtype=t.dtype, device="cuda")
    view = buf[pad:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def to_host(t):
    import torch
    t = t.detach().cpu().contiguous()
    return t.numpy() if t.dtype in (torch.float32, torch.int32) else t.view(torch.int16).numpy().view(np.uint16)


def draw_gather(rng, kind, e, rows):
    if kind == "none":
        return None
    g = rng.integers(0, rows, e)
    if kind == "i32":
        return g.astype(np.int32)
    g = g.astype(np.int64)
    bad = np.array([-1, rows, 2 ** 40], np.int64)       # ids that name no row
    g[1::4] = np.resize(bad, len(g[1::4]))
    return g


def plan():
    """The calls of the parity test for one d: SIZES x KS, the other dimensions rotating with
    periods chosen so that every value (and the pairs asserted in check_plan_covers) occurs."""
    calls = []
    for n in range(len(SIZES) * len(KS)):
        i, j = divmod(n, len(KS))
        dt = ref.DTYPES[(i + j) % 3]
        calls.append(dict(size=SIZES[i], k=KS[j], dt=dt, out_dt="f32" if (n // 2) % 2 else dt,
                          fill=-1e9 if (n // 3) % 2 else 0.0, kind=("i32", "ids", "none")[(n + n // 3) % 3],
                          ragged=bool((n + n // 2) % 2), count=COUNTS[n % 5], misalign=n % 4 == 1))
    return calls


def check_plan_covers():
    calls = plan()
    uniform = [c for c in calls if not c["ragged"] and c["size"] > 0]
    assert {c["count"] for c in uniform} == set(COUNTS)
    assert {(c["kind"], c["ragged"]) for c in calls if c["size"] > 1} == {
        (a, b) for a in ("i32", "ids", "none") for b in (False, True)}
    assert {(c["dt"], c["out_dt"]) for c in calls} == {(a, a) for a in ref.DTYPES} | {("bf16", "f32"), ("f16", "f32")}
    assert {(c["k"], c["dt"]) for c in calls} == {(k, a) for k in KS for a in ref.DTYPES}
    assert {c["fill"] for c in calls} == {0.0, -1e9}
    assert {(c["misalign"], c["dt"]) for c in calls if c["size"] > 1} >= {(True, a) for a in ref.DTYPES}


@pytest.mark.parametrize("d", DIMS)
def test_values_and_positions_equal_the_restatement(torch, ops, d):
    """every call of plan() at this d: values and positions with return_indices, and the values of
    the kernels that track no positions"""
    check_plan_covers()
    rng = np.random.default_rng(500 + d)
    longest = 0
    for c in plan():
        size, k, dt, out_dt = c["size"], c["k"], c["dt"], c["out_dt"]
        if c["ragged"]:
            seg_ptr, count = ref.ragged_ptr(rng, size), None
            e = int(seg_ptr[-1]) + 5                    # seg_ptr[0] > 0 and seg_ptr[-1] < e
            longest = max(longest, int((seg_ptr[1:] - seg_ptr[:-1]).max(initial=0)))
        else:
            seg_ptr, count = None, c["count"]
            e = size * count
        # without a gather array position p reads row p: the ragged form then covers the table's rows
        rows = e if c["kind"] == "none" and c["ragged"] else ROWS
        params = ref.tie_table(rng, (rows, d), dt)
        g = draw_gather(rng, c["kind"], e, rows)
        want, want_sel = ref.topk(params, dt, g, size, k, seg_ptr=seg_ptr, count=count, fill=c["fill"],
                                  out_dt=out_dt, e=e)
        tp = to_dev(torch, params, dt, c["misalign"])
        tg = None if g is None else torch.from_numpy(g).cuda()
        tsp = None if seg_ptr is None else torch.from_numpy(seg_ptr).cuda()
        kw = dict(seg_ptr=tsp, count=count, fill=c["fill"], out_dtype=torch.float32 if out_dt == "f32" else None)
        got, sel = ops.gather_segment_topk(tp, tg, size, k, return_indices=True, **kw)
        tag = (d, sorted(c.items()))
        assert got.shape == (size, k, d) and got.dtype == TDT(torch, out_dt) and sel.dtype == torch.int32, tag
        assert ref.same(to_host(got), want, out_dt), tag
        assert np.array_equal(to_host(sel), want_sel), tag
        plain = ops.gather_segment_topk(tp, tg, size, k, **kw)
        assert ref.same(to_host(plain), want, out_dt), tag
    assert longest == 40


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_equals_torch_topk_and_autograd_on_distinct_values(torch, ops, dt):
    """distinct finite values: out == torch.topk of the composition; with every table row used by
    one edge at most (a permutation as the gather array) the table gradient is autograd's, bit for
    bit"""
    rng = np.random.default_rng(9)
    b, nb, d, k = 65, 10, 12, 3
    rows = b * nb + 7
    # distinct within every column and exact in bf16: 2^q * (1 + m / 128) from a permutation per column
    cols = np.stack([rng.permutation(rows) for _ in range(d)], 1)
    vals = (2.0 ** (cols // 128 - 4) * (1 + (cols % 128) / 128) * np.where(cols % 2, 1, -1)).astype(np.float32)
    table = torch.from_numpy(vals).cuda().to(TDT(torch, dt))
    assert torch.equal(table.float().cpu(), torch.from_numpy(vals))
    gi = torch.from_numpy(rng.permutation(rows)[:b * nb].astype(np.int64)).cuda()
    w = torch.from_numpy(rng.standard_normal((b, k, d)).astype(np.float32)).cuda()
    p1 = table.clone().requires_grad_(True)
    out = ops.gather_segment_topk(p1, gi, b, k, count=nb)
    (out.float() * w).sum().backward()
    p2 = table.clone().requires_grad_(True)
    want = torch.topk(p2[gi].view(b, nb, d), k, dim=1).values
    (want.float() * w).sum().backward()
    bits = torch.int32 if dt == "f32" else torch.int16
    assert torch.equal(out, want)
    assert torch.equal(p1.grad.view(bits), p2.grad.view(bits))
    assert int((p1.grad != 0).sum()) == b * k * d


@pytest.mark.parametrize("form", ["count", "ragged", "none"])
def test_gradient_equals_the_restatement(torch, ops, form):
    """per-edge block == the restatement; table gradient == scatter_add of that block; rows named
    only by ids outside the table get nothing; positions outside every segment are +0; grad is
    accepted in 16 bits"""
    rng = np.random.default_rng({"count": 1, "ragged": 2, "none": 3}[form])
    size, d, k, rows = 65, 12, 3, 40
    for dt, gdt in (("f32", "f32"), ("bf16", "f32"), ("f16", "f16"), ("bf16", "bf16")):
        params = ref.tie_table(rng, (rows, d), dt)
        if form == "count":
            seg_ptr, count, e = None, 10, size * 10
        else:
            seg_ptr, count = ref.ragged_ptr(rng, size), None
            e = int(seg_ptr[-1]) + 5
        if form == "none":
            g, e = None, rows                               # (segments past the table are cut at e)
        elif form == "ragged":
            g = rng.integers(-1, rows + 1, e).astype(np.int32)
        else:
            g = rng.integers(0, rows, e).astype(np.int64)
            g[g == 5] = 6                                   # row 5: named only by ids outside the table
            g[2::7] = np.resize(np.array([2 ** 40 + 5, -1, rows, 2 ** 32 + 5], np.int64), len(g[2::7]))
        _, want_sel = ref.topk(params, dt, g, size, k, seg_ptr=seg_ptr, count=count, e=e)
        grad = ref.narrow(rng.standard_normal((size, k, d)).astype(np.float32), gdt)
        want_pe = ref.per_edge(ref.widen(grad, gdt), want_sel, e)
        tp = to_dev(torch, params, dt).requires_grad_(True)
        tg = None if g is None else torch.from_numpy(g).cuda()
        tsp = None if seg_ptr is None else torch.from_numpy(seg_ptr).cuda()
        out, sel = ops.gather_segment_topk(tp, tg, size, k, seg_ptr=tsp, count=count, return_indices=True,
                                           out_dtype=torch.float32 if gdt == "f32" else None)
        assert np.array_equal(to_host(sel), want_sel) and not sel.requires_grad
        tgrad = to_dev(torch, grad, gdt)
        pe = ops._segment_topk_grad_raw(tgrad, sel, e)
        assert ref.same(to_host(pe), want_pe, "f32"), (form, dt, gdt)
        if form == "ragged":
            lo, hi = int(seg_ptr[0]), int(seg_ptr[-1])
            assert lo > 0 and hi < e and not to_host(pe)[:lo].view(np.uint32).any()
            assert not to_host(pe)[hi:].view(np.uint32).any()
        out.backward(tgrad)
        keys = torch.arange(e, device="cuda") if tg is None else tg.to(torch.int64)
        keys = torch.where((keys >= 0) & (keys < rows), keys, torch.full_like(keys, -1))
        want_grad = ops.scatter_add(pe, keys, rows)
        assert ref.same(to_host(tp.grad), to_host(want_grad.to(TDT(torch, dt))), dt), (form, dt, gdt)
        # (scatter_add adds in input order from +0: the restatement's sequential loop)
        assert ref.same(to_host(want_grad), ref.table_grad(want_pe, g, rows), "f32"), (form, dt, gdt)
        if form == "count":
            assert not to_host(tp.grad.float())[5].view(np.uint32).any()
            assert to_host(tp.grad.float()).view(np.uint32).any()


def test_c_abi_guard_rows_and_einval(torch, ops):
    """through ctypes: out, sel and per_edge sit between guard rows that must stay untouched; every
    EINVAL case returns the code and writes nothing"""
    from euler_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(4)
    size, count, d, k, rows, guard = 65, 3, 12, 3, 30, 2
    e = size * count
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def p(t, off=0):
        return None if t is None else C.c_void_p(t.data_ptr() + off)

    for dt in ref.DTYPES:
        params = ref.tie_table(rng, (rows, d), dt)
        g = rng.integers(-1, rows + 1, e).astype(np.int64)
        want, want_sel = ref.topk(params, dt, g, size, k, count=count)
        tp, tg = to_dev(torch, params, dt), torch.from_numpy(g).cuda()
        esz = 4 if dt == "f32" else 2
        out = torch.full((size * k + 2 * guard, d), 7.0, dtype=TDT(torch, dt), device="cuda")
        sel = torch.full((size * k + 2 * guard, d), -7, dtype=torch.int32, device="cuda")
        pe = torch.full((e + 2 * guard, d), 7.0, device="cuda")
        grad = torch.from_numpy(rng.standard_normal((size, k, d)).astype(np.float32)).cuda()
        out0, sel0, pe0 = out.clone(), sel.clone(), pe.clone()

        def fwd(k=k, in_dt=ref.DTYPES.index(dt), out_dt=None,
                seg=None, count=count, e=e, params=tp, outp=out):
            out_dt = in_dt if out_dt is None else out_dt
            return L.euler_gpu_gather_segment_topk(st, p(params), in_dt, rows, p(tg), 1, p(seg), count, e, d, size, k,
                                                   0.0, p(outp, guard * d * esz), out_dt, p(sel, guard * d * 4))

        def bwd(k=k, gdt=0, g=grad, s=sel, pep=pe):
            return L.euler_gpu_segment_topk_grad(st, p(g), gdt, p(s, guard * d * 4) if s is not None else None, e, d,
                                                 size, k, p(pep, guard * d * 4))
        sp = torch.zeros(size + 1, dtype=torch.int64, device="cuda")
        bad = [fwd(k=0), fwd(k=17), fwd(e=e - 1), fwd(in_dt=3), fwd(out_dt=3), fwd(seg=sp), fwd(count=0),
               fwd(params=None), fwd(outp=None), bwd(k=0), bwd(k=17), bwd(gdt=3), bwd(g=None), bwd(s=None),
               bwd(pep=None)]
        if dt != "f32":
            bad.append(fwd(out_dt=3 - ref.DTYPES.index(dt)))          # the other 16-bit type
        torch.cuda.synchronize()
        assert all(rc == _lib.EINVAL for rc in bad), bad
        assert torch.equal(out.view(torch.int16), out0.view(torch.int16)) and torch.equal(sel, sel0)
        assert torch.equal(pe, pe0)
        assert fwd() == 0 and bwd() == 0
        torch.cuda.synchronize()
        body = slice(guard, guard + size * k)
        assert ref.same(to_host(out[body]).reshape(size, k, d), want, dt)
        assert np.array_equal(to_host(sel[body]).reshape(size, k, d), want_sel)
        assert ref.same(to_host(pe[guard:guard + e]), ref.per_edge(to_host(grad), want_sel, e), "f32")
        for t, t0 in ((out, out0), (sel, sel0), (pe, pe0)):
            assert torch.equal(t[:guard], t0[:guard]) and torch.equal(t[-guard:], t0[-guard:])


def test_two_runs_give_the_same_bits_on_any_stream(torch, ops):
    """determinism, and the op runs on the caller's (non-default) stream"""
    rng = np.random.default_rng(6)
    size, count, d, k = 257, 10, 64, 3
    params = ref.tie_table(rng, (ROWS, d), "f32")
    g = rng.integers(-1, ROWS + 1, size * count).astype(np.int64)
    want, want_sel = ref.topk(params, "f32", g, size, k, count=count)
    tp, tg = to_dev(torch, params, "f32"), torch.from_numpy(g).cuda()
    grad = torch.from_numpy(rng.standard_normal((size, k, d)).astype(np.float32)).cuda()

    def run():
        t = tp.clone().requires_grad_(True)
        out, sel = ops.gather_segment_topk(t, tg, size, k, count=count, return_indices=True)
        out.backward(grad)
        return out.detach(), sel, t.grad
    a = run()
    b = run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = run()
    s.synchronize()
    torch.cuda.synchronize()
    assert ref.same(to_host(a[0]), want, "f32") and np.array_equal(to_host(a[1]), want_sel)
    for other in (b, c):
        for x, y in zip(a, other):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_argument_errors(torch, ops):
    t = torch.zeros((4, 4), device="cuda")
    g = torch.zeros(6, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ops.gather_segment_topk(t, g, 2, 0, count=3)
    with pytest.raises(ValueError):
        ops.gather_segment_topk(t, g, 2, 17, count=3)
    with pytest.raises(ValueError):
        ops.gather_segment_topk(t, g, 2, 2)
    with pytest.raises(ValueError):
        ops.gather_segment_topk(t, g, 2, 2, count=2)
    with pytest.raises(TypeError):
        ops.gather_segment_topk(t.double(), g, 2, 2, count=3)
    with pytest.raises(TypeError):
        ops.gather_segment_topk(t.half(), g, 2, 2, count=3, out_dtype=torch.bfloat16)
    with pytest.raises(IndexError):
        ops.gather_segment_topk(t, g + 4, 2, 2, count=3, validate=True)
    # tensors in host memory are refused before any launch, whichever arguments are given
    with pytest.raises(RuntimeError):
        ops.gather_segment_topk(t.cpu(), None, 2, 2, count=2)
    with pytest.raises(RuntimeError):
        ops.gather_segment_topk(t.cpu(), g, 2, 2, count=3)
    with pytest.raises(RuntimeError):
        ops.gather_segment_topk(t, g.cpu(), 2, 2, count=3)
    with pytest.raises(RuntimeError):
        ops.gather_segment_topk(t, None, 2, 2, seg_ptr=torch.tensor([0, 2, 4]))
    empty = ops.gather_segment_topk(t[:, :0], g, 2, 2, count=3)
    assert empty.shape == (2, 2, 0)


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "lgcn_minibatch.py"), "--steps", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [float(line.split("loss")[1]) for line in r.stdout.splitlines() if "loss" in line]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout
