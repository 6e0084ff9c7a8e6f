"""Edge-weighted message passing: gather_scatter / gather_segment_reduce with edge_weight, and
edge_dot.

Contract (include/euler_gpu.h, DESIGN):
A. forward - fp32: the bits of scatter_(op, gather(x, gi) * w_expanded, si, n) (torch's fp32
   multiply, the existing ops); storage dtype S: f_S(x, w, out_dtype=fp32) has the bits of
   f_fp32(x.float(), w.float()), f_S(..., out_dtype=S) those bits after .to(S).
B. grad_params has the bits of the composition's gradient under torch autograd.
C. edge_dot and grad_edge_weight lie within gamma * sum_c |a_c b_c| of the float64 dot product of
   the widened inputs, gamma = dh u / (1 - dh u), u = 2^-24 - the bound of ANY summation order of
   dh correctly rounded fp32 products (derived, so no margin) - plus half an ulp of a 16-bit
   output type at the reference value; two identical calls are bit-equal; dh = 1 is the product.
Inputs are finite with |x| <= 4."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from test_half_mp_gpu import DIMS
import weighted_mp_ref as ref

pytestmark = pytest.mark.gpu

MODES = ["add", "max", "mean"]
HEADS = [1, 2, 8]
U = 2.0 ** -24


def _dtypes(torch):
    return [torch.float32, torch.bfloat16, torch.float16]


def bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same(got, want):
    import torch
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got), bits(want))


def draw(torch, gen, shape, S, unaligned=False, scale=8.0):
    """values of dtype S in [-scale / 2, scale / 2]; unaligned: a contiguous view that starts one
    element into its storage (aligned to the element, not to 16 bytes)"""
    x = ((torch.rand(shape, generator=gen, device="cuda") - 0.5) * scale).to(S)
    if unaligned:
        buf = torch.empty(x.numel() + 1, dtype=S, device="cuda")
        buf[1:] = x.reshape(-1)
        x = buf[1:].view(shape)
        assert x.data_ptr() % 16 == x.element_size() and x.is_contiguous()
    return x


def expand(w, d):
    w2 = w.reshape(w.shape[0], -1)
    return w2.repeat_interleave(d // w2.shape[1], dim=1)


@pytest.fixture(scope="module")
def gen(torch_cuda):
    g = torch_cuda.Generator(device="cuda")
    g.manual_seed(4321)
    return g


def composition(ops, op, x, gi, si, size, w):
    """the five-pass form, fp32 only"""
    msg = ops.gather(x, gi) if gi is not None else x
    return ops.scatter_(op, msg * expand(w, x.shape[1]), si, size)


def check_forward(torch, fused, composed, x, w, S):
    """fused(x, w, out_dtype); composed(x32, w32) or None (then only the storage contract)"""
    if S == torch.float32:
        assert same(fused(x, w, None), composed(x, w))
        return
    want32 = fused(x.float(), w.float(), None)
    if composed is not None:
        assert same(want32, composed(x.float(), w.float()))
    assert same(fused(x, w, torch.float32), want32), "out fp32"
    gotS = fused(x, w, S)
    assert same(gotS, want32.to(S)), "out S"
    assert same(fused(x, w, None), gotS)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_forward_meets_contract_a(EA, torch_cuda, gen, which, d):
    torch = torch_cuda
    S = _dtypes(torch)[which]
    ops = EA.ops
    rows, size, count = 300, 90, 10
    e = size * count
    gi = torch.randint(0, rows, (e,), generator=gen, device="cuda", dtype=torch.int32)
    si = torch.randint(0, size + 5, (e,), generator=gen, device="cuda", dtype=torch.int32)   # some keys >= size
    si[(si % 7) == 3] += 1                                   # destinations 3, 10, 17, ... stay empty
    si_sorted = torch.sort(si).values
    lens = torch.randint(0, 23, (size,), generator=gen, device="cuda")
    lens[::9] = 0
    seg_ptr = torch.zeros(size + 1, dtype=torch.int64, device="cuda")
    seg_ptr[1:] = torch.cumsum(lens, 0)
    ep = int(seg_ptr[-1])
    gp = torch.randint(0, rows, (ep,), generator=gen, device="cuda", dtype=torch.int32)
    ids = torch.randint(0, rows + 40, (e,), generator=gen, device="cuda", dtype=torch.int64)
    ids[::13] = -1                                           # default_node: reads the last row
    ids[5::17] += 1 << 33                                    # only the low word counts
    ids_rows = torch.clamp(ids & 0xFFFFFFFF, max=rows - 1).to(torch.int32)
    dst_count = torch.arange(size, device="cuda", dtype=torch.int32).repeat_interleave(count)
    dst_ptr = torch.repeat_interleave(torch.arange(size, device="cuda", dtype=torch.int32), lens)
    tested = 0
    for H in HEADS:
        if d % H:
            continue
        tested += 1
        for unaligned in (False, True):
            x = draw(torch, gen, (rows, d), S, unaligned)
            for WS in {torch.float32, S}:
                w = draw(torch, gen, (e, H), WS, scale=4.0)
                wp = draw(torch, gen, (ep, H), WS, unaligned, scale=4.0)
                for op in MODES:
                    for keys in (si, si_sorted):
                        check_forward(torch,
                                      lambda t, ww, od: ops.gather_scatter(op, t, gi, keys, size, out_dtype=od,
                                                                           edge_weight=ww),
                                      lambda t, ww: composition(ops, op, t, gi, keys, size, ww), x, w, S)
                    # the segment forms against gather_scatter with the explicit destinations
                    check_forward(torch,
                                  lambda t, ww, od: ops.gather_segment_reduce(op, t, gi, size, count=count,
                                                                              out_dtype=od, edge_weight=ww),
                                  lambda t, ww: ops.gather_scatter(op, t, gi, dst_count, size, edge_weight=ww),
                                  x, w, S)
                    check_forward(torch,
                                  lambda t, ww, od: ops.gather_segment_reduce(op, t, gp, size, seg_ptr=seg_ptr,
                                                                              out_dtype=od, edge_weight=ww),
                                  lambda t, ww: ops.gather_scatter(op, t, gp, dst_ptr, size, edge_weight=ww),
                                  x, wp, S)
                    check_forward(torch,
                                  lambda t, ww, od: ops.gather_segment_reduce(op, t, ids, size, count=count,
                                                                              out_dtype=od, edge_weight=ww),
                                  lambda t, ww: ops.gather_scatter(op, t, ids_rows, dst_count, size,
                                                                   edge_weight=ww), x, w, S)
        if H == 1:       # [E] and [E, 1] are the same weights
            w1 = draw(torch, gen, (e,), torch.float32, scale=4.0)
            assert same(ops.gather_scatter("add", x, gi, si, size, edge_weight=w1),
                        ops.gather_scatter("add", x, gi, si, size, edge_weight=w1.reshape(-1, 1)))
    assert tested >= 1      # (d = 3 and d = 20 with H = 2 give a dh that is not a multiple of 4)


@pytest.mark.parametrize("op", MODES)
def test_against_the_numpy_restatement(EA, torch_cuda, gen, op):
    """the GPU path against code that is not GPU code: one mid-sized case per mode"""
    torch = torch_cuda
    ops = EA.ops
    rows, size, e, d, H = 200, 64, 700, 24, 2
    x = draw(torch, gen, (rows, d), torch.float32)
    w = draw(torch, gen, (e, H), torch.float32, scale=4.0)
    gi = torch.randint(0, rows, (e,), generator=gen, device="cuda", dtype=torch.int32)
    si = torch.randint(0, size + 3, (e,), generator=gen, device="cuda", dtype=torch.int32)
    si[si == 5] = 6
    want = ref.gather_scatter_ref(op, x.cpu().numpy(), gi.cpu().numpy(), si.cpu().numpy(), size, w.cpu().numpy())
    got = ops.gather_scatter(op, x, gi, si, size, edge_weight=w)
    assert same(got, torch.from_numpy(want).cuda())
    count = 7
    gi2 = gi[:size * count]
    want = ref.gather_scatter_ref(op, x.cpu().numpy(), gi2.cpu().numpy(), ref.segment_dst(size, count=count), size,
                                  w[:size * count].cpu().numpy())
    got = ops.gather_segment_reduce(op, x, gi2, size, count=count, edge_weight=w[:size * count])
    assert same(got, torch.from_numpy(want).cuda())
    for S in (torch.bfloat16, torch.float16):
        xs, ws = x.to(S), w.to(S)
        want = ref.gather_scatter_ref(op, xs.float().cpu().numpy(), gi.cpu().numpy(), si.cpu().numpy(), size,
                                      ws.float().cpu().numpy())
        got = ops.gather_scatter(op, xs, gi, si, size, edge_weight=ws, out_dtype=torch.float32)
        assert same(got, torch.from_numpy(want).cuda())


def dot_bound(torch, a_rows, b_rows, heads, out_dtype=None):
    """float64 reference [E, H] and its bound: gamma * sum |a_c b_c| (+ half an ulp of a 16-bit
    out_dtype at the reference value)"""
    e, d = a_rows.shape
    dh = d // heads
    prod = a_rows.double() * b_rows.double()
    want = prod.view(e, heads, dh).sum(-1)
    gamma = dh * U / (1 - dh * U)
    bound = gamma * prod.abs().view(e, heads, dh).sum(-1)
    if out_dtype in (torch.bfloat16, torch.float16):
        mant, emin = (7, -126) if out_dtype == torch.bfloat16 else (10, -14)
        exp = torch.frexp(want.abs())[1].double() - 1            # floor(log2 |want|)
        exp = torch.clamp(exp, min=emin)
        bound = bound + 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64, device=want.device), exp - mant)
    return want, bound


def within(torch, got, want, bound):
    err = (got.double() - want).abs()
    return bool((err <= bound).all())


@pytest.mark.parametrize("op", MODES)
@pytest.mark.parametrize("form", ["scatter", "scatter_sorted", "count", "ptr", "ids"])
def test_gradients_meet_contracts_b_and_c(EA, torch_cuda, gen, op, form):
    torch = torch_cuda
    ops = EA.ops
    rows, size, count = 80, 30, 6
    e = size * count
    for d, H in ((8, 1), (20, 2), (64, 8), (3, 1), (8, 8)):
        dh = d // H
        gi = torch.randint(0, rows, (e,), generator=gen, device="cuda", dtype=torch.int32)
        si = torch.randint(0, size, (e,), generator=gen, device="cuda", dtype=torch.int32)
        if form == "scatter_sorted":
            si = torch.sort(si).values
        kw = {}
        if form in ("count", "ids"):
            si = torch.arange(size, device="cuda", dtype=torch.int32).repeat_interleave(count)
            kw = dict(count=count)
        if form == "ptr":
            lens = torch.randint(0, 13, (size,), generator=gen, device="cuda")
            lens[::7] = 0
            seg_ptr = torch.zeros(size + 1, dtype=torch.int64, device="cuda")
            seg_ptr[1:] = torch.cumsum(lens, 0)
            n_e = int(seg_ptr[-1])
            gi = torch.randint(0, rows, (n_e,), generator=gen, device="cuda", dtype=torch.int32)
            si = torch.repeat_interleave(torch.arange(size, device="cuda", dtype=torch.int32), lens)
            kw = dict(seg_ptr=seg_ptr)
        gi_in = gi
        if form == "ids":
            gi_in = gi.to(torch.int64).clone()
            gi_in[::11] = -1                                  # reads, and sends its gradient to, the last row
            gi = torch.clamp(gi_in & 0xFFFFFFFF, max=rows - 1).to(torch.int32)
        n_e = gi.numel()

        def fused(xx, ww, od=None):
            if form.startswith("scatter"):
                return ops.gather_scatter(op, xx, gi_in, si, size, out_dtype=od, edge_weight=ww)
            return ops.gather_segment_reduce(op, xx, gi_in, size, out_dtype=od, edge_weight=ww, **kw)

        x = draw(torch, gen, (rows, d), torch.float32)
        w = draw(torch, gen, (n_e, H), torch.float32, scale=4.0)
        g = draw(torch, gen, (size, d), torch.float32)
        # B: grad_params, bit for bit
        xf, wf = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        gx_f, gw_f = torch.autograd.grad(fused(xf, wf), (xf, wf), g)
        xc, wc = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        xg = ops.gather(xc, gi)
        msg = xg * expand(wc, d)
        msg.retain_grad()
        out_c = ops.scatter_(op, msg, si, size)
        assert same(fused(x, w), out_c.detach())
        out_c.backward(g)
        assert same(gx_f, xc.grad), (d, H)
        assert gw_f.shape == w.shape and gw_f.dtype == w.dtype
        # C: grad_edge_weight[p, h] = sum_c (d out / d msg)[p, c] * x[gi[p], c] over the head's columns
        want, bound = dot_bound(torch, msg.grad, xg.detach(), H)
        assert within(torch, gw_f, want, bound), (d, H)
        assert within(torch, wc.grad, want, bound)             # (and so is the composition's)
        if dh == 1:
            assert same(gw_f, (msg.grad * xg.detach()))
        # 16-bit storage: the fp32 gradients of the widened inputs, rounded once
        for S in (torch.bfloat16, torch.float16):
            for WS in (torch.float32, S):
                xs, ws = x.to(S), w.to(WS)
                x32, w32 = xs.float().requires_grad_(True), ws.float().requires_grad_(True)
                out32 = fused(x32, w32)
                for od in (S, torch.float32):
                    gs = g.to(od)
                    a, b = xs.clone().requires_grad_(True), ws.clone().requires_grad_(True)
                    out = fused(a, b, od)
                    assert out.dtype == od
                    ga, gb = torch.autograd.grad(out, (a, b), gs)
                    g32x, g32w = torch.autograd.grad(out32, (x32, w32), gs.float(), retain_graph=True)
                    assert ga.dtype == S and gb.dtype == WS and gb.shape == ws.shape
                    assert same(ga, g32x.to(S)), (S, WS, od)
                    assert same(gb, g32w.to(WS)), (S, WS, od)


@pytest.mark.parametrize("dh", [1, 3, 16, 64, 128, 512])
def test_edge_dot_meets_contract_c(EA, torch_cuda, gen, dh):
    torch = torch_cuda
    ops = EA.ops
    ra, rb, e = 150, 170, 1000
    for H in (1, 2, 8):
        d = H * dh
        ai = torch.randint(0, ra, (e,), generator=gen, device="cuda", dtype=torch.int32)
        bi = torch.randint(0, rb, (e,), generator=gen, device="cuda", dtype=torch.int32)
        for SA, SB in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                       (torch.float16, torch.float16), (torch.float32, torch.bfloat16),
                       (torch.float16, torch.float32)):
            for unaligned in (False, True):
                a = draw(torch, gen, (ra, d), SA, unaligned)
                b = draw(torch, gen, (rb, d), SB, unaligned)
                a_rows, b_rows = a.float()[ai.long()], b.float()[bi.long()]
                outs = [torch.float32] + [S for S in {SA, SB} if S != torch.float32]
                for od in outs:
                    got = ops.edge_dot(a, ai, b, bi, heads=H, out_dtype=od)
                    assert got.shape == (e, H) and got.dtype == od
                    want, bound = dot_bound(torch, a_rows, b_rows, H, od)
                    assert within(torch, got, want, bound), (H, SA, SB, od, unaligned)
                    assert same(got, ops.edge_dot(a, ai, b, bi, heads=H, out_dtype=od))      # run to run
                    # the bits do not depend on E or on the grid: a prefix of the edges, alone
                    assert same(got[:37], ops.edge_dot(a, ai[:37], b, bi[:37], heads=H, out_dtype=od))
                if dh == 1:
                    assert same(ops.edge_dot(a, ai, b, bi, heads=H, out_dtype=torch.float32), a_rows * b_rows)
        # no index: row p
        a = draw(torch, gen, (e, d), torch.float32)
        b = draw(torch, gen, (rb, d), torch.float32)
        assert same(ops.edge_dot(a, None, b, bi, heads=H),
                    ops.edge_dot(a, torch.arange(e, device="cuda", dtype=torch.int32), b, bi, heads=H))
        assert ops.edge_dot(a, None, b, bi, heads=H).dtype == torch.float32


@pytest.mark.parametrize("dh", [1, 3, 16, 64])
def test_edge_dot_gradients(EA, torch_cuda, gen, dh):
    """grad_a[r, c] = sum over the edges p with a_index[p] = r of grad[p, h] * b[b_index[p], c]: a
    sum of n_r fp32 products, compared with float64 under the bound of n_r terms; and with the
    gradient of the composition gather * gather -> sum, whose products are the same pairs."""
    torch = torch_cuda
    ops = EA.ops
    ra, rb, e, H = 40, 50, 600, 2
    d = H * dh
    ai = torch.randint(0, ra, (e,), generator=gen, device="cuda", dtype=torch.int32)
    bi = torch.randint(0, rb, (e,), generator=gen, device="cuda", dtype=torch.int32)
    for S in _dtypes(torch):
        a0, b0 = draw(torch, gen, (ra, d), S), draw(torch, gen, (rb, d), S)
        g = draw(torch, gen, (e, H), torch.float32)
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        ga, gb = torch.autograd.grad(ops.edge_dot(a, ai, b, bi, heads=H, out_dtype=torch.float32), (a, b), g)
        assert ga.dtype == S and gb.dtype == S
        gexp = expand(g, d).double()
        for got, idx, other, oidx, n_rows in ((ga, ai, b0, bi, ra), (gb, bi, a0, ai, rb)):
            terms = gexp * other.double()[oidx.long()]
            want = torch.zeros((n_rows, d), dtype=torch.float64, device="cuda").index_add_(0, idx.long(), terms)
            mag = torch.zeros((n_rows, d), dtype=torch.float64, device="cuda").index_add_(0, idx.long(), terms.abs())
            n = torch.bincount(idx.long(), minlength=n_rows).double().reshape(-1, 1)
            bound = n * U / (1 - n * U) * mag
            if S != torch.float32:
                mant, emin = (7, -126) if S == torch.bfloat16 else (10, -14)
                exp = torch.clamp(torch.frexp(want.abs())[1].double() - 1, min=emin)
                bound = bound + 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64, device="cuda"), exp - mant)
            assert within(torch, got, want, bound), (S, dh)
        if S == torch.float32:
            ac, bc = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            comp = (ops.gather(ac, ai) * ops.gather(bc, bi)).view(e, H, dh).sum(-1)
            comp.backward(g)
            assert same(ga, ac.grad) and same(gb, bc.grad)


def test_errors(EA, torch_cuda, gen):
    torch = torch_cuda
    ops = EA.ops
    x = draw(torch, gen, (10, 12), torch.float32)
    idx = torch.zeros(6, dtype=torch.int32, device="cuda")
    w = torch.ones((6, 1), device="cuda")
    calls = [lambda xx, ww: ops.gather_scatter("add", xx, idx, idx, 2, edge_weight=ww),
             lambda xx, ww: ops.gather_segment_reduce("mean", xx, idx, 2, count=3, edge_weight=ww)]
    for call in calls:
        with pytest.raises(ValueError):
            call(x, torch.ones((6, 5), device="cuda"))                  # 5 does not divide 12
        with pytest.raises(ValueError):
            call(x, torch.ones((7, 1), device="cuda"))                  # one weight row per edge
        with pytest.raises(ValueError):
            call(x, torch.ones((6, 1, 1), device="cuda"))
        with pytest.raises(TypeError):
            call(x, torch.ones((6, 1), device="cuda", dtype=torch.int64))
        with pytest.raises(TypeError):
            call(x, torch.ones((6, 1), device="cuda", dtype=torch.float64))
        with pytest.raises(TypeError):
            call(x, torch.ones((6, 1), device="cuda", dtype=torch.bfloat16))      # neither fp32 nor x's dtype
        with pytest.raises(TypeError):
            call(x.to(torch.float16), torch.ones((6, 1), device="cuda", dtype=torch.bfloat16))
        with pytest.raises(RuntimeError):
            call(x, torch.ones((6, 1)))                                  # a CPU tensor
        with pytest.raises(RuntimeError):
            call(x.cpu(), w)
    with pytest.raises(ValueError):
        ops.edge_dot(x, idx, x, idx, heads=5)
    with pytest.raises(ValueError):
        ops.edge_dot(x, idx, x[:, :8], idx)
    with pytest.raises(ValueError):
        ops.edge_dot(x, idx, x, idx[:3])
    with pytest.raises(TypeError):
        ops.edge_dot(x.double(), idx, x, idx)
    with pytest.raises(TypeError):
        ops.edge_dot(x, idx, x, idx, out_dtype=torch.float64)
    with pytest.raises(RuntimeError):
        ops.edge_dot(x.cpu(), idx, x, idx)
    # the raw C entries: EULER_GPU_EINVAL, and nothing touched for size == 0 / d == 0
    L = EA._lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    out = torch.full((2, 12), 7.0, device="cuda")
    EINVAL = EA._lib.EINVAL
    assert L.euler_gpu_gather_scatter_w(None, 0, p(x), p(idx), p(idx), 6, 12, 2, p(out), p(w), 0) == EINVAL
    assert b"heads" in L.euler_gpu_last_error()
    assert L.euler_gpu_gather_scatter_w(None, 0, p(x), p(idx), p(idx), 6, 12, 2, p(out), p(w), 5) == EINVAL
    assert L.euler_gpu_gather_scatter_w(None, 0, p(x), p(idx), p(idx), 6, 12, 2, p(out), None, 1) == EINVAL
    assert b"null" in L.euler_gpu_last_error()
    assert L.euler_gpu_gather_scatter_w(None, 0, p(x), p(idx), p(idx), 1 << 31, 12, 2, p(out), p(w), 1) == EINVAL
    assert L.euler_gpu_gather_scatter_w(None, 2, p(x), p(idx), p(idx), 1 << 24, 12, 2, p(out), p(w), 1) == EINVAL
    assert L.euler_gpu_gather_scatter_w(None, 3, p(x), p(idx), p(idx), 6, 12, 2, p(out), p(w), 1) == EINVAL
    assert L.euler_gpu_gather_segment_reduce_w(None, 0, p(x), p(idx), None, 3, 12, 2, p(out), p(w), 7) == EINVAL
    assert L.euler_gpu_gather_segment_reduce_w(None, 2, p(x), p(idx), None, 1 << 24, 12, 2, p(out), p(w), 1) == EINVAL
    assert L.euler_gpu_gather_segment_reduce_ids_w(None, 0, p(x), 10, None, None, 3, 12, 2, p(out), p(w), 1) == EINVAL
    assert L.euler_gpu_gather_scatter_w_t(None, 0, p(x), 1, p(idx), p(idx), 6, 12, 2, p(out), 1, p(w), 2, 1) == EINVAL
    assert b"w_dtype" in L.euler_gpu_last_error()
    assert L.euler_gpu_edge_dot(None, p(x), p(idx), p(x), p(idx), 6, 12, 5, p(out)) == EINVAL
    assert L.euler_gpu_edge_dot(None, p(x), p(idx), p(x), p(idx), 6, 12, 0, p(out)) == EINVAL
    assert L.euler_gpu_edge_dot(None, None, p(idx), p(x), p(idx), 6, 12, 1, p(out)) == EINVAL
    assert L.euler_gpu_edge_dot_t(None, p(x), 5, p(idx), p(x), 0, p(idx), 6, 12, 1, p(out), 0) == EINVAL
    assert L.euler_gpu_gather_scatter_w(None, 0, p(x), p(idx), p(idx), 6, 12, 0, p(out), p(w), 1) == 0
    assert L.euler_gpu_gather_scatter_w(None, 0, p(x), p(idx), p(idx), 6, 0, 2, p(out), p(w), 1) == 0
    assert L.euler_gpu_edge_dot(None, p(x), p(idx), p(x), p(idx), 0, 12, 1, p(out)) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("op", MODES)
def test_without_a_weight_nothing_changes(EA, torch_cuda, gen, op):
    torch = torch_cuda
    ops = EA.ops
    rows, size, count, d = 100, 40, 5, 24
    e = size * count
    x = draw(torch, gen, (rows, d), torch.float32)
    gi = torch.randint(0, rows, (e,), generator=gen, device="cuda", dtype=torch.int32)
    si = torch.randint(0, size, (e,), generator=gen, device="cuda", dtype=torch.int32)
    want = ops.scatter_(op, ops.gather(x, gi), si, size)
    assert same(ops.gather_scatter(op, x, gi, si, size), want)
    assert same(ops.gather_scatter(op, x, gi, si, size, edge_weight=None), want)
    dst = torch.arange(size, device="cuda", dtype=torch.int32).repeat_interleave(count)
    want = ops.scatter_(op, ops.gather(x, gi), dst, size)
    assert same(ops.gather_segment_reduce(op, x, gi, size, count=count, edge_weight=None), want)
    if op != "max":     # a weight of ones is the unweighted op (x * 1 = x)
        assert same(ops.gather_scatter(op, x, gi, si, size, edge_weight=torch.ones(e, device="cuda")),
                    ops.gather_scatter(op, x, gi, si, size))


def test_gcn_example_equals_the_composition(EA, torch_cuda):
    torch = torch_cuda
    spec = importlib.util.spec_from_file_location(
        "gcn_minibatch", os.path.join(ROOT, "examples", "python", "gcn_minibatch.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    G = EA.Graph.load(os.path.join(ROOT, "tests", "golden", "fixture_dat"))
    max_id = int(G.id_range()[0])
    roots = torch.arange(1, min(max_id, 6) + 1, device="cuda", dtype=torch.int64)
    fused = ex.run(G, roots, 8)
    composed = ex.run(G, roots, 8, composed=True)
    assert fused.shape == (roots.numel(), 8) and float(fused.abs().sum()) > 0
    assert same(fused, composed)
    # block by block, with the normalisation of gcn_conv.py:33-40 written out
    flow = ex.GCNDataFlow(G, [[0, 1], [0, 1]], add_self_loops=True)
    df = flow(roots)
    x = G.get_dense_feature(df[0].n_id, [0], [8])[0]
    for blk in df:
        dst, src = blk.edge_index[0], blk.edge_index[1]
        ones = torch.ones((dst.numel(), 1), device="cuda")
        norm_i = EA.ops.scatter_add(ones, dst, blk.size[0]) ** -0.5
        norm_j = EA.ops.scatter_add(ones, src, blk.size[1]) ** -0.5
        want = EA.ops.scatter_add(norm_i[dst.long()] * norm_j[src.long()] * x[src.long()], dst, blk.size[0])
        got = ex.aggregate(x, blk)
        assert same(got, want)
        x = got
